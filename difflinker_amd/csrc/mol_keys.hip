// mol_keys.hip — scores of the bond graphs bonds.hip left on the device: atoms over their valence limit, pieces, and a
// 64-bit key per molecule that does not change when its atoms are renumbered (colour refinement, 1-WL).  The questions
// the reference puts to RDKit (src/metrics.py:12-54: sanitisation, GetMolFrags, canonical SMILES) asked of the graph.
//
// One 256-thread workgroup per molecule, one launch per batch, reading what dl_perceive_bonds wrote for the same batch.
// Atoms are numbered as bonds.hip numbers them (the k-th row with node_mask != 0).  drop_mask (the reference's pocket_mask)
// removes atoms after that numbering; a bond counts when both its atoms are kept.
//
// THE MIXING FUNCTION AND THE ROUNDS (written down here; mol_graph.h holds the code, include/difflinker_hip.h quotes it and
// tests/mol_keys_ref.py restates it).  All arithmetic is on 64-bit unsigned integers, modulo 2^64.
//   mix64(z)   z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
//              return z ^ z >> 31                                              (the splitmix64 finaliser)
//   mix2(a, b) mix64(a + b * 0xD6E8FEB86659FD93)
//   c_0[i]     mix2(0x243F6A8885A308D3, type_i + 1)
//   c_r+1[i]   mix2(c_r[i], sum over the kept bonds (i, j, order) of mix2(c_r[j], order))
//   rounds     exactly n_atoms (kept atoms): colour refinement of n atoms settles within n rounds, and a count that depends
//              on n_atoms alone is the same under every renumbering.  No settle test, so no sort and no class count.
//   key        mix2(mix2(mix2(0x13198A2E03707344, n_atoms), n_bonds), sum over the kept atoms of mix64(c_final[i]))
// The sums are commutative, so neither the order of the bond list nor the order in which LDS atomics land can change a bit.
//
// LDS: EIGHT words per atom (two 64-bit colour buffers = 4, type and keep flag, degree and valence, CSR row end, component
// label; 1024 atoms: 32 KiB) plus one word per CSR entry, two entries per kept bond (neighbour | order << 10), at most what
// is left of 60 KiB (1024 atoms: 7168 entries, 3.5 bonds per atom; 292 atoms: 12 per atom).  A molecule beyond either limit
// gets DL_KEYS_TOO_LARGE and a zero key.
//
//   stage   real rows compacted in row order (number_rows of mol_graph.h); type = first maximum of the one-hot row
//   count   one thread per list entry: degree and valence of both atoms by integer LDS adds (one packed word)
//   label   with drop_mask only: min-label propagation and pointer jumping as in bonds.hip, over the list instead of over
//           all pairs; without it n_components is taken as given
//   scan    exclusive prefix sum of the degrees -> CSR row starts;  fill: an LDS add on the row's cursor gives the slot
//   round   one gather per atom: its row of the CSR, the neighbours' colours from the buffer of the round before
//
// Global memory is written with plain vector stores only; no global atomics of any kind.
#include "mol_graph.h"

namespace {

constexpr int MAX_ATOMS = 1024;
constexpr int MAX_TYPES = 16;
constexpr int WORDS_PER_ATOM = 8;
constexpr size_t LDS_BUDGET = 60 * 1024;         // dynamic LDS; the static arrays below take under 4 KiB of the 64 KiB

constexpr int KEEP = 1 << 8;                     // s_tk: type | KEEP

__global__ __launch_bounds__(WG) void molecule_keys_kernel(dl_mol_keys_args a, int atoms_lds, int adj_cap) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int s_scan[WG_WAVES];
    __shared__ int s_maxval[MAX_TYPES];
    __shared__ u64 s_part[WG];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf;
    u64* s_col0 = reinterpret_cast<u64*>(lds_raw);
    u64* s_col1 = s_col0 + atoms_lds;
    int* s_tk = reinterpret_cast<int*>(s_col1 + atoms_lds);   // type | KEEP
    int* s_dv = s_tk + atoms_lds;                // degree | valence << 16, over the kept bonds
    int* s_end = s_dv + atoms_lds;               // CSR: the row's start, after the fill its end (= the next row's start)
    int* s_label = s_end + atoms_lds;
    int* s_adj = s_label + atoms_lds;            // [adj_cap]: neighbour | order << 10

    if (tid < nf) s_maxval[tid] = a.max_valence[tid];

    // ---- stage: compact the real rows
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;
    const int status_in = a.status_in[b];
    uint64_t* colour = a.colour + size_t(b) * N;

    if (n > MAX_ATOMS) {                         // uniform over the workgroup: nothing below fits
        for (int i = tid; i < N; i += WG) colour[i] = 0;
        if (tid == 0) {
            a.n_atoms[b] = n_kept;
            a.n_over[b] = 0;
            a.n_components[b] = 0;
            a.n_bonds[b] = 0;
            a.key[b] = 0;
            a.status[b] = status_in | DL_KEYS_TOO_LARGE;
        }
        return;
    }

    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int) {
        s_tk[k] = first_maximum(a.one_hot + (size_t(b) * N + r) * nf, nf) | (kept ? KEEP : 0);
    });
    for (int i = tid; i < n; i += WG) { s_dv[i] = 0; s_label[i] = i; }
    __syncthreads();

    // ---- count: degree and valence over the kept bonds
    const int nb = bonds_in(a.n_bonds_in, nullptr, b, a.capacity).nb;   // status_in passes through as it is: no overflow bit here
    const int* list = a.bonds + size_t(b) * a.capacity * 3;
    int bad = 0, mine_bonds = 0;
    Bond bd;
    for (int e = tid; e < nb; e += WG) {
        if (!load_bond(list, e, n, bd, bad) || !(s_tk[bd.i] & s_tk[bd.j] & KEEP)) continue;
        atomicAdd(&s_dv[bd.i], 1 | (bd.order << 16));
        atomicAdd(&s_dv[bd.j], 1 | (bd.order << 16));
        ++mine_bonds;
    }
    bad = __syncthreads_or(bad);
    const int n_bonds = block_sum(mine_bonds, s_scan);

    // ---- label: pieces of the graph over the kept atoms (labels of dropped atoms are never touched)
    int n_comp = 0;
    if (drop) {
        for (;;) {
            int changed = 0, unused = 0;
            for (int e = tid; e < nb; e += WG) {
                if (!load_bond(list, e, n, bd, unused) || !(s_tk[bd.i] & s_tk[bd.j] & KEEP)) continue;
                const int li = s_label[bd.i], lj = s_label[bd.j];
                if (li != lj) {
                    changed = 1;
                    atomicMin(li < lj ? &s_label[bd.j] : &s_label[bd.i], min(li, lj));
                }
            }
            __syncthreads();
            for (int i = tid; i < n; i += WG) {
                const int l = s_label[i], ll = s_label[l];
                if (ll != l) { s_label[i] = ll; changed = 1; }      // ll <= l: concurrent jumps only lower labels further
            }
            if (!__syncthreads_or(changed)) break;
        }
        int roots = 0;
        for (int i = tid; i < n; i += WG) roots += (s_tk[i] & KEEP) && s_label[i] == i;
        n_comp = block_sum(roots, s_scan);
    } else {
        n_comp = a.n_components_in[b];
    }

    // ---- valence rule: with every atom kept the valence of bonds.hip holds (also for a list its capacity cut short)
    int over = 0;
    for (int i = tid; i < n; i += WG) {
        if (!(s_tk[i] & KEEP)) continue;
        const int v = drop ? (s_dv[i] >> 16) : a.valence_in[size_t(b) * N + i];
        over += v > s_maxval[s_tk[i] & 0xFF];
    }
    const int n_over = block_sum(over, s_scan);

    // ---- scan: CSR row starts (thread t owns the contiguous atoms [t * pa, t * pa + pa))
    const int pa = (n + WG - 1) / WG;
    const int a0 = tid * pa;
    int sum = 0;
    for (int q = 0; q < pa; ++q)
        if (a0 + q < n) sum += s_dv[a0 + q] & 0xFFFF;
    int n_adj = 0;
    int at = block_exclusive_scan(sum, s_scan, n_adj);
    for (int q = 0; q < pa; ++q)
        if (a0 + q < n) { s_end[a0 + q] = at; at += s_dv[a0 + q] & 0xFFFF; }
    __syncthreads();
    const bool too_large = n_adj > adj_cap;      // uniform

    u64* cur = s_col0;
    u64* nxt = s_col1;
    u64 key = 0;
    if (!too_large) {
        // ---- fill: the slot of an entry is the row's cursor; the order inside a row is free, the rounds only sum over it
        int unused = 0;
        for (int e = tid; e < nb; e += WG) {
            if (!load_bond(list, e, n, bd, unused) || !(s_tk[bd.i] & s_tk[bd.j] & KEEP)) continue;
            const int pi = atomicAdd(&s_end[bd.i], 1), pj = atomicAdd(&s_end[bd.j], 1);
            if (pi < n_adj) s_adj[pi] = bd.j | (bd.order << 10);
            if (pj < n_adj) s_adj[pj] = bd.i | (bd.order << 10);
        }
        for (int i = tid; i < n; i += WG) {
            cur[i] = (s_tk[i] & KEEP) ? mix2(SEED_COLOUR, u64((s_tk[i] & 0xFF) + 1)) : 0;
            nxt[i] = 0;
        }
        __syncthreads();

        // ---- rounds: n_kept of them, one gather per atom
        for (int r = 0; r < n_kept; ++r) {
            for (int i = tid; i < n; i += WG) {
                if (!(s_tk[i] & KEEP)) continue;
                const int lo = i ? s_end[i - 1] : 0, hi = min(s_end[i], n_adj);
                u64 s = 0;
                for (int p = lo; p < hi; ++p) {
                    const int e = s_adj[p];
                    s += mix2(cur[min(e & 1023, n - 1)], u64(e >> 10));     // the clamp never binds for a list of distinct bonds
                }
                nxt[i] = mix2(cur[i], s);
            }
            __syncthreads();
            u64* t = cur; cur = nxt; nxt = t;
        }

        u64 part = 0;
        for (int i = tid; i < n; i += WG)
            if (s_tk[i] & KEEP) part += mix64(cur[i]);
        s_part[tid] = part;
        __syncthreads();
        if (tid == 0) {
            u64 total = 0;
            for (int t = 0; t < WG; ++t) total += s_part[t];
            key = mix2(mix2(mix2(SEED_KEY, u64(n_kept)), u64(n_bonds)), total);
        }
    }

    for (int i = tid; i < N; i += WG) colour[i] = (i < n && !too_large) ? cur[i] : 0;
    if (tid == 0) {
        a.n_atoms[b] = n_kept;
        a.n_over[b] = n_over;
        a.n_components[b] = n_comp;
        a.n_bonds[b] = n_bonds;
        a.key[b] = key;
        a.status[b] = status_in | (too_large ? DL_KEYS_TOO_LARGE : 0) | (bad ? DL_KEYS_BAD_BOND : 0);
    }
}

}  // namespace

extern "C" {

int32_t dl_molecule_keys(const dl_mol_keys_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > (1 << 20) || a->nf < 1 || a->nf > MAX_TYPES || a->capacity < 0) return DL_ERR_BAD_ARG;
    if (a->max_valence_len != a->nf) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->node_mask || !a->n_bonds_in || !a->valence_in || !a->n_components_in || !a->status_in ||
        !a->max_valence || !a->n_atoms || !a->n_over || !a->n_components || !a->n_bonds || !a->key || !a->colour || !a->status ||
        (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    const int atoms_lds = a->N < MAX_ATOMS ? a->N : MAX_ATOMS;
    const size_t atom_bytes = size_t(WORDS_PER_ATOM) * 4 * atoms_lds;
    const long long pairs = (long long)atoms_lds * (atoms_lds - 1) / 2;
    const long long want = 2 * (a->capacity < pairs ? (long long)a->capacity : pairs);
    const long long room = (long long)((LDS_BUDGET - atom_bytes) / 4);
    const int adj_cap = int(want < room ? want : room);
    hipLaunchKernelGGL(molecule_keys_kernel, dim3(a->B), dim3(WG), atom_bytes + size_t(adj_cap) * 4, static_cast<hipStream_t>(stream),
                       *a, atoms_lds, adj_cap);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
