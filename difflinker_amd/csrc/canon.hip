// canon.hip — canonical atom ranks and a canonical 64-bit code of the bond graphs bonds.hip left on the device: an
// individualisation-refinement search over the colour refinement of mol_keys.hip.  Where the key of dl_molecule_keys is 1-WL
// (cubane and cuneane share it), the search below labels the atoms, so equal codes mean equal graphs up to a 64-bit hash of
// the labelled form, and the ranks give molecule_builder.smiles its atom order.  The reference asks RDKit for canonical
// SMILES (src/metrics.py:12-54); this is the project's own rule, NOT RDKit's ranks.
//
// One 256-thread workgroup per molecule, one launch per batch, reading what dl_perceive_bonds wrote for the same batch, with
// the conventions of mol_graph.h: atom k is the k-th row with node_mask != 0; drop_mask removes atoms after that numbering
// together with every bond that touches them.  At most DL_CANON_MAX_ATOMS = 256 KEPT atoms (N may be 1024) and
// DL_CANON_MAX_BONDS kept list entries.  Thread i owns kept atom i throughout.
//
// THE RULE is written down in include/difflinker_hip.h and restated in tests/canon_ref.py; the kernel agrees with that in
// every output bit.  In short: refine(c) is n rounds of c'[i] = mix2(c[i], sum over the kept bonds of mix2(c[j], order));
// rank[i] counts the strictly smaller colours; a node whose ranks are distinct is a leaf; any other node takes its tied cell
// of smallest rank and individualises its members in ascending kept index (only the lowest one when the cell is a twin cell
// or the path already has DL_CANON_MAX_DEPTH branching levels); the leaf with the smallest code wins.
//
// LDS (static, 27 KiB): two colour buffers (4 KiB), the map from atom number to kept index (4 KiB), the CSR adjacency as
// 16-bit entries neighbour | order << 8 (8 KiB) with one row end per atom (1 KiB), type / current rank / best rank as bytes,
// and one saved rank vector per branching level (32 x 256 B).
//
//   stage    rows numbered (number_rows of mol_graph.h); s_map[atom] = kept index or -1; the type by kept index
//   count    one thread per list entry: LDS add on both ends' degree;  scan: row starts;  fill: an LDS add on the row's
//            cursor gives the slot (the order inside a row is free: the rounds and the leaf code only sum over it)
//   repeat   thread i walks row i with a 256-bit set in registers: a neighbour met twice is a repeated pair (BAD_BOND)
//   refine   n rounds, one gather per atom and one barrier per round
//   rank     thread i compares colour i with all n colours (every lane reads the same LDS word: a broadcast), and counts
//            the equal ones as well: an atom with an equal partner is tied
//   control  ONE minimum over rank << 8 | index of the tied atoms gives the cell and its lowest member; one min/max over the
//            members' only CSR entry is the twin test; the next member on backtracking is a minimum again.  Every value that
//            steers the search is the result of a workgroup reduction, hence the same in every thread; the stack's cell and
//            member words are written by thread 0 and read only after later barriers
//   leaf     two block_sums of 64-bit partials
//
// Global memory is written with plain vector stores only; no global atomics of any kind; every output element is written.
#include "mol_graph.h"

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = DL_CANON_MAX_ATOMS;
constexpr int MAX_ADJ = 2 * DL_CANON_MAX_BONDS;  // CSR entries
constexpr int MAX_DEPTH = DL_CANON_MAX_DEPTH;
constexpr int NONE = 0x7fffffff;
static_assert(MAX_KEPT == WG && MAX_KEPT == MATRIX_ATOMS, "one thread per kept atom, ranks and neighbours fit a byte");

struct Canon {
    u64* col0;                                   // [MAX_KEPT] the colours a refinement starts from
    u64* col1;
    const unsigned short* adj;                   // [MAX_ADJ] neighbour | order << 8
    const int* end;                              // [MAX_KEPT] row i is [end[i - 1], end[i])
    unsigned char* rank;                         // [MAX_KEPT] the current node's ranks
    int* red;                                    // [2 * WG_WAVES] the reductions' words
    int n;
};

// minimum of `lo` and maximum of `hi` over the workgroup in one pass; the same in every thread
__device__ __forceinline__ void block_min_max(int& lo, int& hi, int* lds /* [2 * WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        lds[threadIdx.x >> 6] = lo;
        lds[WG_WAVES + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = lds[0];
    hi = lds[WG_WAVES];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) {
        lo = min(lo, lds[k]);
        hi = max(hi, lds[WG_WAVES + k]);
    }
    __syncthreads();
}

// individualise `v` on the ranks `from`, refine for n rounds, rank.  Returns rank << 8 | index of the lowest member of the
// tied cell of smallest rank, or NONE when the ranks are all distinct.  Ends with a barrier after its last LDS access
__device__ __forceinline__ int refine_and_rank(const Canon& g, const unsigned char* from, int v, const unsigned char* type) {
    const int tid = threadIdx.x, n = g.n;
    const bool atom = tid < n;
    const int lo = (atom && tid) ? g.end[tid - 1] : 0, hi = atom ? g.end[tid] : 0;
    if (atom) g.col0[tid] = from ? mix2(SEED_COLOUR, u64(2 * from[tid] + (tid == v ? 0 : 1))) : mix2(SEED_COLOUR, u64(type[tid] + 1));
    __syncthreads();
    u64* cur = g.col0;
    u64* nxt = g.col1;
    for (int r = 0; r < n; ++r) {
        if (atom) {
            u64 s = 0;
            for (int p = lo; p < hi; ++p) {
                const int e = g.adj[p];
                s += mix2(cur[e & 0xFF], u64(e >> 8));
            }
            nxt[tid] = mix2(cur[tid], s);
        }
        __syncthreads();
        u64* t = cur; cur = nxt; nxt = t;
    }
    int packed = NONE;
    if (atom) {
        const u64 c = cur[tid];
        int less = 0, equal = 0;
        for (int j = 0; j < n; ++j) {
            const u64 cj = cur[j];
            less += cj < c;
            equal += cj == c;
        }
        g.rank[tid] = (unsigned char)less;
        if (equal > 1) packed = less << 8 | tid;
    }
    return block_min(packed, g.red);
}

__global__ __launch_bounds__(WG) void canonical_ranks_kernel(dl_canon_args a) {
    __shared__ u64 s_col0[MAX_KEPT], s_col1[MAX_KEPT];
    __shared__ long long s_sum[WG_WAVES];
    __shared__ int s_map[MAX_ROWS];
    __shared__ int s_end[MAX_KEPT];
    __shared__ int s_deg[MAX_KEPT];
    __shared__ int s_cell[MAX_DEPTH], s_member[MAX_DEPTH];
    __shared__ int s_red[2 * WG_WAVES];
    __shared__ unsigned short s_adj[MAX_ADJ];
    __shared__ unsigned char s_type[MAX_KEPT], s_rank[MAX_KEPT], s_best[MAX_KEPT];
    __shared__ unsigned char s_saved[MAX_DEPTH][MAX_KEPT];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity;

    // ---- stage: number the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_red);
    const int n_real = rn.n, n = rn.n_kept;
    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb;
    int* rank_out = a.rank + size_t(b) * N;

    if (n > MAX_KEPT) {                          // uniform over the workgroup
        for (int i = tid; i < N; i += WG) rank_out[i] = -1;
        if (tid == 0) {
            a.code[b] = 0;
            a.n_leaves[b] = 0;
            a.status[b] = in.status | DL_CANON_TOO_LARGE;
        }
        return;
    }

    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? kk : -1;
        if (kept) s_type[kk] = (unsigned char)first_maximum(a.one_hot + (size_t(b) * N + r) * nf, nf);
    });
    s_deg[tid] = 0;
    __syncthreads();

    // ---- count: the degrees over the kept entries
    const int* list = a.bonds + size_t(b) * capacity * 3;       // never read when nb == 0
    int bad = 0, mine = 0;
    Bond bd;
    for (int e = tid; e < nb; e += WG) {
        if (!load_bond(list, e, n_real, bd, bad)) continue;
        const int u = s_map[bd.i], v = s_map[bd.j];
        if ((u | v) < 0) continue;                               // an end is dropped: no bond of this graph, and no error
        atomicAdd(&s_deg[u], 1);
        atomicAdd(&s_deg[v], 1);
        ++mine;
    }
    bad = __syncthreads_or(bad);
    const int n_bonds = block_sum(mine, s_red);
    if (2 * n_bonds > MAX_ADJ) {                 // uniform: the adjacency does not hold this molecule
        for (int i = tid; i < N; i += WG) rank_out[i] = -1;
        if (tid == 0) {
            a.code[b] = 0;
            a.n_leaves[b] = 0;
            a.status[b] = in.status | DL_CANON_TOO_LARGE | (bad ? DL_CANON_BAD_BOND : 0);
        }
        return;
    }

    // ---- scan and fill: thread i owns row i
    int n_adj = 0;
    const int start = block_exclusive_scan(tid < n ? s_deg[tid] : 0, s_red, n_adj);
    s_end[tid] = start;
    __syncthreads();
    int unused = 0;
    for (int e = tid; e < nb; e += WG) {
        if (!load_bond(list, e, n_real, bd, unused)) continue;
        const int u = s_map[bd.i], v = s_map[bd.j];
        if ((u | v) < 0) continue;
        const int pu = atomicAdd(&s_end[u], 1), pv = atomicAdd(&s_end[v], 1);
        if (pu < MAX_ADJ) s_adj[pu] = (unsigned short)(v | bd.order << 8);      // the bounds never bind: the cursors stay
        if (pv < MAX_ADJ) s_adj[pv] = (unsigned short)(u | bd.order << 8);      // inside the rows the scan laid out
    }
    __syncthreads();

    // ---- repeat: a neighbour twice in one row
    int repeated = 0;
    if (tid < n) {
        u64 seen[MATRIX_WORDS] = {0, 0, 0, 0};
        for (int p = start; p < s_end[tid]; ++p) {
            const int w = s_adj[p] & 0xFF;
#pragma unroll
            for (int q = 0; q < MATRIX_WORDS; ++q) {
                const u64 one = bit_in_word(w, q);
                repeated |= (seen[q] & one) != 0;
                seen[q] |= one;
            }
        }
    }
    bad |= __syncthreads_or(repeated);

    // ---- the search
    const Canon g{s_col0, s_col1, s_adj, s_end, s_rank, s_red, n};
    const bool atom = tid < n;
    const int row_hi = atom ? s_end[tid] : 0;
    const int max_leaves = a.max_leaves;
    int depth = 0, leaves = 0, budget = 0;
    u64 best = 0;
    int packed = refine_and_rank(g, nullptr, 0, s_type);
    for (;;) {
        // descend to a leaf: every step splits a cell, so there are fewer than n of them (the bound only guards the loop
        // against a collision of two 64-bit colours, which could merge cells again)
        for (int step = 0; packed != NONE; ++step) {
            if (step >= n) { budget = 1; break; }
            const int cell = packed >> 8, v = packed & 0xFF;
            const bool member = atom && s_rank[tid] == cell;
            int lo = NONE, hi = -1;
            if (member) lo = hi = (row_hi - start == 1) ? int(s_adj[start]) : 0x10000 + tid;
            block_min_max(lo, hi, s_red);
            if (lo != hi) {                      // no twin cell (two members with no single bond differ by their index)
                if (depth >= MAX_DEPTH) {
                    budget = 1;
                } else {
                    s_saved[depth][tid] = s_rank[tid];
                    if (tid == 0) { s_cell[depth] = cell; s_member[depth] = v; }
                    ++depth;
                }
            }
            packed = refine_and_rank(g, s_rank, v, s_type);
        }

        // the leaf's code
        ++leaves;
        u64 pa = 0, pb = 0;
        if (atom) {
            const u64 ri = s_rank[tid];
            pa = mix2(ri, u64(s_type[tid] + 1));
            for (int p = start; p < row_hi; ++p) {
                const int e = s_adj[p], w = e & 0xFF;
                if (w <= tid) continue;          // every entry once, from its lower end
                const u64 rj = s_rank[w];
                pb += mix2(mix2(ri < rj ? ri : rj, ri < rj ? rj : ri), u64(e >> 8));
            }
        }
        const u64 sa = u64(block_sum((long long)pa, s_sum)), sb = u64(block_sum((long long)pb, s_sum));
        const u64 code = mix2(mix2(SEED_KEY, sa), sb);
        if (leaves == 1 || code < best) {
            best = code;
            s_best[tid] = s_rank[tid];
        }

        // backtrack to the deepest level with a member left
        int next = NONE, d = 0;
        while (depth > 0) {
            d = depth - 1;
            const int cell = s_cell[d], m = s_member[d];
            next = block_min((atom && tid > m && s_saved[d][tid] == cell) ? tid : NONE, s_red);
            if (next != NONE) break;
            --depth;
        }
        if (depth == 0) break;
        if (leaves >= max_leaves) { budget = 1; break; }
        if (tid == 0) s_member[d] = next;        // read again only behind the barriers of the next refinement
        packed = refine_and_rank(g, s_saved[d], next, s_type);
    }
    __syncthreads();

    for (int i = tid; i < N; i += WG) rank_out[i] = (i < n_real && s_map[i] >= 0) ? int(s_best[s_map[i]]) : -1;
    if (tid == 0) {
        a.code[b] = best;
        a.n_leaves[b] = leaves;
        a.status[b] = in.status | (bad ? DL_CANON_BAD_BOND : 0) | (budget ? DL_CANON_BUDGET : 0);
    }
}

}  // namespace

extern "C" {

int32_t dl_canonical_ranks(const dl_canon_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->nf > 256 || a->capacity < 0 || a->max_leaves < 1 ||
        a->max_leaves > DL_CANON_MAX_LEAVES)
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->node_mask || !a->n_bonds_in || !a->status_in || !a->rank || !a->code || !a->n_leaves || !a->status ||
        (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(canonical_ranks_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
