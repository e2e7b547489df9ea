// rings.hip — ring perception of the bond graphs bonds.hip left on the device: for every bond the size of the smallest ring
// through it, for every atom the smallest ring it lies in, the number of pieces and the cyclomatic number.  What the
// reference asks of RDKit's ring perception (compute_metrics.py:128-145, CalcNumRings of the linker) asked of the graph.
//
// One 256-thread workgroup per molecule, one launch per batch, reading what dl_perceive_bonds wrote for the same batch, with
// the conventions of mol_keys.hip: atom k is the k-th row with node_mask != 0; drop_mask removes atoms after that numbering
// together with every bond that touches them; an entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and
// 1 <= order <= 3, in either orientation; anything else is skipped and sets DL_RINGS_BAD_BOND.  mark_mask marks atoms (the
// callers pass the linker): the second histogram row counts the bonds with a marked end.
//
// At most DL_RINGS_MAX_ATOMS = 256 KEPT atoms (N itself may be 1024: pocket rows are dropped, not counted).  The graph over
// the kept atoms is a 256 x 256 bit matrix in LDS, four 64-bit words per row.
//
//   stage   real rows ranked in row order (the scan of mol_keys.hip), kept rows ranked among themselves; s_map[atom] is the
//           kept index | MARK, or -1 for a dropped atom
//   build   one thread per list entry: LDS atomicOr of bit (lo, hi) and bit (hi, lo).  The old value of the first says
//           whether the pair was there already: exactly one entry of each distinct pair sees it unset, whatever the order, so
//           the count of those is n_bonds and the OR of the others is "a pair is repeated"
//   label   thread i owns kept atom i: the smallest label among its row's neighbours, then one pointer jump, until nothing
//           changes.  Reads and writes of a round are separated by barriers; the fixed point (every atom labelled with the
//           smallest index of its piece) is unique
//   search  one thread per list entry (u, v): a level-synchronous breadth-first search from u with frontier and visited set
//           as four 64-bit words each in registers.  v is masked out of u's row at level 0 only - the bond can be walked
//           nowhere else, because u is visited from the start - and the search ends when a level contains v (the ring has
//           level + 1 atoms) or is empty (a bridge: 0).  Each search reads the matrix only, so its answer depends on no other
//           lane; the per-atom minimum and the histograms are LDS integer atomics (min and add: commutative)
//
// LDS: 8 KiB matrix + 4 KiB map + 2 KiB labels and per-atom minima + the histograms: 14.4 KiB, static.  Rows are 32 bytes, so
// lanes that read different rows of one 256-byte bank row at once conflict; nothing here pads against it.
// Global memory is written with plain vector stores only; no global atomics of any kind; every output element is written.
#include "pack_layout.h"

namespace {

using u64 = unsigned long long;

constexpr int RT = 256;                          // threads per molecule
constexpr int RW = RT / 64;                      // waves
constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = DL_RINGS_MAX_ATOMS;
constexpr int WORDS = MAX_KEPT / 64;             // 64-bit words per row of the matrix
constexpr int BINS = DL_RING_BINS;
constexpr int MARK = 1 << 16;                    // s_map: kept index | MARK
constexpr int NO_RING = 0x7fffffff;
constexpr int BONDS_OVERFLOW = 1;                // DL_BONDS_OVERFLOW of dl_bonds_args.status
static_assert(MAX_KEPT == RT && WORDS == 4, "one thread per kept atom, four words per row");

// exclusive prefix sum of one int per thread over the workgroup; returns the total through `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds /* [RW] */, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < RW; ++k) {
        if (k < w) base += lds[k];
        sum += lds[k];
    }
    __syncthreads();
    total = sum;
    return base + incl - v;
}

__device__ __forceinline__ int block_sum(int v, int* lds) {
    int total = 0;
    block_exclusive_scan(v, lds, total);
    return total;
}

// entry e of the list: a bond of this molecule (0 <= i, j < n, i != j, order 1..3)?
__device__ __forceinline__ bool load_bond(const int* list, int e, int n, int& i, int& j) {
    i = list[e * 3];
    j = list[e * 3 + 1];
    const int order = list[e * 3 + 2];
    return i >= 0 && j >= 0 && i < n && j < n && i != j && order >= 1 && order <= 3;
}

__device__ __forceinline__ u64 bit_in_word(int atom, int w) { return (atom >> 6) == w ? 1ull << (atom & 63) : 0ull; }

// atoms of the smallest cycle through the bond (u, v) of the matrix, 0 when the bond is a bridge
__device__ __forceinline__ int smallest_ring(const u64* adj, int u, int v) {
    u64 frontier[WORDS], visited[WORDS], target[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        target[w] = bit_in_word(v, w);
        frontier[w] = adj[u * WORDS + w] & ~target[w];          // level 1 without the bond itself
        visited[w] = frontier[w] | bit_in_word(u, w);
    }
    for (int level = 1; level < MAX_KEPT; ++level) {             // frontier = the atoms `level` bonds from u
        u64 next[WORDS] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            u64 f = frontier[w];
            while (f) {
                const u64* row = adj + (w * 64 + __builtin_ctzll(f)) * WORDS;
                f &= f - 1;
#pragma unroll
                for (int q = 0; q < WORDS; ++q) next[q] |= row[q];
            }
        }
        u64 hit = 0, any = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            next[w] &= ~visited[w];
            hit |= next[w] & target[w];
            any |= next[w];
            visited[w] |= next[w];
            frontier[w] = next[w];
        }
        if (hit) return level + 2;                               // v is level + 1 bonds from u: that path and the bond
        if (!any) return 0;
    }
    return 0;                                                    // not reached: every level adds an atom or ends the search
}

__device__ __forceinline__ int ring_bin(int ring) { return ring == 0 ? 0 : (ring <= 7 ? ring - 2 : BINS - 1); }

__global__ __launch_bounds__(RT) void ring_scores_kernel(dl_rings_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];
    __shared__ int s_map[MAX_ROWS];
    __shared__ int s_label[MAX_KEPT];
    __shared__ int s_min[MAX_KEPT];
    __shared__ int s_hist[2 * BINS];
    __shared__ int s_scan[RW];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, capacity = a.capacity;

    // ---- stage: rank the real rows, and the kept rows among themselves (thread t owns the rows [t * per, t * per + per))
    const int per = (N + RT - 1) / RT;
    const int r0 = min(tid * per, N), r1 = min(r0 + per, N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    int mine = 0, mine_kept = 0;
    for (int r = r0; r < r1; ++r) {
        if (mask[r] == 0.0f) continue;
        ++mine;
        mine_kept += !(drop && drop[r] != 0.0f);
    }
    int n = 0, n_kept = 0;
    int k = block_exclusive_scan(mine, s_scan, n);
    int kk = block_exclusive_scan(mine_kept, s_scan, n_kept);

    const int given = a.n_bonds_in[b];
    const int nb = min(max(given, 0), capacity);
    const int status_in = a.status_in[b] | (given > capacity ? BONDS_OVERFLOW : 0);
    int* bond_ring = a.bond_ring + size_t(b) * capacity;
    int* atom_ring = a.atom_ring + size_t(b) * N;
    int* hist = a.ring_hist + size_t(b) * 2 * BINS;

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrix does not hold this molecule
        for (int e = tid; e < capacity; e += RT) bond_ring[e] = 0;
        for (int i = tid; i < N; i += RT) atom_ring[i] = 0;
        if (tid < 2 * BINS) hist[tid] = 0;
        if (tid == 0) {
            a.n_atoms[b] = n_kept;
            a.n_bonds[b] = 0;
            a.n_components[b] = 0;
            a.n_rings[b] = 0;
            a.status[b] = status_in | DL_RINGS_TOO_LARGE;
        }
        return;
    }

    for (int r = r0; r < r1; ++r) {
        if (mask[r] == 0.0f) continue;
        const bool kept = !(drop && drop[r] != 0.0f);
        s_map[k++] = kept ? (kk | ((mark && mark[r] != 0.0f) ? MARK : 0)) : -1;
        kk += kept;
    }
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = 0;
    s_label[tid] = tid;
    s_min[tid] = NO_RING;
    if (tid < 2 * BINS) s_hist[tid] = 0;
    __syncthreads();

    // ---- build: the bit matrix over the kept atoms
    const int* list = a.bonds + size_t(b) * capacity * 3;       // never read when nb == 0
    int bad = 0, mine_bonds = 0;
    for (int e = tid; e < nb; e += RT) {
        int i, j;
        if (!load_bond(list, e, n, i, j)) { bad = 1; continue; }
        const int mi = s_map[i], mj = s_map[j];
        if ((mi | mj) < 0) continue;                             // an end is dropped: no bond of this graph, and no error
        const int u = mi & 0xFFFF, v = mj & 0xFFFF;
        const int lo = min(u, v), hi = max(u, v);
        const u64 bit = 1ull << (hi & 63);
        const u64 old = atomicOr(&s_adj[lo * WORDS + (hi >> 6)], bit);
        atomicOr(&s_adj[hi * WORDS + (lo >> 6)], 1ull << (lo & 63));
        if (old & bit) bad = 1;                                  // the pair a second time
        else ++mine_bonds;
    }
    bad = __syncthreads_or(bad);
    const int n_bonds = block_sum(mine_bonds, s_scan);

    // ---- label: pieces of the graph
    const bool atom = tid < n_kept;
    for (;;) {
        int changed = 0, best = tid;
        if (atom) {
            best = s_label[tid];
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = s_adj[tid * WORDS + w];
                while (f) {
                    best = min(best, s_label[w * 64 + __builtin_ctzll(f)]);
                    f &= f - 1;
                }
            }
        }
        __syncthreads();
        if (atom && best < s_label[tid]) { s_label[tid] = best; changed = 1; }
        __syncthreads();
        const int jump = s_label[s_label[tid]];                  // labels of threads beyond n_kept stay their own index
        __syncthreads();
        if (jump != s_label[tid]) { s_label[tid] = jump; changed = 1; }
        if (!__syncthreads_or(changed)) break;
    }
    const int n_comp = block_sum(atom && s_label[tid] == tid, s_scan);

    // ---- search: the smallest ring through every bond of the list
    for (int e = tid; e < capacity; e += RT) {
        int ring = 0, i, j;
        if (e < nb && load_bond(list, e, n, i, j)) {
            const int mi = s_map[i], mj = s_map[j];
            if ((mi | mj) >= 0) {
                const int u = mi & 0xFFFF, v = mj & 0xFFFF;
                ring = smallest_ring(s_adj, u, v);
                const int bin = ring_bin(ring);
                atomicAdd(&s_hist[bin], 1);
                if ((mi | mj) & MARK) atomicAdd(&s_hist[BINS + bin], 1);
                if (ring) {
                    atomicMin(&s_min[u], ring);
                    atomicMin(&s_min[v], ring);
                }
            }
        }
        bond_ring[e] = ring;
    }
    __syncthreads();

    for (int i = tid; i < N; i += RT) {
        int ring = 0;
        if (i < n && s_map[i] >= 0) {
            const int least = s_min[s_map[i] & 0xFFFF];
            ring = least == NO_RING ? 0 : least;
        }
        atom_ring[i] = ring;
    }
    if (tid < 2 * BINS) hist[tid] = s_hist[tid];
    if (tid == 0) {
        a.n_atoms[b] = n_kept;
        a.n_bonds[b] = n_bonds;
        a.n_components[b] = n_comp;
        a.n_rings[b] = n_bonds - n_kept + n_comp;
        a.status[b] = status_in | (bad ? DL_RINGS_BAD_BOND : 0);
    }
}

}  // namespace

extern "C" {

int32_t dl_ring_scores(const dl_rings_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->capacity < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->node_mask || !a->n_bonds_in || !a->status_in || !a->n_atoms || !a->n_bonds || !a->n_components || !a->n_rings ||
        !a->atom_ring || !a->ring_hist || !a->status || (a->capacity > 0 && (!a->bonds || !a->bond_ring)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(ring_scores_kernel, dim3(a->B), dim3(RT), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
