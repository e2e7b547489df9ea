// rings.hip — ring perception of the bond graphs bonds.hip left on the device: for every bond the size of the smallest ring
// through it, for every atom the smallest ring it lies in, the number of pieces and the cyclomatic number.  What the
// reference asks of RDKit's ring perception (compute_metrics.py:128-145, CalcNumRings of the linker) asked of the graph.
//
// One 256-thread workgroup per molecule, one launch per batch, reading what dl_perceive_bonds wrote for the same batch, with
// the conventions of mol_graph.h: atom k is the k-th row with node_mask != 0; drop_mask removes atoms after that numbering
// together with every bond that touches them; an entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and
// 1 <= order <= 3, in either orientation; anything else is skipped and sets DL_RINGS_BAD_BOND.  mark_mask marks atoms (the
// callers pass the linker): the second histogram row counts the bonds with a marked end.
//
// At most DL_RINGS_MAX_ATOMS = 256 KEPT atoms (N itself may be 1024: pocket rows are dropped, not counted).  The graph over
// the kept atoms is a 256 x 256 bit matrix in LDS, four 64-bit words per row.
//
//   stage   real rows ranked in row order (number_rows of mol_graph.h), kept rows ranked among themselves; s_map[atom] is the
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
#include "mol_graph.h"

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_RINGS_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;              // 64-bit words per row of the matrix
constexpr int BINS = DL_RING_BINS;
constexpr int MARK = 1 << 16;                    // s_map: kept index | MARK
constexpr int NO_RING = 0x7fffffff;

__device__ __forceinline__ int ring_bin(int ring) { return ring == 0 ? 0 : (ring <= 7 ? ring - 2 : BINS - 1); }

__global__ __launch_bounds__(WG) void ring_scores_kernel(dl_rings_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];
    __shared__ int s_map[MAX_ROWS];
    __shared__ int s_label[MAX_KEPT];
    __shared__ int s_min[MAX_KEPT];
    __shared__ int s_hist[2 * BINS];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, capacity = a.capacity;

    // ---- stage: rank the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;

    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb, status_in = in.status;
    int* bond_ring = a.bond_ring + size_t(b) * capacity;
    int* atom_ring = a.atom_ring + size_t(b) * N;
    int* hist = a.ring_hist + size_t(b) * 2 * BINS;

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrix does not hold this molecule
        for (int e = tid; e < capacity; e += WG) bond_ring[e] = 0;
        for (int i = tid; i < N; i += WG) atom_ring[i] = 0;
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

    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? (kk | ((mark && mark[r] != 0.0f) ? MARK : 0)) : -1;
    });
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = 0;
    s_label[tid] = tid;
    s_min[tid] = NO_RING;
    if (tid < 2 * BINS) s_hist[tid] = 0;
    __syncthreads();

    // ---- build: the bit matrix over the kept atoms
    const int* list = a.bonds + size_t(b) * capacity * 3;       // never read when nb == 0
    int bad = 0, mine_bonds = 0;
    for (int e = tid; e < nb; e += WG) {
        int i, j, order;
        if (!load_bond<3>(list, e, n, i, j, order)) { bad = 1; continue; }
        const int mi = s_map[i], mj = s_map[j];
        if ((mi | mj) < 0) continue;                             // an end is dropped: no bond of this graph, and no error
        if (add_pair(s_adj, mi & 0xFFFF, mj & 0xFFFF)) ++mine_bonds;
        else bad = 1;                                            // the pair a second time
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
    for (int e = tid; e < capacity; e += WG) {
        int ring = 0, i, j, order;
        if (e < nb && load_bond<3>(list, e, n, i, j, order)) {
            const int mi = s_map[i], mj = s_map[j];
            if ((mi | mj) >= 0) {
                const int u = mi & 0xFFFF, v = mj & 0xFFFF;
                u64 visited[WORDS];
                const int d = search(s_adj, u, v, v, visited);   // v is d bonds from u without the bond itself
                ring = d < 0 ? 0 : d + 1;                        // that path and the bond; a bridge: 0
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

    for (int i = tid; i < N; i += WG) {
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
    hipLaunchKernelGGL(ring_scores_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
