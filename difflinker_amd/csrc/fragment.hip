// fragment.hip — matched-pair double cuts of molecules: every pair of cuttable bonds splits a molecule into two fragments
// and the linker between them, the examples a linker-design data set is made of.  What the reference asks of RDKit's
// FragmentMol with minCuts = maxCuts = 2 and DeLinker's pattern [#6+0;!$(*=,#[!#6])]!@!=!#[*], asked of the bond graph.
//
// One 256-thread workgroup per molecule, one launch per batch, with the conventions of rings.hip: atom k is the k-th row
// with node_mask != 0, its type the first largest entry of its one_hot row; an entry (i, j, order) is a bond when
// 0 <= i, j < atoms, i != j and 1 <= order <= 4 (4: aromatic), in either orientation; anything else is skipped and sets
// DL_FRAG_BAD_BOND.  Of a repeated pair the FIRST entry is the bond (its order counts); the others set DL_FRAG_BAD_BOND.
//
// A bond is CUTTABLE when its order is 1, it lies in no ring, and at least one end is a carbon of charge 0 without an
// order-2 or order-3 bond to a non-carbon atom.  Cuttable bonds are bridges of a graph of at most 256 atoms, so there are
// at most 255 of them: bond c keeps its entry, its two atoms and SIDE(c), the 256-bit set of the atoms on the side of its
// atom i, in LDS.  For the pair (c1 < c2): when i2 lies in SIDE(c1) the linker is on i1's side, so exit_1 = i1,
// anchor_1 = j1 and fragment 1 is the complement of SIDE(c1); otherwise exit_1 = j1, anchor_1 = i1 and fragment 1 is
// SIDE(c1).  The same with the roles swapped gives fragment 2; the linker is the rest.
//
//   stage   real rows ranked in row order; per atom: carbon?, carbon of charge 0?
//   build   one thread per list entry: LDS atomicOr into the 256 x 256 bit matrix.  Only when some entry met its pair
//           already set (rare; uniform over the workgroup) an entry later asks the list whether an earlier entry holds its
//           pair - which entry is the first must not depend on the order the atomics landed in
//   marks   a first entry of order 2 or 3 marks each end whose partner is no carbon ("multiple bond to a hetero atom")
//   search  chunks of 256 entries: a candidate (first entry, order 1, a qualifying end) runs a register-resident
//           breadth-first search from i with the bond masked; reaching j makes it a ring bond, otherwise the visited set
//           is SIDE.  Cuttable bonds are numbered in list order by a block prefix scan per chunk
//   pairs   chunks of 256 pairs in lexicographic order: sizes from |SIDE|, the size filter, then - only for pairs that
//           pass it - a breadth-first search from exit_1 to exit_2 for path_atoms (both cut bonds are bridges, so the
//           shortest path of the whole graph stays inside the linker).  Kept pairs are numbered by a block prefix scan per
//           chunk, their records written by their threads and their label rows by the whole workgroup
//
// LDS: 8 KiB matrix + 8 KiB sides + 3 KiB cuttable bonds + 1 KiB atoms + 1 KiB chunk staging: 21 KiB, static.
// Global memory is written with plain vector stores only; no global atomics of any kind; every output element is written.
#include "pack_layout.h"

namespace {

using u64 = unsigned long long;

constexpr int FT = 256;                          // threads per molecule
constexpr int FW = FT / 64;                      // waves
constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_ATOMS = DL_FRAG_MAX_ATOMS;
constexpr int WORDS = MAX_ATOMS / 64;            // 64-bit words per row of the matrix
constexpr int FIELDS = DL_FRAG_CUT_FIELDS;
constexpr int BONDS_OVERFLOW = 1;                // DL_BONDS_OVERFLOW of dl_bonds_args.status
constexpr int IS_CARBON = 1, NEUTRAL_CARBON = 2, HETERO_MULTIPLE = 4;     // s_atom bits
static_assert(MAX_ATOMS == FT && WORDS == 4 && FIELDS == 10, "one thread per atom, four words per row, ten ints per record");

// exclusive prefix sum of one int per thread over the workgroup; returns the total through `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds /* [FW] */, int& total) {
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
    for (int k = 0; k < FW; ++k) {
        if (k < w) base += lds[k];
        sum += lds[k];
    }
    __syncthreads();
    total = sum;
    return base + incl - v;
}

// entry e of the list: a bond of this molecule (0 <= i, j < n, i != j, order 1..4)?
__device__ __forceinline__ bool load_bond(const int* list, int e, int n, int& i, int& j, int& order) {
    i = list[e * 3];
    j = list[e * 3 + 1];
    order = list[e * 3 + 2];
    return i >= 0 && j >= 0 && i < n && j < n && i != j && order >= 1 && order <= 4;
}

// does an entry before e hold the pair (i, j)?  Only asked when the molecule has a repeated pair somewhere
__device__ __forceinline__ bool seen_before(const int* list, int e, int n, int i, int j) {
    for (int f = 0; f < e; ++f) {
        int fi, fj, forder;
        if (load_bond(list, f, n, fi, fj, forder) && ((fi == i && fj == j) || (fi == j && fj == i))) return true;
    }
    return false;
}

__device__ __forceinline__ u64 bit_in_word(int atom, int w) { return (atom >> 6) == w ? 1ull << (atom & 63) : 0ull; }

// Breadth-first search from u over the matrix, level-synchronous, frontier and visited set in registers.  `masked` (or -1)
// is taken out of u's row at level 0 only: the bond (u, masked) can be walked nowhere else, because u is visited from the
// start.  Ends when a level contains `target` (returns its distance in bonds from u) or is empty (returns -1: visited[] is
// then everything that can be reached).  target == u returns 0.
__device__ __forceinline__ int search(const u64* adj, int u, int masked, int target, u64 (&visited)[WORDS]) {
    u64 frontier[WORDS], goal[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        goal[w] = bit_in_word(target, w);
        frontier[w] = adj[u * WORDS + w] & ~bit_in_word(masked, w);
        visited[w] = frontier[w] | bit_in_word(u, w);
    }
    if (u == target) return 0;
    for (int level = 1; level <= MAX_ATOMS; ++level) {           // frontier = the atoms `level` bonds from u
        u64 hit = 0, any = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            hit |= frontier[w] & goal[w];
            any |= frontier[w];
        }
        if (hit) return level;
        if (!any) return -1;
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
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            frontier[w] = next[w] & ~visited[w];
            visited[w] |= frontier[w];
        }
    }
    return -1;                                                   // not reached: every level adds an atom or ends the search
}

__device__ __forceinline__ int popcount(const u64 (&s)[WORDS]) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) c += __popcll(s[w]);
    return c;
}

__device__ __forceinline__ bool has(const u64* set, int atom) { return (set[atom >> 6] >> (atom & 63)) & 1ull; }

__global__ __launch_bounds__(FT) void fragment_cuts_kernel(dl_fragment_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_ATOMS * WORDS];
    __shared__ __align__(16) u64 s_side[MAX_ATOMS * WORDS];      // SIDE(c) of cuttable bond c
    __shared__ int s_cut_e[MAX_ATOMS], s_cut_i[MAX_ATOMS], s_cut_j[MAX_ATOMS];
    __shared__ int s_atom[MAX_ATOMS];
    __shared__ int s_keep[FT];                                   // the kept pairs of a chunk: c1 | c2 << 8 | flip1 << 16 | flip2 << 17
    __shared__ int s_scan[FW];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity, R = a.R;

    // ---- stage: rank the real rows (thread t owns the rows [t * per, t * per + per))
    const int per = (N + FT - 1) / FT;
    const int r0 = min(tid * per, N), r1 = min(r0 + per, N);
    const float* mask = a.node_mask + size_t(b) * N;
    int mine = 0;
    for (int r = r0; r < r1; ++r) mine += mask[r] != 0.0f;
    int n = 0;
    int k = block_exclusive_scan(mine, s_scan, n);

    const int given = a.n_bonds_in[b];
    const int nb = min(max(given, 0), capacity);
    const int status_in = (a.status_in ? a.status_in[b] : 0) | (given > capacity ? BONDS_OVERFLOW : 0);
    int* bond_side = a.bond_side + size_t(b) * capacity;         // never written when capacity == 0
    int* cuts = a.cuts + size_t(b) * R * FIELDS;                 // never written when R == 0
    unsigned char* labels = a.labels + size_t(b) * R * N;

    if (n > MAX_ATOMS) {                         // uniform over the workgroup: the matrix does not hold this molecule
        for (int e = tid; e < capacity; e += FT) bond_side[e] = 0;
        for (int q = tid; q < R * FIELDS; q += FT) cuts[q] = 0;
        for (size_t q = tid; q < size_t(R) * N; q += FT) labels[q] = 255;
        if (tid == 0) {
            a.n_atoms[b] = n;
            a.n_bonds[b] = 0;
            a.n_cuttable[b] = 0;
            a.n_cuts[b] = 0;
            a.status[b] = status_in | DL_FRAG_TOO_LARGE;
        }
        return;
    }

    const float* one_hot = a.one_hot + size_t(b) * N * nf;
    const int* charge = a.charge ? a.charge + size_t(b) * N : nullptr;
    for (int r = r0; r < r1; ++r) {
        if (mask[r] == 0.0f) continue;
        int type = 0;
        float best = one_hot[size_t(r) * nf];
        for (int t = 1; t < nf; ++t) {
            const float v = one_hot[size_t(r) * nf + t];
            if (v > best) { best = v; type = t; }
        }
        const bool carbon = type == a.carbon_type;
        s_atom[k++] = carbon ? (IS_CARBON | ((charge ? charge[r] : 0) == 0 ? NEUTRAL_CARBON : 0)) : 0;
    }
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = 0;
    __syncthreads();

    // ---- build: the bit matrix
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    int bad = 0, repeated = 0, mine_bonds = 0;
    for (int e = tid; e < nb; e += FT) {
        int i, j, order;
        if (!load_bond(list, e, n, i, j, order)) { bad = 1; continue; }
        const int lo = min(i, j), hi = max(i, j);
        const u64 bit = 1ull << (hi & 63);
        const u64 old = atomicOr(&s_adj[lo * WORDS + (hi >> 6)], bit);
        atomicOr(&s_adj[hi * WORDS + (lo >> 6)], 1ull << (lo & 63));
        if (old & bit) repeated = 1;                             // exactly one entry of each distinct pair sees it unset
        else ++mine_bonds;
    }
    bad = __syncthreads_or(bad);
    repeated = __syncthreads_or(repeated);
    int n_bonds = 0;
    block_exclusive_scan(mine_bonds, s_scan, n_bonds);

    // ---- marks: atoms with a double or triple bond to an atom that is no carbon
    for (int e = tid; e < nb; e += FT) {
        int i, j, order;
        if (!load_bond(list, e, n, i, j, order) || (order != 2 && order != 3)) continue;
        if (repeated && seen_before(list, e, n, i, j)) continue;
        if (!(s_atom[j] & IS_CARBON)) atomicOr(&s_atom[i], HETERO_MULTIPLE);
        if (!(s_atom[i] & IS_CARBON)) atomicOr(&s_atom[j], HETERO_MULTIPLE);
    }
    __syncthreads();

    // ---- one piece?  Every thread runs the same search from atom 0 (the LDS reads broadcast)
    bool whole = true;
    if (n > 0) {
        u64 visited[WORDS];
        search(s_adj, 0, -1, -1, visited);
        whole = popcount(visited) == n;
    }

    // ---- search: the cuttable bonds, numbered in list order
    int n_cuttable = 0;
    for (int e0 = 0; e0 < nb; e0 += FT) {                        // uniform trip count: the scan below has barriers
        const int e = e0 + tid;
        int side = 0, i = 0, j = 0, order;
        u64 visited[WORDS] = {0, 0, 0, 0};
        if (e < nb && load_bond(list, e, n, i, j, order) && order == 1) {
            const int ai = s_atom[i], aj = s_atom[j];
            const bool qualifies = (ai & (NEUTRAL_CARBON | HETERO_MULTIPLE)) == NEUTRAL_CARBON ||
                                   (aj & (NEUTRAL_CARBON | HETERO_MULTIPLE)) == NEUTRAL_CARBON;
            if (qualifies && !(repeated && seen_before(list, e, n, i, j)) && search(s_adj, i, j, j, visited) < 0)
                side = popcount(visited);
        }
        int chunk = 0;
        const int c = n_cuttable + block_exclusive_scan(side != 0, s_scan, chunk);
        if (side && c < MAX_ATOMS) {                             // bridges of at most 256 atoms: c <= 254 always
            s_cut_e[c] = e;
            s_cut_i[c] = i;
            s_cut_j[c] = j;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) s_side[c * WORDS + w] = visited[w];
        }
        if (e < capacity) bond_side[e] = side;
        n_cuttable += chunk;
    }
    for (int e = (nb + FT - 1) / FT * FT + tid; e < capacity; e += FT) bond_side[e] = 0;
    n_cuttable = min(n_cuttable, MAX_ATOMS);
    __syncthreads();

    // ---- pairs: thread t takes pair number t of every chunk of 256, in lexicographic order of (c1, c2)
    const int n_pairs = whole ? n_cuttable * (n_cuttable - 1) / 2 : 0;
    int n_cuts = 0;
    int c1 = 0, off = tid, len = n_cuttable - 1;                 // the pair (c1, c1 + 1 + off); the row of c1 has `len` pairs
    for (int p0 = 0; p0 < n_pairs; p0 += FT) {
        while (len > 0 && off >= len) { off -= len; ++c1; --len; }
        int keep = 0, staged = 0, rec[FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (len > 0) {
            const int c2 = c1 + 1 + off;
            const int i1 = s_cut_i[c1], j1 = s_cut_j[c1], i2 = s_cut_i[c2], j2 = s_cut_j[c2];
            const bool flip1 = has(s_side + c1 * WORDS, i2);     // the linker is on i1's side
            const bool flip2 = has(s_side + c2 * WORDS, i1);
            int side1 = 0, side2 = 0;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                side1 += __popcll(s_side[c1 * WORDS + w]);
                side2 += __popcll(s_side[c2 * WORDS + w]);
            }
            const int f1 = flip1 ? n - side1 : side1, f2 = flip2 ? n - side2 : side2;
            const int linker = n - f1 - f2;
            const int exit1 = flip1 ? i1 : j1, exit2 = flip2 ? i2 : j2;
            if (linker >= a.min_linker && f1 >= a.min_fragment && f2 >= a.min_fragment &&
                (!a.linker_leq_frags || linker <= min(f1, f2))) {
                u64 visited[WORDS];
                const int path = search(s_adj, exit1, -1, exit2, visited) + 1;
                if (path >= a.min_path_atoms) {
                    keep = 1;
                    staged = c1 | (c2 << 8) | (int(flip1) << 16) | (int(flip2) << 17);
                    rec[0] = s_cut_e[c1];
                    rec[1] = s_cut_e[c2];
                    rec[2] = flip1 ? j1 : i1;
                    rec[3] = exit1;
                    rec[4] = flip2 ? j2 : i2;
                    rec[5] = exit2;
                    rec[6] = f1;
                    rec[7] = f2;
                    rec[8] = linker;
                    rec[9] = path;
                }
            }
        }
        int chunk = 0;
        const int r = n_cuts + block_exclusive_scan(keep, s_scan, chunk);
        if (keep && r < R) {
#pragma unroll
            for (int q = 0; q < FIELDS; ++q) cuts[size_t(r) * FIELDS + q] = rec[q];
            s_keep[r - n_cuts] = staged;                         // what the label rows below are made from
        }
        __syncthreads();
        const int rows = max(min(n_cuts + chunk, R) - n_cuts, 0);
        for (int q = 0; q < rows; ++q) {                         // label rows, one at a time, the workgroup side by side
            const int word = s_keep[q];
            const u64* sa = s_side + (word & 255) * WORDS;
            const u64* sb = s_side + ((word >> 8) & 255) * WORDS;
            const bool fa = (word >> 16) & 1, fb = (word >> 17) & 1;
            unsigned char* row = labels + (size_t(n_cuts) + q) * N;
            for (int atom = tid; atom < N; atom += FT) {
                unsigned char label = 255;
                if (atom < n) label = has(sa, atom) != fa ? 0 : (has(sb, atom) != fb ? 1 : 2);
                row[atom] = label;
            }
        }
        __syncthreads();                                         // s_keep is staged again in the next chunk
        n_cuts += chunk;
        off += FT;
    }

    // ---- the records nobody used
    const int used = min(n_cuts, R);
    for (int q = used * FIELDS + tid; q < R * FIELDS; q += FT) cuts[q] = 0;
    for (size_t q = size_t(used) * N + tid; q < size_t(R) * N; q += FT) labels[q] = 255;
    if (tid == 0) {
        a.n_atoms[b] = n;
        a.n_bonds[b] = n_bonds;
        a.n_cuttable[b] = n_cuttable;
        a.n_cuts[b] = n_cuts;
        a.status[b] = status_in | (bad || repeated ? DL_FRAG_BAD_BOND : 0) | (whole ? 0 : DL_FRAG_DISCONNECTED) |
                      (n_cuts > R ? DL_FRAG_TRUNCATED : 0);
    }
}

}  // namespace

extern "C" {

int32_t dl_fragment_cuts(const dl_fragment_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->carbon_type < 0 || a->carbon_type >= a->nf ||
        a->capacity < 0 || a->R < 0)
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->node_mask || !a->n_bonds_in || !a->n_atoms || !a->n_bonds || !a->n_cuttable || !a->n_cuts ||
        !a->status || (a->capacity > 0 && (!a->bonds || !a->bond_side)) || (a->R > 0 && (!a->cuts || !a->labels)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(fragment_cuts_kernel, dim3(a->B), dim3(FT), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
