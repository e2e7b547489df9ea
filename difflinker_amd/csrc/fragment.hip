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
//
// dl_fragment_multicuts (below the double cuts) shares everything up to `search` as front_half() and then looks for STARS:
// sets of 3 to 5 cuttable bonds with one piece, the linker, touching all of them (the reference's multi-fragment sets).
// Cuttable bonds are bridges, so the other cuttable bonds lie whole on one side of bond c or the other: INSIDE(c) is the
// 64-bit mask of those inside SIDE(c), and a set S is a star iff for every c in S the rest of S is all inside or all outside
// INSIDE(c) - outside: fragment c is SIDE(c), inside: its complement.  No graph search per set, k AND/compare steps.
//
//   tables  C(v, j) for v <= 64, j <= 5; INSIDE(c) and |SIDE(c)| per cuttable bond
//   stars   per k = 3, 4, 5: the C(m, k) sets in lexicographic order are split into 256 contiguous runs of ranks, one per
//           thread.  A thread unranks the first set of its run with the binomial table and goes on a PREFIX (the first
//           k - 1 bonds) at a time: the prefix alone says which last bonds it allows, as one 64-bit mask, and only those are
//           looked at.  One walk counts the kept stars, ONE block prefix scan per k numbers them, and a second walk - only
//           by threads whose first number is below R, only until R - writes the 22-integer records
//   labels  a thread per record reads it back (written by this workgroup, behind a barrier), finds its bonds again by
//           binary search of their entries among the cuttable bonds and packs them into 64 bits; a wave per row then writes
//           the rows of its 64 records, the lanes over the atoms, the packed words passed by shuffle
//
// LDS of the multi-cut kernel: the 20 KiB above without the chunk staging + 0.75 KiB INSIDE and sizes + 1.5 KiB binomials.
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

// What the list says of one molecule, after the front half
struct Front {
    int n;                                       // atoms
    int n_bonds;                                 // distinct pairs
    int n_cuttable;                              // cuttable bonds: bond c < MAX_ATOMS has s_cut_* [c] and s_side[c]
    int status;                                  // status_in, BONDS_OVERFLOW, DL_FRAG_TOO_LARGE, DL_FRAG_BAD_BOND, DL_FRAG_DISCONNECTED
    bool whole;                                  // one piece (or no atoms)
};

struct Lds {
    u64* adj;                                    // [MAX_ATOMS * WORDS] the bit matrix
    u64* side;                                   // [MAX_ATOMS * WORDS] SIDE(c) of cuttable bond c
    int *cut_e, *cut_i, *cut_j;                  // [MAX_ATOMS] entry and atoms of cuttable bond c
    int* atom;                                   // [MAX_ATOMS]
    int* scan;                                   // [FW]
};

// The front half both kernels share: stage, build, marks, one piece?, search.  `a` is either argument struct (the input
// fields have the same names); `bond_side` is this molecule's row, or null when the caller has no such output.  Returns
// false, with n and status set, when the molecule has more than MAX_ATOMS atoms: nothing else was looked at then.
template <class Args>
__device__ __forceinline__ bool front_half(const Args& a, int b, const Lds& s, int* bond_side, Front& f) {
    const int tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity;

    // ---- stage: rank the real rows (thread t owns the rows [t * per, t * per + per))
    const int per = (N + FT - 1) / FT;
    const int r0 = min(tid * per, N), r1 = min(r0 + per, N);
    const float* mask = a.node_mask + size_t(b) * N;
    int mine = 0;
    for (int r = r0; r < r1; ++r) mine += mask[r] != 0.0f;
    int n = 0;
    int k = block_exclusive_scan(mine, s.scan, n);

    const int given = a.n_bonds_in[b];
    const int nb = min(max(given, 0), capacity);
    const int status_in = (a.status_in ? a.status_in[b] : 0) | (given > capacity ? BONDS_OVERFLOW : 0);
    f.n = n;
    f.n_bonds = f.n_cuttable = 0;
    f.whole = false;
    f.status = status_in | DL_FRAG_TOO_LARGE;
    if (n > MAX_ATOMS) return false;             // uniform over the workgroup: the matrix does not hold this molecule

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
        s.atom[k++] = carbon ? (IS_CARBON | ((charge ? charge[r] : 0) == 0 ? NEUTRAL_CARBON : 0)) : 0;
    }
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s.adj[tid * WORDS + w] = 0;
    __syncthreads();

    // ---- build: the bit matrix
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    int bad = 0, repeated = 0, mine_bonds = 0;
    for (int e = tid; e < nb; e += FT) {
        int i, j, order;
        if (!load_bond(list, e, n, i, j, order)) { bad = 1; continue; }
        const int lo = min(i, j), hi = max(i, j);
        const u64 bit = 1ull << (hi & 63);
        const u64 old = atomicOr(&s.adj[lo * WORDS + (hi >> 6)], bit);
        atomicOr(&s.adj[hi * WORDS + (lo >> 6)], 1ull << (lo & 63));
        if (old & bit) repeated = 1;                             // exactly one entry of each distinct pair sees it unset
        else ++mine_bonds;
    }
    bad = __syncthreads_or(bad);
    repeated = __syncthreads_or(repeated);
    int n_bonds = 0;
    block_exclusive_scan(mine_bonds, s.scan, n_bonds);

    // ---- marks: atoms with a double or triple bond to an atom that is no carbon
    for (int e = tid; e < nb; e += FT) {
        int i, j, order;
        if (!load_bond(list, e, n, i, j, order) || (order != 2 && order != 3)) continue;
        if (repeated && seen_before(list, e, n, i, j)) continue;
        if (!(s.atom[j] & IS_CARBON)) atomicOr(&s.atom[i], HETERO_MULTIPLE);
        if (!(s.atom[i] & IS_CARBON)) atomicOr(&s.atom[j], HETERO_MULTIPLE);
    }
    __syncthreads();

    // ---- one piece?  Every thread runs the same search from atom 0 (the LDS reads broadcast)
    bool whole = true;
    if (n > 0) {
        u64 visited[WORDS];
        search(s.adj, 0, -1, -1, visited);
        whole = popcount(visited) == n;
    }

    // ---- search: the cuttable bonds, numbered in list order
    int n_cuttable = 0;
    for (int e0 = 0; e0 < nb; e0 += FT) {                        // uniform trip count: the scan below has barriers
        const int e = e0 + tid;
        int side = 0, i = 0, j = 0, order;
        u64 visited[WORDS] = {0, 0, 0, 0};
        if (e < nb && load_bond(list, e, n, i, j, order) && order == 1) {
            const int ai = s.atom[i], aj = s.atom[j];
            const bool qualifies = (ai & (NEUTRAL_CARBON | HETERO_MULTIPLE)) == NEUTRAL_CARBON ||
                                   (aj & (NEUTRAL_CARBON | HETERO_MULTIPLE)) == NEUTRAL_CARBON;
            if (qualifies && !(repeated && seen_before(list, e, n, i, j)) && search(s.adj, i, j, j, visited) < 0)
                side = popcount(visited);
        }
        int chunk = 0;
        const int c = n_cuttable + block_exclusive_scan(side != 0, s.scan, chunk);
        if (side && c < MAX_ATOMS) {                             // bridges of at most 256 atoms: c <= 254 always
            s.cut_e[c] = e;
            s.cut_i[c] = i;
            s.cut_j[c] = j;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) s.side[c * WORDS + w] = visited[w];
        }
        if (bond_side && e < capacity) bond_side[e] = side;
        n_cuttable += chunk;
    }
    if (bond_side)
        for (int e = (nb + FT - 1) / FT * FT + tid; e < capacity; e += FT) bond_side[e] = 0;
    __syncthreads();

    f.n_bonds = n_bonds;
    f.n_cuttable = min(n_cuttable, MAX_ATOMS);
    f.whole = whole;
    f.status = status_in | (bad || repeated ? DL_FRAG_BAD_BOND : 0) | (whole ? 0 : DL_FRAG_DISCONNECTED);
    return true;
}

__global__ __launch_bounds__(FT) void fragment_cuts_kernel(dl_fragment_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_ATOMS * WORDS];
    __shared__ __align__(16) u64 s_side[MAX_ATOMS * WORDS];      // SIDE(c) of cuttable bond c
    __shared__ int s_cut_e[MAX_ATOMS], s_cut_i[MAX_ATOMS], s_cut_j[MAX_ATOMS];
    __shared__ int s_atom[MAX_ATOMS];
    __shared__ int s_keep[FT];                                   // the kept pairs of a chunk: c1 | c2 << 8 | flip1 << 16 | flip2 << 17
    __shared__ int s_scan[FW];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, capacity = a.capacity, R = a.R;
    int* bond_side = a.bond_side + size_t(b) * capacity;         // never written when capacity == 0
    int* cuts = a.cuts + size_t(b) * R * FIELDS;                 // never written when R == 0
    unsigned char* labels = a.labels + size_t(b) * R * N;

    Front f;
    if (!front_half(a, b, Lds{s_adj, s_side, s_cut_e, s_cut_i, s_cut_j, s_atom, s_scan}, bond_side, f)) {
        for (int e = tid; e < capacity; e += FT) bond_side[e] = 0;
        for (int q = tid; q < R * FIELDS; q += FT) cuts[q] = 0;
        for (size_t q = tid; q < size_t(R) * N; q += FT) labels[q] = 255;
        if (tid == 0) {
            a.n_atoms[b] = f.n;
            a.n_bonds[b] = 0;
            a.n_cuttable[b] = 0;
            a.n_cuts[b] = 0;
            a.status[b] = f.status;
        }
        return;
    }
    const int n = f.n, n_cuttable = f.n_cuttable;
    const bool whole = f.whole;

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
        a.n_bonds[b] = f.n_bonds;
        a.n_cuttable[b] = n_cuttable;
        a.n_cuts[b] = n_cuts;
        a.status[b] = f.status | (n_cuts > R ? DL_FRAG_TRUNCATED : 0);
    }
}

// ---- multi-cuts: stars of 3 to 5 cuttable bonds ----------------------------------------------------------------------------
// C(v, j) for 0 <= v <= MC, 0 <= j <= KMAX sits at s_binom[v * BW + j]; C(64, 5) = 7 624 512 fits an int
constexpr int MC = DL_FRAG_MULTI_MAX_CUTTABLE, KMIN = DL_FRAG_MULTI_MIN_CUTS, KMAX = DL_FRAG_MULTI_MAX_CUTS;
constexpr int MF = DL_FRAG_MULTI_FIELDS, BW = KMAX + 1, LINKER = DL_FRAG_MULTI_LINKER;
static_assert(MC == 64 && KMIN == 3 && KMAX == 5 && MF == 2 + 4 * KMAX, "one 64-bit mask per set; k, n_linker and four rows of five");

struct Stars {
    const u64* inside;                           // [MC] INSIDE(c): the other cuttable bonds inside SIDE(c)
    const int* size;                             // [MC] |SIDE(c)|
    const int* binom;
    const int *cut_e, *cut_i, *cut_j;
    int m, n, min_linker, min_fragment;
};

// the set c[0] < ... < c[K-1] of rank `rank` < C(m, K) in lexicographic order
template <int K>
__device__ __forceinline__ void unrank(const Stars& s, int rank, int (&c)[K]) {
    int v = 0;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        for (;;) {                               // C(m - 1 - v, K - 1 - q) sets go on with v here
            const int with_v = s.binom[(s.m - 1 - v) * BW + (K - 1 - q)];
            if (rank < with_v) break;
            rank -= with_v;
            ++v;
        }
        c[q] = v++;
    }
}

// the next set in lexicographic order; there is one: the caller counts
template <int K>
__device__ __forceinline__ void next(int m, int (&c)[K]) {
    int p = K - 1;
#pragma unroll
    for (int q = K - 1; q > 0; --q)
        if (p == q && c[q] == m - K + q) p = q - 1;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        if (q == p) ++c[q];
        else if (q > p) c[q] = c[q - 1] + 1;                     // q >= 1 here
    }
}

// The sets of ranks [lo, hi) in lexicographic order, a PREFIX c[0..K-2] at a time: the sets that share it differ in their
// last bond d alone, and form a run of ranks.  For a bond q of the prefix the rest of the prefix must lie all inside or all
// outside INSIDE(c_q) - which of the two also says where d has to lie, so the d that the prefix allows are one 64-bit mask,
// the AND of INSIDE(c_q) or its complement over q.  Only those d are looked at: d itself must see the whole prefix on one
// side, and the sizes must pass.  A prefix that is no star by itself, or has a fragment too small, costs nothing more.
// Returns the number of kept stars, at most `stop`; with WRITE their records go to cuts[at], cuts[at + 1], ... below R.
template <int K, bool WRITE>
__device__ __forceinline__ int walk(const Stars& s, int lo, int hi, int stop, int at, int R, int* cuts) {
    int c[K], frag[K], count = 0;
    unrank<K>(s, lo, c);
    for (int r = lo; r < hi && count < stop;) {
        const int run = min(hi - r, s.m - c[K - 1]);             // the last bonds c[K-1] .. c[K-1] + run - 1
        u64 prefix = 0;
#pragma unroll
        for (int q = 0; q < K - 1; ++q) prefix |= 1ull << c[q];
        u64 allowed = ~0ull;
        int sum = 0, flip = 0;
        bool ok = true;
#pragma unroll
        for (int q = 0; q < K - 1; ++q) {
            const u64 inside = s.inside[c[q]];
            const int size = s.size[c[q]];
            const u64 others = prefix ^ (1ull << c[q]);          // K - 2 >= 1 bonds
            const u64 in = others & inside;
            ok = ok && (in == 0 || in == others);
            allowed &= in ? inside : ~inside;
            frag[q] = in ? s.n - size : size;                    // inside: the fragment is the complement of SIDE
            flip |= in ? 1 << q : 0;
            ok = ok && frag[q] >= s.min_fragment;
            sum += frag[q];
        }
        u64 candidates = ok ? allowed & ((run >= 64 ? ~0ull : (1ull << run) - 1) << c[K - 1]) : 0;
        while (candidates && count < stop) {
            const int d = __builtin_ctzll(candidates);
            candidates &= candidates - 1;
            const u64 in = prefix & s.inside[d];
            const int size = s.size[d];
            frag[K - 1] = in ? s.n - size : size;
            const int linker = s.n - sum - frag[K - 1];
            if ((in != 0 && in != prefix) || frag[K - 1] < s.min_fragment || linker < s.min_linker) continue;
            ++count;
            if (!WRITE) continue;
            if (at >= R) return count;
            int* rec = cuts + size_t(at++) * MF;
            rec[0] = K;
            rec[1] = linker;
#pragma unroll
            for (int q = 0; q < KMAX; ++q) {
                const bool used = q < K;
                const int cq = used ? (q == K - 1 ? d : c[used ? q : 0]) : 0;
                const int i = s.cut_i[cq], j = s.cut_j[cq];
                const bool inwards = used && (q == K - 1 ? in != 0 : (flip >> q) & 1);
                rec[2 + q] = used ? s.cut_e[cq] : -1;
                rec[2 + KMAX + q] = used ? (inwards ? j : i) : -1;            // anchor: the fragment's atom
                rec[2 + 2 * KMAX + q] = used ? (inwards ? i : j) : -1;        // exit: the linker's
                rec[2 + 3 * KMAX + q] = used ? frag[used ? q : 0] : -1;
            }
        }
        r += run;
        if (r < hi) {                            // the next prefix: the set after the last one of this prefix
            c[K - 1] = s.m - 1;
            next<K>(s.m, c);
        }
    }
    return count;
}

// The kept stars of K bonds: counted in one walk, numbered from `first` on by a block scan, and the records below R written
// in a second walk by the threads that own them.  Thread t walks the ranks [t * per, t * per + per).  Returns their number.
template <int K>
__device__ __forceinline__ int stars_of(const Stars& s, int first, int R, int* cuts, int* lds_scan) {
    const int total = s.m >= K ? s.binom[s.m * BW + K] : 0;
    const int per = (total + FT - 1) / FT;
    const int lo = min(int(threadIdx.x) * per, total), hi = min(lo + per, total);
    const int mine = lo < hi ? walk<K, false>(s, lo, hi, per, 0, 0, nullptr) : 0;
    int all = 0;
    const int at = first + block_exclusive_scan(mine, lds_scan, all);
    if (mine && at < R) walk<K, true>(s, lo, hi, mine, at, R, cuts);
    return all;
}

__global__ __launch_bounds__(FT) void fragment_multicuts_kernel(dl_fragment_multi_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_ATOMS * WORDS];
    __shared__ __align__(16) u64 s_side[MAX_ATOMS * WORDS];
    __shared__ u64 s_inside[MC];
    __shared__ int s_cut_e[MAX_ATOMS], s_cut_i[MAX_ATOMS], s_cut_j[MAX_ATOMS];
    __shared__ int s_atom[MAX_ATOMS];
    __shared__ int s_size[MC];
    __shared__ int s_binom[(MC + 1) * BW];
    __shared__ int s_scan[FW];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, R = a.R;
    int* cuts = a.cuts + size_t(b) * R * MF;                     // never written when R == 0
    unsigned char* labels = a.labels + size_t(b) * R * N;
    int* n_cuts_k = a.n_cuts_k + size_t(b) * (KMAX - KMIN + 1);

    Front f;
    if (!front_half(a, b, Lds{s_adj, s_side, s_cut_e, s_cut_i, s_cut_j, s_atom, s_scan}, nullptr, f)) {
        for (int q = tid; q < R * MF; q += FT) cuts[q] = 0;
        for (size_t q = tid; q < size_t(R) * N; q += FT) labels[q] = 255;
        if (tid == 0) {
            a.n_atoms[b] = f.n;
            a.n_bonds[b] = 0;
            a.n_cuttable[b] = 0;
            a.n_cuts[b] = 0;
            a.status[b] = f.status;
        }
        if (tid <= KMAX - KMIN) n_cuts_k[tid] = 0;
        return;
    }
    const int n = f.n;
    const bool gates = n <= a.max_atoms && f.n_bonds - n + 1 >= a.min_rings;
    const bool many = gates && f.n_cuttable > MC;
    const int m = f.whole && gates && !many ? f.n_cuttable : 0;  // the bonds to choose from

    // ---- tables: C(v, j), exact at every step: C(v - j + t, t) = C(v - j + t - 1, t - 1) * (v - j + t) / t
    for (int q = tid; q < (MC + 1) * BW; q += FT) {
        const int v = q / BW, j = q % BW;
        u64 c = j <= v;
        for (int t = 1; t <= j && j <= v; ++t) c = c * u64(v - j + t) / u64(t);
        s_binom[q] = int(c);
    }
    // ---- INSIDE(c): both atoms of another cuttable bond lie on one side of c, so its atom i decides
    if (tid < m) {
        u64 inside = 0;
        for (int d = 0; d < m; ++d)
            if (d != tid && has(s_side + tid * WORDS, s_cut_i[d])) inside |= 1ull << d;
        s_inside[tid] = inside;
        int size = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) size += __popcll(s_side[tid * WORDS + w]);
        s_size[tid] = size;
    }
    __syncthreads();

    // ---- stars: k ascending, lexicographic within a k
    const Stars s{s_inside, s_size, s_binom, s_cut_e, s_cut_i, s_cut_j, m, n, a.min_linker, a.min_fragment};
    int n_cuts = 0, of3 = 0, of4 = 0, of5 = 0;
    if (a.min_cuts <= 3 && 3 <= a.max_cuts) n_cuts += of3 = stars_of<3>(s, n_cuts, R, cuts, s_scan);
    if (a.min_cuts <= 4 && 4 <= a.max_cuts) n_cuts += of4 = stars_of<4>(s, n_cuts, R, cuts, s_scan);
    if (a.min_cuts <= 5 && 5 <= a.max_cuts) n_cuts += of5 = stars_of<5>(s, n_cuts, R, cuts, s_scan);
    __syncthreads();                                             // the records are read back below

    // ---- label rows.  Thread t describes record 256 * chunk + t: it reads the record back, finds its bonds again by their
    // entries (s_cut_e ascends) and packs, per fragment q, bond c_q into bits 8q..8q+5 and "the fragment is the complement
    // of SIDE" into bit 8q+6, k into bits 40..42.  Then every wave writes the rows of its 64 records, a row at a time with
    // the lanes over the atoms; the descriptions travel by shuffle, so no row waits for a load from memory
    const int used = min(n_cuts, R);
    const int lane = tid & 63, wave = tid >> 6;
    for (int r0 = 0; r0 < used; r0 += FT) {
        u64 mine = 0;
        if (r0 + tid < used) {
            const int* rec = cuts + size_t(r0 + tid) * MF;
            const int k = rec[0];
            mine = u64(k) << 40;
#pragma unroll
            for (int q = 0; q < KMAX; ++q) {
                if (q >= k) continue;
                const int e = rec[2 + q];
                int c = 0, hi = m - 1;                           // the last c with s_cut_e[c] <= e
                while (c < hi) {
                    const int mid = (c + hi + 1) >> 1;
                    if (s_cut_e[mid] <= e) c = mid;
                    else hi = mid - 1;
                }
                mine |= u64(c | (rec[2 + KMAX + q] != s_cut_i[c] ? 64 : 0)) << (8 * q);   // the anchor is j: the complement
            }
        }
        const int rows = min(used - (r0 + wave * 64), 64);       // uniform over the wave; may be negative
        for (int t = 0; t < rows; ++t) {
            const u64 word = __shfl(mine, t, 64);
            const int k = int(word >> 40);
            unsigned char* row = labels + size_t(r0 + wave * 64 + t) * N;
            for (int atom = lane; atom < N; atom += 64) {
                unsigned char label = 255;
                if (atom < n) {
                    label = LINKER;
#pragma unroll
                    for (int q = KMAX - 1; q >= 0; --q) {
                        const int c = int(word >> (8 * q)) & 63;
                        const bool flip = (word >> (8 * q + 6)) & 1;
                        if (q < k && has(s_side + c * WORDS, atom) != flip) label = q;
                    }
                }
                row[atom] = label;
            }
        }
    }

    // ---- the records nobody used
    for (int q = used * MF + tid; q < R * MF; q += FT) cuts[q] = 0;
    for (size_t q = size_t(used) * N + tid; q < size_t(R) * N; q += FT) labels[q] = 255;
    if (tid == 0) {
        a.n_atoms[b] = n;
        a.n_bonds[b] = f.n_bonds;
        a.n_cuttable[b] = f.n_cuttable;
        a.n_cuts[b] = n_cuts;
        a.status[b] = f.status | (many ? DL_FRAG_MANY_CUTTABLE : 0) | (n_cuts > R ? DL_FRAG_TRUNCATED : 0);
        n_cuts_k[0] = of3;
        n_cuts_k[1] = of4;
        n_cuts_k[2] = of5;
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

int32_t dl_fragment_multicuts(const dl_fragment_multi_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->carbon_type < 0 || a->carbon_type >= a->nf ||
        a->capacity < 0 || a->R < 0 || a->min_cuts < KMIN || a->max_cuts > KMAX || a->min_cuts > a->max_cuts)
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->node_mask || !a->n_bonds_in || !a->n_atoms || !a->n_bonds || !a->n_cuttable || !a->n_cuts ||
        !a->status || !a->n_cuts_k || (a->capacity > 0 && !a->bonds) || (a->R > 0 && (!a->cuts || !a->labels)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(fragment_multicuts_kernel, dim3(a->B), dim3(FT), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
