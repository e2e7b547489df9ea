// mol_graph.h — what the kernels that read a perceived bond list with 256 threads per molecule share (mol_keys.hip,
// fingerprint.hip, rings.hip, aromatic.hip, pharmacophore.hip, hydrogens.hip, pose_checks.hip, relax.hip, canon.hip, stereo.hip), on top of workgroup.h: the
// 64-bit mixing function of the colour refinement, the test that says whether a list entry is a bond, the list's length and
// overflow bit, the numbering of the real and of the kept rows, the 256 x 256 bit matrix in LDS with its breadth-first search,
// and the two-pass build of the matrices by bond order that the last three share (rings.hip and aromatic.hip build through
// tagged maps, in their own text; pose_checks.hip has the second pass in its own text: profiles/graph_build/README.md).  Integers only: those three's coordinates are in points.h.  Small functions that each kernel
// calls in its own order; what a kernel counts and flags around them is its own and is specified in include/difflinker_hip.h.
// fragment.hip is to use them too and still carries its own copies of the scan, load_bond, seen_before, bit_in_word, has and
// search: with the shared ones its star enumeration measured 3 to 7 % slower although its text is the same, so it waits
// until that is understood (profiles/mol_graph/README.md).
#pragma once
#include "workgroup.h"

namespace {

using u64 = unsigned long long;                  // the 64-bit type the LDS atomics take; uint64_t outputs convert by value

constexpr u64 SEED_COLOUR = 0x243F6A8885A308D3ull, SEED_KEY = 0x13198A2E03707344ull, MIX_B = 0xD6E8FEB86659FD93ull;

__device__ __forceinline__ u64 mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u64 mix2(u64 a, u64 b) { return mix64(a + b * MIX_B); }

// ---- the bond list ------------------------------------------------------------------------------------------------------------
// entry e of the list: a bond of this molecule (0 <= i, j < n, i != j, 1 <= order <= MAX_ORDER)?  MAX_ORDER is 3 wherever the
// list is what dl_perceive_bonds wrote, whose orders are 1..3.  fragment.hip's rule is 4 (its own copy today): it cuts the
// molecules of a data set, read from files in which 4 marks an aromatic bond - a bond of the graph, never cuttable, no bad entry
template <int MAX_ORDER>
__device__ __forceinline__ bool load_bond(const int* list, int e, int n, int& i, int& j, int& order) {
    i = list[e * 3];
    j = list[e * 3 + 1];
    order = list[e * 3 + 2];
    return i >= 0 && j >= 0 && i < n && j < n && i != j && order >= 1 && order <= MAX_ORDER;
}

struct Bond {
    int i, j, order;
};

// the same for a list of dl_perceive_bonds; `bad` collects the entries that are no bond
__device__ __forceinline__ bool load_bond(const int* list, int e, int n, Bond& bd, int& bad) {
    const bool ok = load_bond<3>(list, e, n, bd.i, bd.j, bd.order);
    bad |= !ok;
    return ok;
}

// does an entry before e hold the pair (i, j), in either orientation?  "The first entry of a repeated pair" needs list order,
// which the bit matrix does not keep; this walks the list, so ask only when the build saw a repeated pair somewhere
template <int MAX_ORDER>
__device__ __forceinline__ bool seen_before(const int* list, int e, int n, int i, int j) {
    for (int f = 0; f < e; ++f) {
        int fi, fj, forder;
        if (load_bond<MAX_ORDER>(list, f, n, fi, fj, forder) && ((fi == i && fj == j) || (fi == j && fj == i))) return true;
    }
    return false;
}

// How much of molecule b's list is read: n_bonds_in clamped to [0, capacity] (a negative count is 0).  `status` is the
// incoming status (status_in may be null: none) with DL_BONDS_OVERFLOW when the list was cut short at its capacity
struct BondsIn {
    int nb, status;
};

__device__ __forceinline__ BondsIn bonds_in(const int* n_bonds_in, const int* status_in, int b, int capacity) {
    const int given = n_bonds_in[b];
    return {min(max(given, 0), capacity), (status_in ? status_in[b] : 0) | (given > capacity ? DL_BONDS_OVERFLOW : 0)};
}

// ---- atoms ----------------------------------------------------------------------------------------------------------------------
// Atom k is the k-th row with node_mask != 0 (as bonds.hip numbers them); drop_mask (may be null) removes atoms after that
// numbering, and the kept atoms are numbered among themselves.  number_rows counts this thread's rows and scans the counts:
// n and n_kept are the molecule's, k and kk the numbers of this thread's first real and first kept row.  for_each_real_row
// then calls f(r, k, kept, kk) for every real row r of the thread, where each kernel stages its own payload
struct RowNumbers {
    int n, n_kept, k, kk;
};

__device__ __forceinline__ RowNumbers number_rows(const Rows& rows, const float* mask, const float* drop, int* lds /* [WG_WAVES] */) {
    int mine = 0, mine_kept = 0;
    for (int r = rows.r0; r < rows.r1; ++r) {
        if (mask[r] == 0.0f) continue;
        ++mine;
        mine_kept += !(drop && drop[r] != 0.0f);
    }
    RowNumbers s;
    s.k = block_exclusive_scan(mine, lds, s.n);
    s.kk = block_exclusive_scan(mine_kept, lds, s.n_kept);
    return s;
}

template <class F>
__device__ __forceinline__ void for_each_real_row(const Rows& rows, const float* mask, const float* drop, const RowNumbers& s, F&& f) {
    int k = s.k, kk = s.kk;
    for (int r = rows.r0; r < rows.r1; ++r) {
        if (mask[r] == 0.0f) continue;
        const bool kept = !(drop && drop[r] != 0.0f);
        f(r, k, kept, kk);
        ++k;
        kk += kept;
    }
}

// ---- the bit matrix -------------------------------------------------------------------------------------------------------------
// A graph of at most MATRIX_ATOMS atoms as MATRIX_ATOMS rows of MATRIX_WORDS 64-bit words in LDS: bit v of row u is the pair
// (u, v).  One thread per atom clears or reads a row, hence MATRIX_ATOMS == WG
constexpr int MATRIX_ATOMS = 256, MATRIX_WORDS = MATRIX_ATOMS / 64;
static_assert(MATRIX_ATOMS == WG && MATRIX_WORDS == 4, "one thread per atom, four words per row");
static_assert(DL_RINGS_MAX_ATOMS == MATRIX_ATOMS && DL_AROM_MAX_ATOMS == MATRIX_ATOMS && DL_FRAG_MAX_ATOMS == MATRIX_ATOMS,
              "the limits the header promises are the matrix's");

__device__ __forceinline__ u64 bit_in_word(int atom, int w) { return (atom >> 6) == w ? 1ull << (atom & 63) : 0ull; }

// is `atom` in the set (one row of a matrix, or any MATRIX_WORDS words)?
__device__ __forceinline__ bool has(const u64* set, int atom) { return (set[atom >> 6] >> (atom & 63)) & 1ull; }

__device__ __forceinline__ bool bit(const u64* m, int u, int v) { return has(m + u * MATRIX_WORDS, v); }

__device__ __forceinline__ void set_pair(u64* m, int u, int v) {
    atomicOr(&m[u * MATRIX_WORDS + (v >> 6)], 1ull << (v & 63));
    atomicOr(&m[v * MATRIX_WORDS + (u >> 6)], 1ull << (u & 63));
}

// set_pair for the build from a list: returns whether the pair was not there yet.  atomicOr returns the old value, so exactly
// one entry of each distinct pair sees it unset, whatever the order the atomics land in and whichever orientation an entry has
// (the bit that decides is always the one in the smaller atom's row)
__device__ __forceinline__ bool add_pair(u64* adj, int u, int v) {
    const int lo = min(u, v), hi = max(u, v);
    const u64 one = 1ull << (hi & 63);
    const u64 old = atomicOr(&adj[lo * MATRIX_WORDS + (hi >> 6)], one);
    atomicOr(&adj[hi * MATRIX_WORDS + (lo >> 6)], 1ull << (lo & 63));
    return !(old & one);
}

// ---- the ordered build ------------------------------------------------------------------------------------------------------------
// The matrices of a list of dl_perceive_bonds whose ends go through a plain map from atom number to kept index, or -1 for a
// dropped atom: "the first entry of a repeated pair gives the pair its order" (include/difflinker_hip.h), written once.
// build_pairs is the first pass: every bond of the kept graph into adj.  Before the call `map` is written and `adj` is cleared,
// and a barrier of the kernel's has run since.  Its two workgroup reductions also complete adj; the result is uniform: `bad`
// (an entry that is no bond, or a repeated pair) and `repeated`
struct PairBuild {
    int bad, repeated;
};

__device__ __forceinline__ PairBuild build_pairs(const int* list, int nb, int n, const int* map, u64* adj) {
    int bad = 0, repeated = 0;
    for (int e = threadIdx.x; e < nb; e += WG) {
        Bond bd;
        if (!load_bond(list, e, n, bd, bad)) continue;
        const int u = map[bd.i], v = map[bd.j];
        if ((u | v) < 0) continue;                               // an end is dropped: no bond of this graph, and no error
        if (!add_pair(adj, u, v)) repeated = 1;
    }
    repeated = __syncthreads_or(repeated);
    bad = __syncthreads_or(bad) | repeated;
    return {bad, repeated};
}

// the second pass: f(e, bond, u, v) for every entry e that is a bond of the kept graph (kept ends u, v) and the first entry of
// its pair.  What f writes is ordered by the kernel's own barrier after the pass
template <class F>
__device__ __forceinline__ void for_each_first_entry(const int* list, int nb, int n, const int* map, int repeated, F&& f) {
    for (int e = threadIdx.x; e < nb; e += WG) {
        Bond bd;
        int ignored = 0;
        if (!load_bond(list, e, n, bd, ignored)) continue;
        const int u = map[bd.i], v = map[bd.j];
        if ((u | v) < 0 || (repeated && seen_before<3>(list, e, n, bd.i, bd.j))) continue;
        f(e, bd, u, v);
    }
}

// the first `limit` atoms of row u of m other than `skip`, ascending; returns how many were written
__device__ __forceinline__ int first_members(const u64* m, int u, int skip, int* out, int limit) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < MATRIX_WORDS; ++w) {
        u64 f = m[u * MATRIX_WORDS + w] & ~bit_in_word(skip, w);
        while (f && c < limit) {
            out[c++] = w * 64 + __builtin_ctzll(f);
            f &= f - 1;
        }
    }
    return c;
}

__device__ __forceinline__ int count_row(const u64* m, int u) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < MATRIX_WORDS; ++w) c += __popcll(m[u * MATRIX_WORDS + w]);
    return c;
}

// Breadth-first search from u over the matrix, level-synchronous, frontier and visited set in registers.  `masked` (or -1)
// is taken out of u's row at level 0 only: the bond (u, masked) can be walked nowhere else, because u is visited from the
// start.  Ends when a level contains `target` (returns its distance in bonds from u) or is empty (returns -1: visited[] is
// then everything that can be reached).  target must not be u: u is in no frontier, so the search would never meet it
// (rings.hip passes the two ends of a bond, which differ).  Reads the matrix only: no other lane matters
__device__ __forceinline__ int search(const u64* adj, int u, int masked, int target, u64 (&visited)[MATRIX_WORDS]) {
    u64 frontier[MATRIX_WORDS], goal[MATRIX_WORDS];
#pragma unroll
    for (int w = 0; w < MATRIX_WORDS; ++w) {
        goal[w] = bit_in_word(target, w);
        frontier[w] = adj[u * MATRIX_WORDS + w] & ~bit_in_word(masked, w);
        visited[w] = frontier[w] | bit_in_word(u, w);
    }
    for (int level = 1; level <= MATRIX_ATOMS; ++level) {        // frontier = the atoms `level` bonds from u
        u64 hit = 0, any = 0;
#pragma unroll
        for (int w = 0; w < MATRIX_WORDS; ++w) {
            hit |= frontier[w] & goal[w];
            any |= frontier[w];
        }
        if (hit) return level;
        if (!any) return -1;
        u64 next[MATRIX_WORDS] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < MATRIX_WORDS; ++w) {
            u64 f = frontier[w];
            while (f) {
                const u64* row = adj + (w * 64 + __builtin_ctzll(f)) * MATRIX_WORDS;
                f &= f - 1;
#pragma unroll
                for (int q = 0; q < MATRIX_WORDS; ++q) next[q] |= row[q];
            }
        }
#pragma unroll
        for (int w = 0; w < MATRIX_WORDS; ++w) {
            frontier[w] = next[w] & ~visited[w];
            visited[w] |= frontier[w];
        }
    }
    return -1;                                                   // not reached: every level adds an atom or ends the search
}

}  // namespace
