// pose_checks.hip — is a molecule's own 3D geometry plausible?  Bond lengths, bond angles and internal clashes of the bond graphs
// bonds.hip and aromatic.hip left on the device.  The rule is this project's own, after the idea of PoseBusters' intramolecular
// checks; it is stated in full in include/difflinker_hip.h and restated in tests/pose_checks_ref.py, and it is NOT PoseBusters.
//
// dl_pose_checks: one 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h.
//
//   stage    rows ranked by number_rows; type, planar flag, mark and coordinates of the kept atoms go to LDS by kept index
//   build    three 256 x 256 bit matrices over the kept atoms: the pairs (build_pairs of mol_graph.h), those of order 2 and 3:
//            the first entry of a pair alone gives the pair its order, and its thread compares the pair's length with its
//            bounds (for_each_first_entry's text written out: as a functor 2 % slower, profiles/graph_build/README.md)
//   atoms    thread u owns kept atom u: its rows give d and the class, its (at most six) angles are compared with the class's
//            cosines; three rounds of OR over its neighbours' rows give its ball of radius 3, and of the half of the molecule
//            that follows u cyclically the atoms outside the ball are its far pairs (every pair at exactly one of its atoms)
//   counts   every thread's sixteen counts, all and marked packed in one 64-bit word each, go through block_sum; the flags,
//            set with LDS atomics by kept index, are written by atom number through the map of the stage
//
// Every comparison is an fp64 comparison against a table the host made; nothing but integers is ever summed.
// LDS: 3 x 8 KiB matrices + 4 KiB map + 3 KiB coordinates + 2 KiB clash table + per-atom arrays: about 35 KiB, static.
// Global memory is written with plain vector stores only; no atomics on global memory; no workspace.
#include "mol_graph.h"
#include "points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_POSE_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;
constexpr int CLASH_TYPES = 16, CLASH_IN_LDS = CLASH_TYPES * CLASH_TYPES;        // clash2 is staged in LDS up to 16 types, and read in place beyond
static_assert(DL_POSE_MAX_ATOMS == MATRIX_ATOMS, "the matrix holds a molecule");
static_assert(DL_POSE_TOO_LARGE == DL_HYDRO_TOO_LARGE && DL_POSE_BAD_BOND == DL_HYDRO_BAD_BOND &&
                  DL_POSE_NONFINITE == DL_HYDRO_NONFINITE,
              "the status bits are those of dl_add_hydrogens");
static_assert(DL_POSE_COUNTS == 8, "eight counts per row");

enum : int { BONDS_CHECKED, BONDS_UNTABLED, BONDS_SHORT, BONDS_LONG, ANGLES_CHECKED, ANGLES_BAD, PAIRS_CHECKED, PAIRS_CLASH };
enum : int { LINEAR = 0, TRIGONAL = 1, TETRAHEDRAL = 2 };
enum : int { FLAG_BOND = 1, FLAG_ANGLE = 2, FLAG_CLASH = 4 };

// one item in the low half, one more in the high half when it is marked: all and marked counts travel in one word
__device__ __forceinline__ long long item(bool marked) { return 1ll + (static_cast<long long>(marked) << 32); }

// word w of a set held in registers, w not known at compile time: selects, so that the set stays in registers
__device__ __forceinline__ u64 word_of(const u64 (&set)[MATRIX_WORDS], int w) {
    return w == 0 ? set[0] : w == 1 ? set[1] : w == 2 ? set[2] : set[3];
}

__global__ __launch_bounds__(WG) void pose_kernel(dl_pose_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_o2[MAX_KEPT * WORDS];          // of order 2
    __shared__ __align__(16) u64 s_o3[MAX_KEPT * WORDS];          // of order 3
    __shared__ int s_map[MAX_ROWS];                               // atom number -> kept index, or -1
    __shared__ float s_x[MAX_KEPT * 3];
    __shared__ int s_flags[MAX_KEPT];
    __shared__ unsigned char s_type[MAX_KEPT], s_planar[MAX_KEPT], s_mark[MAX_KEPT];
    __shared__ int s_scan[WG_WAVES];
    __shared__ long long s_sum[WG_WAVES];
    __shared__ double s_clash[CLASH_IN_LDS];                      // clash2, when the vocabulary is small enough

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity;

    // ---- stage: rank the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    const int* planar = a.atom_planar ? a.atom_planar + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;

    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb;
    int* counts = a.counts + size_t(b) * 2 * DL_POSE_COUNTS;
    int* atom_flags = a.atom_flags + size_t(b) * N;

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrices do not hold this molecule
        for (int k = tid; k < N; k += WG) atom_flags[k] = 0;
        if (tid < 2 * DL_POSE_COUNTS) counts[tid] = 0;
        if (tid == 0) a.status[b] = in.status | DL_POSE_TOO_LARGE;
        return;
    }

    const float* xs = a.x + size_t(b) * N * 3;
    const float* hot = a.one_hot + size_t(b) * N * nf;
    int bad_x = 0;
    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? kk : -1;
        if (!kept) return;
        s_type[kk] = (unsigned char)first_maximum(hot + size_t(r) * nf, nf);
        s_planar[kk] = planar && planar[k] != 0;
        s_mark[kk] = mark && mark[r] != 0.0f;
        bad_x |= stage_point(xs, r, s_x, kk);
    });
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = s_o2[tid * WORDS + w] = s_o3[tid * WORDS + w] = 0;
    s_flags[tid] = 0;
    const bool staged = nf <= CLASH_TYPES;
    if (staged && tid < nf * nf) s_clash[tid] = a.clash2[tid];
    const double* clash = staged ? s_clash : a.clash2;
    bad_x = __syncthreads_or(bad_x);             // a molecule with a non-finite coordinate is counted and flagged nowhere

    long long cnt[DL_POSE_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- build: the pairs first, then what the first entry of every pair says about it, and the pair's length
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    const PairBuild pairs = build_pairs(list, nb, n, s_map, s_adj);
    for (int e = tid; e < nb; e += WG) {
        Bond bd;
        int ignored = 0;
        if (!load_bond(list, e, n, bd, ignored)) continue;
        const int u = s_map[bd.i], v = s_map[bd.j];
        if ((u | v) < 0 || (pairs.repeated && seen_before<3>(list, e, n, bd.i, bd.j))) continue;
        if (bd.order == 2) set_pair(s_o2, u, v);
        if (bd.order == 3) set_pair(s_o3, u, v);
        if (bad_x) continue;
        const int lo = min(u, v), hi = max(u, v);                // kept atoms keep the order of their numbers
        const double* bounds = a.length_bounds2 + ((size_t(s_type[lo]) * nf + s_type[hi]) * 3 + (bd.order - 1)) * 2;
        const double lo2 = bounds[0], hi2 = bounds[1];
        const long long one = item(s_mark[u] | s_mark[v]);
        if (lo2 == 0.0 && hi2 == 0.0) {
            cnt[BONDS_UNTABLED] += one;
            continue;
        }
        cnt[BONDS_CHECKED] += one;
        const V3 w = sub(point(s_x, hi), point(s_x, lo));
        const double d2 = dot(w, w);
        const bool is_short = d2 < lo2, is_long = d2 > hi2;
        if (is_short) cnt[BONDS_SHORT] += one;
        if (is_long) cnt[BONDS_LONG] += one;
        if (is_short || is_long) {
            atomicOr(&s_flags[u], FLAG_BOND);
            atomicOr(&s_flags[v], FLAG_BOND);
        }
    }
    __syncthreads();                             // the matrices are complete

    if (tid < n_kept && !bad_x) {
        const int u = tid;
        const V3 xu = point(s_x, u);
        const bool mark_u = s_mark[u];

        // ---- angles at u
        const int d = count_row(s_adj, u);
        if (d >= 2 && d <= 4) {
            const int n2 = count_row(s_o2, u), n3 = count_row(s_o3, u);
            const int cls = (d == 2 && (n3 >= 1 || n2 == 2)) ? LINEAR : ((d <= 3 && n2 >= 1) || s_planar[u]) ? TRIGONAL : TETRAHEDRAL;
            const double c_lo = a.angle_cos[cls * 2], c_hi = a.angle_cos[cls * 2 + 1];
            int nbr[4];
            first_members(s_adj, u, -1, nbr, 4);
            bool any_bad = false;
            for (int q = 1; q < d; ++q) {
                for (int p = 0; p < q; ++p) {
                    const int j = nbr[p], k = nbr[q];
                    if (bit(s_adj, j, k)) continue;              // a three-ring
                    u64 both = 0;
#pragma unroll
                    for (int w = 0; w < WORDS; ++w) both |= s_adj[j * WORDS + w] & s_adj[k * WORDS + w] & ~bit_in_word(u, w);
                    if (both) continue;                          // a four-ring
                    const long long one = item(mark_u | s_mark[j] | s_mark[k]);
                    cnt[ANGLES_CHECKED] += one;
                    const V3 uj = sub(point(s_x, j), xu), uk = sub(point(s_x, k), xu);
                    const double c = dot(uj, uk) / sqrt(dot(uj, uj) * dot(uk, uk));
                    if (c < c_lo || c > c_hi) {
                        cnt[ANGLES_BAD] += one;
                        any_bad = true;
                    }
                }
            }
            if (any_bad) atomicOr(&s_flags[u], FLAG_ANGLE);
        }

        // ---- far pairs of u: the kept atoms above it outside its ball of radius 3
        u64 frontier[WORDS], ball[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            frontier[w] = s_adj[u * WORDS + w];
            ball[w] = frontier[w] | bit_in_word(u, w);
        }
        for (int level = 2; level <= 3; ++level) {
            u64 next[WORDS] = {0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = frontier[w];
                while (f) {
                    const u64* row = s_adj + (w * 64 + __builtin_ctzll(f)) * WORDS;
                    f &= f - 1;
#pragma unroll
                    for (int q = 0; q < WORDS; ++q) next[q] |= row[q];
                }
            }
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                frontier[w] = next[w] & ~ball[w];
                ball[w] |= frontier[w];
            }
        }
        // every unordered pair falls to exactly one of its atoms: u takes the `half` atoms after it, cyclically, and with an even
        // count the lower of two opposite atoms takes that pair, so that every thread walks half a molecule, not thread 0 all
        const int half = (n_kept - 1) / 2 + ((n_kept & 1) == 0 && u < n_kept / 2);
        const int tu = s_type[u];
        bool any_clash = false;
        for (int k = 1; k <= half; ++k) {
            const int v = u + k < n_kept ? u + k : u + k - n_kept;
            if ((word_of(ball, v >> 6) >> (v & 63)) & 1ull) continue;
            const long long one = item(mark_u | s_mark[v]);
            cnt[PAIRS_CHECKED] += one;
            const V3 r = sub(point(s_x, v), xu);
            const int tv = s_type[v];
            const double t2 = clash[u < v ? tu * nf + tv : tv * nf + tu];        // the lower-numbered atom's type first
            if (t2 > 0.0 && dot(r, r) < t2) {
                cnt[PAIRS_CLASH] += one;
                atomicOr(&s_flags[v], FLAG_CLASH);
                any_clash = true;
            }
        }
        if (any_clash) atomicOr(&s_flags[u], FLAG_CLASH);
    }

    // ---- counts and flags
#pragma unroll
    for (int c = 0; c < DL_POSE_COUNTS; ++c) {   // the barriers of the first sum order s_flags before its reads below
        const long long total = block_sum(cnt[c], s_sum);
        if (tid == 0) {
            counts[c] = int(total & 0xffffffffll);
            counts[DL_POSE_COUNTS + c] = int(total >> 32);
        }
    }
    for (int k = tid; k < N; k += WG) {
        const int kk = k < n ? s_map[k] : -1;
        atom_flags[k] = kk >= 0 ? s_flags[kk] : 0;
    }
    if (tid == 0) a.status[b] = in.status | (pairs.bad ? DL_POSE_BAD_BOND : 0) | (bad_x ? DL_POSE_NONFINITE : 0);
}

}  // namespace

extern "C" {

int32_t dl_pose_checks(const dl_pose_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->capacity < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->length_bounds2 || !a->angle_cos || !a->clash2 || !a->n_bonds_in ||
        !a->counts || !a->atom_flags || !a->status || (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
