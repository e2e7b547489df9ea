// stereo.hip — stereo perception from 3D: which kept atoms are tetrahedral centres, which double bonds are stereo double bonds,
// and which configuration the coordinates show, on the bond graphs bonds.hip and aromatic.hip left on the device.  The rule is
// this project's own; it is stated in full in include/difflinker_hip.h and restated in tests/stereo_ref.py, and it is NOT
// RDKit's stereo perception and NOT CIP: labels 1 and 2 are relative to the colour classes of canon.hip's root refinement.
//
// dl_stereo_perceive: one 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h.
//
//   stage    rows ranked by number_rows; type, planar flag, mark and coordinates of the kept atoms go to LDS by kept index
//   entries  every kept list entry, repeated ones too, packed into LDS (end | end << 8 | order << 16) through an LDS cursor:
//            the classes sum over them as canon.hip's rounds do, and a sum does not ask for their order
//   build    three 256 x 256 bit matrices over the kept atoms: the pairs (build_pairs of mol_graph.h), those of order 2 and 3
//            by the first entry of a pair (for_each_first_entry)
//   classes  n rounds of the colour refinement, one thread per entry adding into its two ends' sums with LDS atomics (integer
//            sums modulo 2^64), one thread per atom mixing; then thread i counts the strictly smaller colours.  canon.hip's
//            refine_and_rank is fused with its individualisation and with the reduction that picks the next cell, and walks
//            a CSR adjacency this kernel has no other use for, so the rounds are written here a second time; the tests hold
//            the two to the same classes
//   centres  thread a owns kept atom a: its rows say whether it is a centre, its (at most four) neighbours are sorted by
//            class, and the sign of one determinant of unit vectors is its label
//   bonds    the thread that owns the first entry of a pair of order 2 searches the ring (search of mol_graph.h with the
//            bond masked, as rings.hip does), finds the two reference neighbours and compares one cosine; it writes the
//            entry's label itself, after the same thread cleared the entry
//   counts   four counts, all and marked packed in one 64-bit word each, go through block_sum
//
// Every fp64 value is computed by one thread from LDS in a fixed order (ends by kept index, neighbours by class); nothing but
// integers is ever summed.  LDS: 3 x 8 KiB matrices + 8 KiB entries + 4 KiB map + 3 KiB coordinates + 6 KiB colours and sums +
// per-atom arrays: about 48 KiB, static.  Global memory is written with plain vector stores only; no workspace.
#include "mol_graph.h"
#include "points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_STEREO_MAX_ATOMS
constexpr int MAX_ENTRIES = DL_STEREO_MAX_BONDS;
constexpr int WORDS = MATRIX_WORDS;
static_assert(DL_STEREO_MAX_ATOMS == MATRIX_ATOMS, "the matrix holds a molecule, a kept index fits a byte");
static_assert(DL_STEREO_TOO_LARGE == DL_POSE_TOO_LARGE && DL_STEREO_BAD_BOND == DL_POSE_BAD_BOND &&
                  DL_STEREO_NONFINITE == DL_POSE_NONFINITE && DL_STEREO_TOO_LARGE == DL_CANON_TOO_LARGE &&
                  DL_STEREO_BAD_BOND == DL_CANON_BAD_BOND,
              "the status bits are those of dl_pose_checks and dl_canonical_ranks");
static_assert(DL_STEREO_MAX_BONDS == DL_CANON_MAX_BONDS && DL_STEREO_COUNTS == 4, "canon's limit; four counts per row");

enum : int { CENTRES, CENTRES_UNDETERMINED, DOUBLE_BONDS, DOUBLE_BONDS_UNDETERMINED };
enum : int { NO_STEREO = 0, UNDETERMINED = 3 };
constexpr int NONE = 0x7fffffff;

// one item in the low half, one more in the high half when it is marked: all and marked counts travel in one word
__device__ __forceinline__ long long item(bool marked) { return 1ll + (static_cast<long long>(marked) << 32); }

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// (ka, a) and (kb, b) in ascending order of the keys
__device__ __forceinline__ void sort2(int& ka, int& a, int& kb, int& b) {
    if (kb < ka) {
        const int k = ka, t = a;
        ka = kb; a = b;
        kb = k; b = t;
    }
}

// v / |v|; false when v has zero length
__device__ __forceinline__ bool unit(V3 v, V3& out) {
    const double l2 = dot(v, v);
    if (l2 == 0.0) return false;
    const double l = sqrt(l2);
    out = {v.x / l, v.y / l, v.z / l};
    return true;
}

// the other neighbours of end `u` of the double bond (u, v): false unless there are one or two, all through pairs of order 1,
// of different classes when there are two.  `ref` is the one with the highest class
__device__ __forceinline__ bool reference_neighbour(const u64* adj, const u64* o2, const u64* o3, const int* cls, int u, int v, int& ref) {
    const int others = count_row(adj, u) - 1;
    if (others < 1 || others > 2 || count_row(o2, u) != 1 || count_row(o3, u) != 0) return false;
    int nbr[2];
    first_members(adj, u, v, nbr, 2);
    ref = nbr[0];
    if (others == 2) {
        if (cls[nbr[0]] == cls[nbr[1]]) return false;
        if (cls[nbr[1]] > cls[nbr[0]]) ref = nbr[1];
    }
    return true;
}

__global__ __launch_bounds__(WG) void stereo_kernel(dl_stereo_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_o2[MAX_KEPT * WORDS];          // of order 2
    __shared__ __align__(16) u64 s_o3[MAX_KEPT * WORDS];          // of order 3
    __shared__ u64 s_col0[MAX_KEPT], s_col1[MAX_KEPT], s_acc[MAX_KEPT];
    __shared__ unsigned s_entry[MAX_ENTRIES];                     // end | end << 8 | order << 16
    __shared__ int s_map[MAX_ROWS];                               // atom number -> kept index, or -1
    __shared__ float s_x[MAX_KEPT * 3];
    __shared__ int s_class[MAX_KEPT], s_label[MAX_KEPT];
    __shared__ unsigned char s_type[MAX_KEPT], s_planar[MAX_KEPT], s_mark[MAX_KEPT];
    __shared__ int s_scan[WG_WAVES];
    __shared__ long long s_sum[WG_WAVES];
    __shared__ int s_cursor;

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
    int* counts = a.counts + size_t(b) * 2 * DL_STEREO_COUNTS;
    int* atom_class = a.atom_class + size_t(b) * N;
    int* atom_stereo = a.atom_stereo + size_t(b) * N;
    int* bond_stereo = capacity ? a.bond_stereo + size_t(b) * capacity : nullptr;

    // the neutral outputs of a molecule the LDS does not hold; called by the whole workgroup or by none of it
    auto neutral = [&](int status) {
        for (int k = tid; k < N; k += WG) atom_class[k] = atom_stereo[k] = -1;
        for (int e = tid; e < capacity; e += WG) bond_stereo[e] = 0;
        if (tid < 2 * DL_STEREO_COUNTS) counts[tid] = 0;
        if (tid == 0) a.status[b] = status;
    };
    if (n_kept > MAX_KEPT) {
        neutral(in.status | DL_STEREO_TOO_LARGE);
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
    s_acc[tid] = 0;
    s_label[tid] = NO_STEREO;
    if (tid == 0) s_cursor = 0;
    bad_x = __syncthreads_or(bad_x);             // a molecule with a non-finite coordinate gets its classes and no label

    // ---- entries: every kept list entry, for the classes
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    int no_bond = 0;
    for (int e = tid; e < nb; e += WG) {
        Bond bd;
        if (!load_bond(list, e, n, bd, no_bond)) continue;
        const int u = s_map[bd.i], v = s_map[bd.j];
        if ((u | v) < 0) continue;                               // an end is dropped: no bond of this graph, and no error
        const int slot = atomicAdd(&s_cursor, 1);
        if (slot < MAX_ENTRIES) s_entry[slot] = unsigned(u) | unsigned(v) << 8 | unsigned(bd.order) << 16;
    }
    no_bond = __syncthreads_or(no_bond);         // its barrier completes s_entry and s_cursor
    const int n_entries = s_cursor;
    if (n_entries > MAX_ENTRIES) {               // uniform: repeated pairs are not looked for, as in canon.hip
        neutral(in.status | DL_STEREO_TOO_LARGE | (no_bond ? DL_STEREO_BAD_BOND : 0));
        return;
    }

    // ---- build: the pairs, then the orders the first entry of every pair gives them
    const PairBuild pairs = build_pairs(list, nb, n, s_map, s_adj);
    for_each_first_entry(list, nb, n, s_map, pairs.repeated, [&](int, const Bond& bd, int u, int v) {
        if (bd.order == 2) set_pair(s_o2, u, v);
        if (bd.order == 3) set_pair(s_o3, u, v);
    });

    // ---- classes: the root refinement of canon.hip, n rounds, then the tied ranks
    const bool atom = tid < n_kept;
    if (atom) s_col0[tid] = mix2(SEED_COLOUR, u64(s_type[tid] + 1));
    __syncthreads();                             // the matrices are complete as well
    u64* cur = s_col0;
    u64* nxt = s_col1;
    for (int r = 0; r < n_kept; ++r) {
        for (int e = tid; e < n_entries; e += WG) {
            const unsigned w = s_entry[e];
            const int u = w & 0xFF, v = (w >> 8) & 0xFF;
            const u64 order = w >> 16;
            atomicAdd(&s_acc[u], mix2(cur[v], order));
            atomicAdd(&s_acc[v], mix2(cur[u], order));
        }
        __syncthreads();
        if (atom) {
            nxt[tid] = mix2(cur[tid], s_acc[tid]);
            s_acc[tid] = 0;                      // its owner clears it for the next round
        }
        __syncthreads();
        u64* t = cur; cur = nxt; nxt = t;
    }
    if (atom) {
        const u64 c = cur[tid];
        int less = 0;
        for (int j = 0; j < n_kept; ++j) less += cur[j] < c;
        s_class[tid] = less;
    }
    __syncthreads();

    long long cnt[DL_STEREO_COUNTS] = {0, 0, 0, 0};

    // ---- centres: thread c owns kept atom c
    if (atom && !bad_x) {
        const int c = tid;
        const int d = count_row(s_adj, c), n2 = count_row(s_o2, c), n3 = count_row(s_o3, c);
        const int h = max(0, a.default_valence[s_type[c]] - (d + n2 + 2 * n3));
        if (!s_planar[c] && n2 == 0 && n3 == 0 && ((d == 4 && h == 0) || (d == 3 && h == 1))) {
            int nbr[4] = {0, 0, 0, 0}, key[4];
            first_members(s_adj, c, -1, nbr, 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) key[q] = q < d ? s_class[nbr[q]] : NONE;      // d == 3: the fourth slot stays last
            sort2(key[0], nbr[0], key[1], nbr[1]);                                   // by ascending class: a network of five
            sort2(key[2], nbr[2], key[3], nbr[3]);                                   // exchanges, so that nothing is indexed
            sort2(key[0], nbr[0], key[2], nbr[2]);                                   // by a variable and the arrays stay in
            sort2(key[1], nbr[1], key[3], nbr[3]);                                   // registers
            sort2(key[1], nbr[1], key[2], nbr[2]);
            bool distinct = true, marked = s_mark[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= d) continue;
                if (q && key[q] == key[q - 1]) distinct = false;
                marked |= s_mark[nbr[q]] != 0;
            }
            if (distinct) {
                const V3 xc = point(s_x, c);
                V3 u[4];
                bool ok = true;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < d) ok &= unit(sub(point(s_x, nbr[q]), xc), u[q]);
                }
                int label = UNDETERMINED;
                if (ok) {
                    double V, T;
                    if (d == 4) {
                        V = dot(sub(u[1], u[0]), cross(sub(u[2], u[0]), sub(u[3], u[0])));
                        T = a.flat * a.v_ideal4;
                    } else {
                        V = dot(u[0], cross(u[1], u[2]));
                        T = a.flat * a.v_ideal3;
                    }
                    if (V > T) label = 1;
                    if (V < -T) label = 2;
                }
                s_label[c] = label;
                cnt[label == UNDETERMINED ? CENTRES_UNDETERMINED : CENTRES] += item(marked);
            }
        }
    }

    // ---- bonds: every entry is cleared, and the first entry of a stereo double bond's pair is labelled by the same thread
    for (int e = tid; e < capacity; e += WG) bond_stereo[e] = 0;
    if (!bad_x) {
        const int* aromatic = a.bond_aromatic ? a.bond_aromatic + size_t(b) * capacity : nullptr;
        for_each_first_entry(list, nb, n, s_map, pairs.repeated, [&](int e, const Bond& bd, int u, int v) {
            if (bd.order != 2 || (aromatic && aromatic[e] != 0)) return;
            const int lo = min(u, v), hi = max(u, v);            // kept atoms keep the order of their numbers
            int ra, rb;
            if (!reference_neighbour(s_adj, s_o2, s_o3, s_class, lo, hi, ra) ||
                !reference_neighbour(s_adj, s_o2, s_o3, s_class, hi, lo, rb))
                return;
            u64 visited[WORDS];
            const int path = search(s_adj, lo, hi, hi, visited);  // bonds of the shortest way round, or -1
            if (path >= 0 && path + 1 < 8) return;                // in a ring of fewer than 8 atoms
            int label = UNDETERMINED;
            const V3 xa = point(s_x, lo), xb = point(s_x, hi);
            V3 ax;
            if (unit(sub(xb, xa), ax)) {
                const V3 wa = sub(point(s_x, ra), xa), wb = sub(point(s_x, rb), xb);
                const double sa = dot(wa, ax), sb = dot(wb, ax);
                const V3 p = sub(wa, V3{sa * ax.x, sa * ax.y, sa * ax.z}), q = sub(wb, V3{sb * ax.x, sb * ax.y, sb * ax.z});
                const double lp = sqrt(dot(p, p)), lq = sqrt(dot(q, q));
                if (!(lp < 0.1) && !(lq < 0.1)) {
                    const double c = dot(p, q) / (lp * lq);
                    if (c > a.twist) label = 1;
                    if (c < -a.twist) label = 2;
                }
            }
            bond_stereo[e] = label;
            cnt[label == UNDETERMINED ? DOUBLE_BONDS_UNDETERMINED : DOUBLE_BONDS] +=
                item(s_mark[lo] | s_mark[hi] | s_mark[ra] | s_mark[rb]);
        });
    }

    // ---- counts, classes and labels
#pragma unroll
    for (int c = 0; c < DL_STEREO_COUNTS; ++c) {  // the barriers of the first sum order s_label before its reads below
        const long long total = block_sum(cnt[c], s_sum);
        if (tid == 0) {
            counts[c] = int(total & 0xffffffffll);
            counts[DL_STEREO_COUNTS + c] = int(total >> 32);
        }
    }
    for (int k = tid; k < N; k += WG) {
        const int kk = k < n ? s_map[k] : -1;
        atom_class[k] = kk >= 0 ? s_class[kk] : -1;
        atom_stereo[k] = kk >= 0 ? s_label[kk] : -1;
    }
    if (tid == 0) a.status[b] = in.status | (pairs.bad ? DL_STEREO_BAD_BOND : 0) | (bad_x ? DL_STEREO_NONFINITE : 0);
}

}  // namespace

extern "C" {

int32_t dl_stereo_perceive(const dl_stereo_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->nf > 256 || a->capacity < 0 || !(a->flat >= 0.0) ||
        !(a->twist >= 0.0) || !(a->v_ideal4 > 0.0) || !(a->v_ideal3 > 0.0))
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->default_valence || !a->n_bonds_in || !a->atom_class || !a->atom_stereo ||
        !a->counts || !a->status || (a->capacity > 0 && (!a->bonds || !a->bond_stereo)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(stereo_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
