// hydrogens.hip — explicit hydrogens with 3D positions for the bond graphs bonds.hip and aromatic.hip left on the device.
// The rule is this project's own; it is stated in full in include/difflinker_hip.h and restated in tests/hydrogens_ref.py,
// and it is NOT RDKit's AddHs and NOT OpenBabel's.
//
// dl_add_hydrogens: one 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h.
//
//   stage    rows ranked by number_rows; type, default valence, planar flag, atom number and coordinates of the kept atoms
//            go to LDS by kept index
//   build    three 256 x 256 bit matrices over the kept atoms: the pairs, the pairs of order 2 and of order 3 (the two
//            passes of mol_graph.h): the first entry of a pair alone gives the pair its order
//   atoms    thread u owns kept atom u: its three rows give d, the valence sum, the class and the count h; a block scan
//            over h gives its hydrogens their places, and the thread computes their directions in fp64, one rounding per
//            operation, from at most three neighbours and one neighbour's neighbour
//   counts   h_count is written by atom number through the map of the stage
//
// LDS: 3 x 8 KiB matrices + 4 KiB map + 3 KiB coordinates + per-atom arrays: about 33 KiB, static.
// Global memory is written with plain vector stores only; no atomics on global memory; no workspace.
#include "mol_graph.h"
#include "points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_HYDRO_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;
static_assert(DL_HYDRO_MAX_ATOMS == MATRIX_ATOMS, "the matrix holds a molecule");
static_assert(DL_HYDRO_TOO_LARGE == DL_PHARM_TOO_LARGE && DL_HYDRO_BAD_BOND == DL_PHARM_BAD_BOND &&
                  DL_HYDRO_OVERFLOW == DL_PHARM_OVERFLOW && DL_HYDRO_NONFINITE == DL_PHARM_NONFINITE,
              "the status bits are those of dl_pharmacophore_features");

constexpr double EPS = 1e-6;
constexpr double SQRT3 = 0x1.bb67ae8584caap+0, SQRT2_3 = 0x1.a20bd700c2c3ep-1, SQRT8_3 = 0x1.e2b7dddfefa67p-1,
                 SQRT3_2 = 0x1.bb67ae8584caap-1;

__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 scale(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 over(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ V3 neg(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a) { return over(a, sqrt(dot(a, a))); }

// e_m - u_m * u for the axis m with the smallest |u_m| (the lowest of equal ones), normalised
__device__ __forceinline__ V3 perp(V3 u) {
    const double ax = fabs(u.x), ay = fabs(u.y), az = fabs(u.z);
    int m = 0;
    double least = ax;
    if (ay < least) { least = ay; m = 1; }
    if (az < least) { m = 2; }
    const double um = m == 0 ? u.x : m == 1 ? u.y : u.z;
    const V3 e = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
    return unit(sub(e, scale(um, u)));
}

enum : int { T2 = 2, T3 = 3, T4 = 4 };           // the class is its number of sites

// the directions of atom u's hydrogens, h of them (h <= sites - d); xs and adj are the LDS copies by kept index
__device__ __forceinline__ void directions(const float* xs, const u64* adj, int u, int cls, int d, int h, V3 (&dir)[4]) {
    const V3 xa = point(xs, u);
    if (d == 0) {                                // T4 alone
        const double g = 1.0 / SQRT3;
        dir[0] = {g, g, g};
        dir[1] = {g, -g, -g};
        dir[2] = {-g, g, -g};
        dir[3] = {-g, -g, g};
        return;
    }
    int nbr[3];
    first_members(adj, u, -1, nbr, 3);           // d >= 1 here and h > 0 means d <= 3
    const V3 u1 = unit(sub(point(xs, nbr[0]), xa));
    if (d == 1) {
        if (cls == T2) {
            dir[0] = neg(u1);
            return;
        }
        const int k = nbr[0];
        int r;
        const bool has_r = first_members(adj, k, u, &r, 1) == 1;
        V3 e1;
        bool from_r = false;
        if (has_r) {
            const V3 w = sub(point(xs, r), point(xs, k));
            const V3 p = sub(w, scale(dot(w, u1), u1));
            const double pp = dot(p, p), ww = dot(w, w);
            if (pp > EPS * ww) {
                e1 = neg(over(p, sqrt(pp)));
                from_r = true;
            }
        }
        if (!from_r) {
            e1 = perp(u1);                       // perp(u1) == perp(-u1): the second atom of a lone pair turns it round,
            if (!has_r && u > k) e1 = neg(e1);   // so that its hydrogens are staggered to the first's (ethane, methanol)
        }
        if (cls == T3) {
            const V3 back = neg(over(u1, 2.0)), side = scale(SQRT3_2, e1);
            dir[0] = add(back, side);
            dir[1] = sub(back, side);
            return;
        }
        const V3 e2 = cross(u1, e1), back = neg(over(u1, 3.0));
        const double cs[3] = {1.0, -0.5, -0.5}, sn[3] = {0.0, SQRT3_2, -SQRT3_2};
#pragma unroll
        for (int q = 0; q < 3; ++q) dir[q] = add(back, scale(SQRT8_3, add(scale(cs[q], e1), scale(sn[q], e2))));
        return;
    }
    const V3 u2 = unit(sub(point(xs, nbr[1]), xa));
    if (d == 2) {
        const V3 s = add(u1, u2), c = cross(u1, u2);
        const double ss = dot(s, s);
        V3 b, n;
        if (ss <= EPS) {
            b = perp(u1);
            n = cross(u1, b);
        } else {
            b = neg(over(s, sqrt(ss)));
            const double cc = dot(c, c);
            n = cc > EPS ? over(c, sqrt(cc)) : perp(u1);
        }
        if (cls == T3) {
            dir[0] = b;
            return;
        }
        const V3 mid = over(b, SQRT3), side = scale(SQRT2_3, n);
        dir[0] = add(mid, side);
        dir[1] = sub(mid, side);
        return;
    }
    const V3 u3 = unit(sub(point(xs, nbr[2]), xa));          // T4, d = 3
    const V3 s = add(add(u1, u2), u3);
    const double ss = dot(s, s);
    if (ss > EPS) {
        dir[0] = neg(over(s, sqrt(ss)));
        return;
    }
    const V3 w = cross(sub(u2, u1), sub(u3, u1));
    const double ww = dot(w, w);
    dir[0] = ww > EPS ? over(w, sqrt(ww)) : perp(u1);
}

__global__ __launch_bounds__(WG) void hydrogens_kernel(dl_hydrogens_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_o2[MAX_KEPT * WORDS];          // of order 2
    __shared__ __align__(16) u64 s_o3[MAX_KEPT * WORDS];          // of order 3
    __shared__ int s_map[MAX_ROWS];                               // atom number -> kept index, or -1
    __shared__ float s_x[MAX_KEPT * 3];
    __shared__ int s_dv[MAX_KEPT];
    __shared__ short s_atom[MAX_KEPT];                            // atom number of a kept atom
    __shared__ unsigned char s_type[MAX_KEPT], s_planar[MAX_KEPT], s_h[MAX_KEPT];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity, Hcap = a.Hcap;

    // ---- stage: rank the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const int* planar = a.atom_planar ? a.atom_planar + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;

    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb;
    int* h_count = a.h_count + size_t(b) * N;

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrices do not hold this molecule
        for (int k = tid; k < N; k += WG) h_count[k] = 0;
        if (tid == 0) {
            a.n_h[b] = 0;
            a.status[b] = in.status | DL_HYDRO_TOO_LARGE;
        }
        return;
    }

    const float* xs = a.x + size_t(b) * N * 3;
    const float* hot = a.one_hot + size_t(b) * N * nf;
    int bad_x = 0;
    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? kk : -1;
        if (!kept) return;
        const int type = first_maximum(hot + size_t(r) * nf, nf);
        s_type[kk] = (unsigned char)type;
        s_dv[kk] = a.default_valence[type];
        s_planar[kk] = planar && planar[k] != 0;
        s_atom[kk] = short(k);
        bad_x |= stage_point(xs, r, s_x, kk);
    });
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = s_o2[tid * WORDS + w] = s_o3[tid * WORDS + w] = 0;
    __syncthreads();

    // ---- build: the pairs first, then what the first entry of every pair says about it
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    const PairBuild pairs = build_pairs(list, nb, n, s_map, s_adj);
    for_each_first_entry(list, nb, n, s_map, pairs.repeated, [&](int, const Bond& bd, int u, int v) {
        if (bd.order == 2) set_pair(s_o2, u, v);
        if (bd.order == 3) set_pair(s_o3, u, v);
    });
    bad_x = __syncthreads_or(bad_x);             // also orders the matrices before their reads

    // ---- atoms: count, class and places; a molecule with a non-finite coordinate gets none
    int h = 0, d = 0, cls = T4;
    if (tid < n_kept && !bad_x) {
        d = count_row(s_adj, tid);
        const int n2 = count_row(s_o2, tid), n3 = count_row(s_o3, tid);
        const int h0 = max(0, s_dv[tid] - (d + n2 + 2 * n3));
        cls = (n3 > 0 || n2 >= 2) ? T2 : (n2 == 1 || (s_planar[tid] && d == 2 && h0 == 1)) ? T3 : T4;
        h = min(h0, max(0, cls - d));
    }
    s_h[tid] = (unsigned char)h;                 // h <= 4
    int n_h;
    const int place = block_exclusive_scan(h, s_scan, n_h);      // its barriers order s_h before the reads below
    for (int k = tid; k < N; k += WG) {
        const int kk = k < n ? s_map[k] : -1;
        h_count[k] = kk >= 0 ? s_h[kk] : 0;
    }
    if (tid == 0) {
        a.n_h[b] = n_h;
        a.status[b] = in.status | (pairs.bad ? DL_HYDRO_BAD_BOND : 0) | (n_h > Hcap ? DL_HYDRO_OVERFLOW : 0) |
                      (bad_x ? DL_HYDRO_NONFINITE : 0);
    }
    if (h == 0 || place >= Hcap) return;         // nothing after this point is shared

    V3 dir[4];
    directions(s_x, s_adj, tid, cls, d, h, dir);
    const V3 xa = point(s_x, tid);
    const double L = a.xh_length[s_type[tid]];
    int* h_parent = a.h_parent + size_t(b) * Hcap;
    double* h_x = a.h_x + size_t(b) * Hcap * 3;
    for (int q = 0; q < h && place + q < Hcap; ++q) {
        const V3 at = add(xa, scale(L, dir[q]));
        h_parent[place + q] = s_atom[tid];
        h_x[(place + q) * 3] = at.x;
        h_x[(place + q) * 3 + 1] = at.y;
        h_x[(place + q) * 3 + 2] = at.z;
    }
}

}  // namespace

extern "C" {

int32_t dl_add_hydrogens(const dl_hydrogens_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->capacity < 0 || a->Hcap < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->default_valence || !a->xh_length || !a->n_bonds_in || !a->n_h ||
        !a->h_count || !a->status || (a->capacity > 0 && !a->bonds) || (a->Hcap > 0 && (!a->h_parent || !a->h_x)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(hydrogens_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
