// interaction.hip — contacts of generated atoms with the protein: the empirical intermolecular terms of Trott & Olson
// (AutoDock Vina, J. Comput. Chem. 31, 455 (2010)) - two steric Gaussians, a repulsion, a hydrophobic and a hydrogen-bond term
// over surface distances - evaluated in place for every molecule of a batch, and the typing of heavy atoms as hydrophobic,
// donor or acceptor that the last two need.  The rule is this project's own after that published functional form and is
// stated in full in include/difflinker_hip.h; tests/interaction_ref.py restates it in numpy.  It is NOT AutoDock Vina's
// numbers: no hydrogens, no PDBQT typing, no search or pose optimisation, no intramolecular term and no rotor normalisation.
//
// dl_interaction_types.  One 256-thread workgroup per molecule, any N.  Rows are taken 256 at a time (thread t owns rows t,
// t + 256, ...); for each such pass every row of the molecule streams through a 256-entry LDS tile (x, y, z, element; group)
// as in clash.hip, and a thread counts the neighbours of its row among the tile's entries of its own group: deg, hetero and
// the first neighbour (whose d2 an oxygen needs) stay in registers.  All lanes read the same tile entry at once: an LDS broadcast.  The
// neighbour test is bonds.hip's (bond_distance_pm of workgroup.h against the single-bond bound, strict).
//
// dl_interaction_scores.  clash.hip's mapping: the query rows are compacted in row order and taken into registers (lane ql of
// Qpad holds query ql, the G = 256 / Qpad lane groups split the targets; above 256 queries four per thread and G = 1), the
// targets pass through the LDS tile, group g walks entries g, g + G, ... - all lanes of a group read one entry, a broadcast.
// A pair inside the cut costs an fp64 square root, two fp64 exp and at most one fp64 division; each term is rounded to a
// signed 64-bit fixed point (llrint(term * 2^32)) and ALL sums are integer sums, in the lane's registers in the pair loop,
// through LDS across the groups, by wave shuffles and one LDS step across the queries: the same bits on every run and
// under every mapping of pairs to lanes.
//
// Global memory is written with plain vector stores only; no atomics of any kind, in LDS or in global memory; every output
// element is written.
#include "workgroup.h"

#pragma clang fp contract(off)

namespace {

constexpr int INTERACT_MAX_QUERY = 1024;         // four queries per thread at most
constexpr int QPT_MAX = INTERACT_MAX_QUERY / WG;
constexpr int MAX_TYPES = 16;
constexpr int TILE = WG;                         // candidates per LDS tile: one per thread
constexpr int TERMS = DL_INTERACT_TERMS;
constexpr int ELEM_MASK = 15;
// the project's atom order (const.GEOM_IDX2ATOM): C O N F S Cl Br I P
constexpr int EL_C = 0, EL_O = 1, EL_N = 2, EL_F = 3, EL_CL = 5, EL_BR = 6, EL_I = 7;

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// clash.hip's squared distance: five fp32 roundings in this order (contraction is off here)
__device__ __forceinline__ float dist2_f32(float dx, float dy, float dz) { return ((dx * dx) + (dy * dy)) + (dz * dz); }

// ---- typing -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int xs_flags(int elem, int deg, int hetero, float first_d2) {
    int flags = 0;
    if (elem == EL_C) flags = hetero ? 0 : DL_XS_HYDROPHOBIC;
    else if (elem == EL_F || elem == EL_CL || elem == EL_BR || elem == EL_I) flags = DL_XS_HYDROPHOBIC;
    else if (elem == EL_N) flags = deg < 3 ? DL_XS_DONOR : 0;
    else if (elem == EL_O) flags = DL_XS_ACCEPTOR | ((deg == 0 || (deg == 1 && first_d2 >= 1.6875f)) ? DL_XS_DONOR : 0);
    return elem | flags;
}

__global__ __launch_bounds__(WG) void interaction_types_kernel(dl_interact_types_args a) {
    __shared__ float4 s_tile[TILE];              // x, y, z, element
    __shared__ int s_group[TILE];                // 0 = no candidate in this slot
    __shared__ float s_table[MAX_TYPES * MAX_TYPES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf;
    const int* grp = a.group + size_t(b) * N;
    const float* xb = a.x + size_t(b) * N * 3;
    const float* hb = a.one_hot + size_t(b) * N * nf;
    int* out = a.xs_type + size_t(b) * N;

    for (int k = tid; k < MAX_TYPES * MAX_TYPES; k += WG) {              // [higher row's element][lower row's], as bonds.hip looks it up
        const int ti = k / MAX_TYPES, tj = k % MAX_TYPES;
        s_table[k] = (ti < nf && tj < nf) ? a.table[ti * nf + tj] : -1.0f;
    }
    int bad = 0;
    for (int r = tid; r < N; r += WG)
        if (grp[r] != 0) bad |= !finite3(xb[3 * r], xb[3 * r + 1], xb[3 * r + 2]);
    if (__syncthreads_or(bad)) {                                         // uniform: the molecule is not typed
        for (int r = tid; r < N; r += WG) out[r] = -1;
        if (tid == 0) a.status[b] = DL_INTERACT_NONFINITE;
        return;
    }

    const int tiles = (N + TILE - 1) / TILE;
    for (int r0 = 0; r0 < N; r0 += WG) {                                 // this pass: row r0 + tid
        const int r = r0 + tid;
        const int mine = r < N ? grp[r] : 0;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        int ti = 0, deg = 0, hetero = 0, first = 0;
        if (mine) {
            px = xb[3 * r]; py = xb[3 * r + 1]; pz = xb[3 * r + 2];
            ti = first_maximum(hb + size_t(r) * nf, nf);
        }
        for (int tile = 0; tile < tiles; ++tile) {
            const int j = tile * TILE + tid;
            float4 cand = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
            int cg = 0;
            if (j < N && (cg = grp[j]) != 0)
                cand = make_float4(xb[3 * j], xb[3 * j + 1], xb[3 * j + 2], __int_as_float(first_maximum(hb + size_t(j) * nf, nf)));
            __syncthreads();                                             // the previous tile has been read
            s_tile[tid] = cand;
            s_group[tid] = cg;
            __syncthreads();
            if (!mine) continue;
            const int n_in = min(TILE, N - tile * TILE);
            for (int jj = 0; jj < n_in; ++jj) {
                const int row = tile * TILE + jj;
                if (s_group[jj] != mine || row == r) continue;
                const float4 t = s_tile[jj];
                const int tj = __float_as_int(t.w);
                const float dx = px - t.x, dy = py - t.y, dz = pz - t.z;
                const float bound = row < r ? s_table[ti * MAX_TYPES + tj] : s_table[tj * MAX_TYPES + ti];
                if (bond_distance_pm(dx, dy, dz) < bound) {
                    if (deg == 0) first = row;
                    ++deg;
                    hetero |= tj != EL_C;
                }
            }
        }
        // The d2 of the first neighbour, which only an oxygen with one neighbour asks for, is evaluated here and not in the
        // loop: there its products would be shared with bond_distance_pm's, and the uncontracted ones would win - the bond
        // distance would no longer round as it does in bonds.hip
        float first_d2 = 0.0f;
        if (deg == 1) first_d2 = dist2_f32(px - xb[3 * first], py - xb[3 * first + 1], pz - xb[3 * first + 2]);
        if (r < N) out[r] = mine ? xs_flags(ti, deg, hetero, first_d2) : -1;
    }
    if (tid == 0) a.status[b] = 0;
}

// ---- scores -------------------------------------------------------------------------------------------------------------------
struct PairSums {
    long long t[TERMS];
};

__device__ __forceinline__ long long fixed(double term) { return llrint(term * 4294967296.0); }

// the pair loop of one tile: QPT queries in this lane's registers against entries g, g + G, ... of the tile
template <int QPT>
__device__ __forceinline__ void score_tile(const float4* s_tile, const double* s_radius, int g, int G, const double (&qx)[QPT_MAX],
                                           const double (&qy)[QPT_MAX], const double (&qz)[QPT_MAX], const double (&qr)[QPT_MAX],
                                           const int (&qs)[QPT_MAX], PairSums (&sum)[QPT_MAX], int& pairs, int& hbonds, int& hydro) {
    for (int j = g; j < TILE; j += G) {
        const float4 t = s_tile[j];
        const int ts = __float_as_int(t.w);
        if (ts < 0) continue;
        const double tx = t.x, ty = t.y, tz = t.z, tr = s_radius[ts & ELEM_MASK];
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            if (qs[q] < 0) continue;
            const double dx = qx[q] - tx, dy = qy[q] - ty, dz = qz[q] - tz;
            const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            if (!(d2 < 64.0)) continue;
            const double s = sqrt(d2) - (qr[q] + tr);
            const double u = s / 0.5, v = (s - 3.0) / 2.0;
            sum[q].t[0] += fixed(exp(-(u * u)));
            sum[q].t[1] += fixed(exp(-(v * v)));
            if (s < 0.0) sum[q].t[2] += fixed(s * s);
            ++pairs;
            if ((qs[q] & ts & DL_XS_HYDROPHOBIC) && s < 1.5) {
                sum[q].t[3] += fixed(s < 0.5 ? 1.0 : 1.5 - s);
                ++hydro;
            }
            const bool pairing = ((qs[q] & DL_XS_DONOR) && (ts & DL_XS_ACCEPTOR)) || ((qs[q] & DL_XS_ACCEPTOR) && (ts & DL_XS_DONOR));
            if (pairing && s < 0.0) {
                sum[q].t[4] += fixed(s < -0.7 ? 1.0 : -s / 0.7);
                ++hbonds;
            }
        }
    }
}

__global__ __launch_bounds__(WG) void interaction_scores_kernel(dl_interact_args a) {
    __shared__ float4 s_tile[TILE];
    __shared__ double s_radius[MAX_TYPES];
    __shared__ __align__(16) long long s_part[TERMS * INTERACT_MAX_QUERY];   // first the staged queries (x, y, z, xs_type), then the partials
    __shared__ int s_scan[WG_WAVES];
    __shared__ long long s_wide[WG_WAVES];
    float4* s_q = reinterpret_cast<float4*>(s_part);

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf;
    const float* qmask = a.query_mask + size_t(b) * N;
    const float* tmask = a.target_mask ? a.target_mask + size_t(b) * N : nullptr;
    const float* xb = a.x + size_t(b) * N * 3;
    const int* xs = a.xs_type + size_t(b) * N;

    // ---- count and compact the query rows: thread t owns rows [r0, r1)
    const Rows rows = own_rows(N);
    const int r0 = rows.r0, r1 = rows.r1;
    int nq = 0;
    const int k0 = block_exclusive_scan(count_rows(rows, qmask), s_scan, nq);
    int status = nq > INTERACT_MAX_QUERY ? DL_INTERACT_TOO_LARGE : 0;    // uniform over the workgroup
    int n_target = 0, pairs = 0, hbonds = 0, hydro = 0;
    int Qpad = 1;
    while (Qpad < nq && Qpad < WG) Qpad <<= 1;
    const int G = WG / Qpad;

    if (!status) {
        if (tid < MAX_TYPES) s_radius[tid] = tid < nf ? a.radius[tid] : 0.0;
        int bad = 0, bad_type = 0, untyped = 0;
        int k = k0;
        for (int r = r0; r < r1; ++r) {
            if (qmask[r] == 0.0f) continue;
            const float px = xb[3 * r], py = xb[3 * r + 1], pz = xb[3 * r + 2];
            const int t = xs[r];
            bad |= !finite3(px, py, pz);
            untyped |= t < 0 || (t & ELEM_MASK) >= nf;
            s_q[k++] = make_float4(px, py, pz, __int_as_float(t));
        }
        __syncthreads();

        // ---- this thread's queries: group g of G, lane ql of Qpad
        const int ql = tid & (Qpad - 1), g = tid / Qpad;
        const bool many = nq > WG;
        double qx[QPT_MAX], qy[QPT_MAX], qz[QPT_MAX], qr[QPT_MAX];
        int qs[QPT_MAX];
        PairSums sum[QPT_MAX];
#pragma unroll
        for (int q = 0; q < QPT_MAX; ++q) {
            const int kq = ql + q * WG;
            const bool have = kq < nq && (q == 0 || many);
            const float4 v = have ? s_q[kq] : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            qx[q] = v.x; qy[q] = v.y; qz[q] = v.z; qs[q] = __float_as_int(v.w);
            qr[q] = qs[q] >= 0 ? s_radius[qs[q] & ELEM_MASK] : 0.0;
#pragma unroll
            for (int c = 0; c < TERMS; ++c) sum[q].t[c] = 0;
        }

        // ---- stream the targets: the molecule's own rows, then the shared list
        const int own_tiles = tmask ? (N + TILE - 1) / TILE : 0;
        const int shared_tiles = (a.M + TILE - 1) / TILE;
        for (int tile = 0; tile < own_tiles + shared_tiles; ++tile) {
            float4 cand = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            if (tile < own_tiles) {
                const int r = tile * TILE + tid;
                if (r < N && tmask[r] != 0.0f && qmask[r] == 0.0f) {
                    const int t = xs[r];
                    if (t < 0 || (t & ELEM_MASK) >= nf) untyped = 1;
                    else cand = make_float4(xb[3 * r], xb[3 * r + 1], xb[3 * r + 2], __int_as_float(t));
                }
            } else {
                const int j = (tile - own_tiles) * TILE + tid;
                if (j < a.M) {
                    const int t = a.target_xs[j];
                    if (t < 0 || (t & ELEM_MASK) >= nf) bad_type = 1;    // skipped: its coordinates are not looked at
                    else cand = make_float4(a.target_x[3 * size_t(j)], a.target_x[3 * size_t(j) + 1],
                                            a.target_x[3 * size_t(j) + 2], __int_as_float(t));
                }
            }
            if (__float_as_int(cand.w) >= 0) {
                bad |= !finite3(cand.x, cand.y, cand.z);
                ++n_target;
            }
            __syncthreads();                                             // the previous tile has been read
            s_tile[tid] = cand;
            __syncthreads();
            if (many) score_tile<QPT_MAX>(s_tile, s_radius, g, G, qx, qy, qz, qr, qs, sum, pairs, hbonds, hydro);
            else score_tile<1>(s_tile, s_radius, g, G, qx, qy, qz, qr, qs, sum, pairs, hbonds, hydro);
        }
        if (__syncthreads_or(bad)) status |= DL_INTERACT_NONFINITE;      // (also: every read of the staged queries is done)
        if (__syncthreads_or(bad_type)) status |= DL_INTERACT_BAD_TYPE;
        if (__syncthreads_or(untyped)) status |= DL_INTERACT_UNTYPED;
        n_target = block_sum(n_target, s_scan);

        // ---- the groups' partials of every query meet: slot q * 256 + tid of term c is this thread's own
#pragma unroll
        for (int q = 0; q < QPT_MAX; ++q)
#pragma unroll
            for (int c = 0; c < TERMS; ++c) s_part[c * INTERACT_MAX_QUERY + q * WG + tid] = sum[q].t[c];
        __syncthreads();
        for (int kq = tid; kq < nq; kq += WG) {                          // with G > 1, nq <= Qpad: column kq is this thread's alone
            for (int c = 0; c < TERMS; ++c) {
                long long v = s_part[c * INTERACT_MAX_QUERY + kq];
                for (int gg = 1; gg < G; ++gg) v += s_part[c * INTERACT_MAX_QUERY + gg * Qpad + kq];
                s_part[c * INTERACT_MAX_QUERY + kq] = v;
            }
        }
        __syncthreads();
    }

    // ---- write: this thread's rows, and the molecule's sums over them
    const bool dead = (status & (DL_INTERACT_TOO_LARGE | DL_INTERACT_NONFINITE | DL_INTERACT_UNTYPED)) != 0;
    long long total[TERMS];
#pragma unroll
    for (int c = 0; c < TERMS; ++c) total[c] = 0;
    int k = k0;
    for (int r = r0; r < r1; ++r) {
        long long v[TERMS];
#pragma unroll
        for (int c = 0; c < TERMS; ++c) v[c] = 0;
        if (qmask[r] != 0.0f) {
            if (!dead) {
#pragma unroll
                for (int c = 0; c < TERMS; ++c) {
                    v[c] = s_part[c * INTERACT_MAX_QUERY + k];
                    total[c] += v[c];
                }
            }
            ++k;
        }
#pragma unroll
        for (int c = 0; c < TERMS; ++c) a.atom_terms[(size_t(b) * N + r) * TERMS + c] = v[c];
    }
#pragma unroll
    for (int c = 0; c < TERMS; ++c) total[c] = block_sum(total[c], s_wide);
    pairs = block_sum(pairs, s_scan);
    hbonds = block_sum(hbonds, s_scan);
    hydro = block_sum(hydro, s_scan);
    if (tid == 0) {
        a.n_query[b] = dead ? 0 : nq;
        a.n_target[b] = dead ? 0 : n_target;
        a.n_pairs[b] = dead ? 0 : pairs;
        a.n_hbonds[b] = dead ? 0 : hbonds;
        a.n_hydrophobic[b] = dead ? 0 : hydro;
#pragma unroll
        for (int c = 0; c < TERMS; ++c) a.terms[size_t(b) * TERMS + c] = dead ? 0 : total[c];
        a.status[b] = status;
    }
}

}  // namespace

extern "C" {

int32_t dl_interaction_types(const dl_interact_types_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->nf < 1 || a->nf > MAX_TYPES) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->group || !a->table || !a->xs_type || !a->status) return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(interaction_types_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_interaction_scores(const dl_interact_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->nf < 1 || a->nf > MAX_TYPES || a->M < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->xs_type || !a->query_mask || !a->radius || !a->n_query || !a->n_target || !a->n_pairs || !a->n_hbonds ||
        !a->n_hydrophobic || !a->terms || !a->status || !a->atom_terms || (a->M > 0 && (!a->target_x || !a->target_xs)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(interaction_scores_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
