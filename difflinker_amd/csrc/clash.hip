// clash.hip — steric clashes of generated atoms with the protein: for every molecule of a batch the pairs of one QUERY atom
// (a generated atom) and one TARGET atom (a protein atom) that sit closer than a per-element-pair threshold.  The reference
// has no code for this (its paper reports the counts, its scripts do not compute them), so the rule is this project's own
// and is stated here in full; tests/clash_ref.py restates it in numpy float32 and gives the same bits.
//
// THE RULE.  Heavy atoms only, hydrogens implicit.  The host builds threshold[a][b] in fp32 Angstrom (const.
// clash_threshold_table: scale * (r_vdw[a] + r_vdw[b]) - tolerance, fp64 rounded once), a the query's type, b the target's.
// An atom's type is the index of the first largest entry of its one-hot row, as bonds.hip reads it.  For a pair
//     dx = xq - xt (dy, dz alike),   d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
// every operation a separate fp32 round-to-nearest operation in exactly this order: contraction is OFF for this file, no
// fused multiply-add may replace a multiply and an add.  With t = threshold[a][b] the pair
//     CLASHES      when d2 < t * t and t > 0        (t * t one fp32 multiply, the comparison strict)
//     is a CONTACT when d2 < c * c                  (c the scalar contact_cutoff, same arithmetic)
// Every output is an integer count or a minimum of such d2: the same bits on every run and under every mapping.
//
// A molecule's query atoms are its rows with query_mask != 0; its targets are its rows with target_mask != 0 that are not
// query rows (a row in both masks is a query), followed by the shared list (target_x, target_type), the same for every
// molecule of the launch.  Rows in neither mask are never read, whatever they hold.
//
// THE MAPPING.  One 256-thread workgroup per molecule, ONE launch per batch.
//   stage    the query rows are compacted in row order (thread t owns a contiguous run of rows; a block scan gives its first
//            slot) and each thread takes its queries into registers: with nq <= 256 queries, lane ql = tid % Qpad holds query ql
//            (Qpad the power of two >= nq) and the G = 256 / Qpad lane groups split the targets; with more, each thread holds up
//            to four queries and G = 1.  The squared-threshold table goes to LDS TRANSPOSED, t2[b * 16 + a]: the lanes of a
//            group share the target type b, so their reads fall on at most 16 consecutive words - no bank conflict.
//   stream   targets pass through a 256-entry LDS tile (x, y, z, type; type -1 = no target in this slot): every thread loads
//            one candidate (a row of the molecule, then an atom of the shared list), the workgroup meets, and group g walks
//            entries g, g + G, ... of the tile against its queries.  All lanes of a group read the same tile entry: an LDS
//            broadcast.  Counts and the minimum stay in the lane's registers; nothing crosses lanes in the pair loop.
//   reduce   the groups' partials of a query meet through LDS (integer sums and minima: the order does not matter), then the
//            per-molecule sums over the queries by wave shuffles and one more LDS step.
//   write    the thread that owns a row writes its two per-atom outputs, query row or not: every output is written in full.
//
// Global memory is written with plain vector stores only; no atomics of any kind, in LDS or in global memory.
#include "workgroup.h"

#pragma clang fp contract(off)

namespace {

constexpr int CLASH_MAX_QUERY = 1024;            // four queries per thread at most
constexpr int QPT_MAX = CLASH_MAX_QUERY / WG;
constexpr int MAX_TYPES = 16;
constexpr int TILE = WG;                         // targets per LDS tile: one candidate per thread

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the pair loop of one tile: QPT queries in this lane's registers against entries g, g + G, ... of the tile
template <int QPT>
__device__ __forceinline__ void score_tile(const float4* s_tile, const float* s_t2, int g, int G, float c2, const float (&qx)[QPT_MAX],
                                           const float (&qy)[QPT_MAX], const float (&qz)[QPT_MAX], const int (&qa)[QPT_MAX],
                                           int (&cnt)[QPT_MAX], int (&con)[QPT_MAX], float (&mn)[QPT_MAX]) {
    for (int j = g; j < TILE; j += G) {
        const float4 t = s_tile[j];
        const int tb = __float_as_int(t.w);
        if (tb < 0) continue;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            if (qa[q] < 0) continue;
            const float dx = qx[q] - t.x, dy = qy[q] - t.y, dz = qz[q] - t.z;
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);         // contraction is off: five roundings, in this order
            cnt[q] += d2 < s_t2[tb * MAX_TYPES + qa[q]];
            con[q] += d2 < c2;
            mn[q] = d2 < mn[q] ? d2 : mn[q];
        }
    }
}

__global__ __launch_bounds__(WG) void clash_scores_kernel(dl_clash_args a) {
    __shared__ float4 s_tile[TILE];
    __shared__ float s_t2[MAX_TYPES * MAX_TYPES];
    __shared__ float4 s_q[CLASH_MAX_QUERY];      // staged queries (x, y, z, type), then the partials: x = clashes, y = contacts, z = minimum
    __shared__ int s_scan[WG_WAVES];
    __shared__ float s_min[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf;
    const float* qmask = a.query_mask + size_t(b) * N;
    const float* tmask = a.target_mask ? a.target_mask + size_t(b) * N : nullptr;
    const float* xb = a.x + size_t(b) * N * 3;
    const float* hb = a.one_hot + size_t(b) * N * nf;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");

    // ---- count and compact the query rows: thread t owns rows [r0, r1)
    const Rows rows = own_rows(N);
    const int r0 = rows.r0, r1 = rows.r1;
    int nq = 0;
    const int k0 = block_exclusive_scan(count_rows(rows, qmask), s_scan, nq);
    int status = nq > CLASH_MAX_QUERY ? DL_CLASH_TOO_LARGE : 0;          // uniform over the workgroup
    int n_target = 0;

    if (!status) {
        for (int k = tid; k < MAX_TYPES * MAX_TYPES; k += WG) {          // t2[b * 16 + a] = threshold[a][b]^2, 0 = never
            const int tb = k / MAX_TYPES, qa = k % MAX_TYPES;
            const float t = (tb < nf && qa < nf) ? a.threshold[qa * nf + tb] : 0.0f;
            s_t2[k] = t > 0.0f ? t * t : 0.0f;                           // d2 >= +0, so `d2 < 0` never holds
        }
        int bad = 0, bad_type = 0;
        int k = k0;
        for (int r = r0; r < r1; ++r) {
            if (qmask[r] == 0.0f) continue;
            const float px = xb[3 * r], py = xb[3 * r + 1], pz = xb[3 * r + 2];
            bad |= !finite3(px, py, pz);
            s_q[k++] = make_float4(px, py, pz, __int_as_float(first_maximum(hb + size_t(r) * nf, nf)));
        }
        __syncthreads();

        // ---- this thread's queries: group g of G, lane ql of Qpad
        int Qpad = 1;
        while (Qpad < nq && Qpad < WG) Qpad <<= 1;
        const int G = WG / Qpad, ql = tid & (Qpad - 1), g = tid / Qpad;
        const bool many = nq > WG;
        float qx[QPT_MAX], qy[QPT_MAX], qz[QPT_MAX], mn[QPT_MAX];
        int qa[QPT_MAX], cnt[QPT_MAX], con[QPT_MAX];
#pragma unroll
        for (int q = 0; q < QPT_MAX; ++q) {
            const int kq = ql + q * WG;
            const bool have = kq < nq && (q == 0 || many);
            const float4 v = have ? s_q[kq] : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            qx[q] = v.x; qy[q] = v.y; qz[q] = v.z; qa[q] = __float_as_int(v.w);
            cnt[q] = 0; con[q] = 0; mn[q] = inf;
        }
        const float c2 = a.contact_cutoff * a.contact_cutoff;

        // ---- stream the targets: the molecule's own rows, then the shared list
        const int own_tiles = tmask ? (N + TILE - 1) / TILE : 0;
        const int shared_tiles = (a.M + TILE - 1) / TILE;
        for (int tile = 0; tile < own_tiles + shared_tiles; ++tile) {
            float4 cand = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            if (tile < own_tiles) {
                const int r = tile * TILE + tid;
                if (r < N && tmask[r] != 0.0f && qmask[r] == 0.0f)
                    cand = make_float4(xb[3 * r], xb[3 * r + 1], xb[3 * r + 2],
                                       __int_as_float(first_maximum(hb + size_t(r) * nf, nf)));
            } else {
                const int j = (tile - own_tiles) * TILE + tid;
                if (j < a.M) {
                    const int tb = a.target_type[j];
                    if (tb < 0 || tb >= nf) bad_type = 1;                // skipped: its coordinates are not looked at
                    else cand = make_float4(a.target_x[3 * size_t(j)], a.target_x[3 * size_t(j) + 1],
                                            a.target_x[3 * size_t(j) + 2], __int_as_float(tb));
                }
            }
            if (__float_as_int(cand.w) >= 0) {
                bad |= !finite3(cand.x, cand.y, cand.z);
                ++n_target;
            }
            __syncthreads();                                             // the previous tile has been read
            s_tile[tid] = cand;
            __syncthreads();
            if (many) score_tile<QPT_MAX>(s_tile, s_t2, g, G, c2, qx, qy, qz, qa, cnt, con, mn);
            else score_tile<1>(s_tile, s_t2, g, G, c2, qx, qy, qz, qa, cnt, con, mn);
        }
        if (__syncthreads_or(bad)) status |= DL_CLASH_NONFINITE;
        if (__syncthreads_or(bad_type)) status |= DL_CLASH_BAD_TYPE;
        n_target = block_sum(n_target, s_scan);

        // ---- the groups' partials of every query meet: slot q * 256 + tid is this thread's own
#pragma unroll
        for (int q = 0; q < QPT_MAX; ++q)
            s_q[q * WG + tid] = make_float4(__int_as_float(cnt[q]), __int_as_float(con[q]), mn[q], 0.0f);
        __syncthreads();
        for (int kq = tid; kq < nq; kq += WG) {                          // with G > 1, nq <= Qpad: column kq is this thread's alone
            float4 sum = s_q[kq];
            int c = __float_as_int(sum.x), n = __float_as_int(sum.y);
            for (int gg = 1; gg < G; ++gg) {
                const float4 v = s_q[gg * Qpad + kq];
                c += __float_as_int(v.x);
                n += __float_as_int(v.y);
                sum.z = v.z < sum.z ? v.z : sum.z;
            }
            s_q[kq] = make_float4(__int_as_float(c), __int_as_float(n), sum.z, 0.0f);
        }
        __syncthreads();
    }

    // ---- write: this thread's rows, and the molecule's sums over them
    const bool dead = (status & (DL_CLASH_TOO_LARGE | DL_CLASH_NONFINITE)) != 0;
    int clashes = 0, clash_atoms = 0, contacts = 0;
    float closest = inf;
    int k = k0;
    for (int r = r0; r < r1; ++r) {
        int c = 0;
        float m = inf;
        if (qmask[r] != 0.0f) {
            if (dead) {
                m = nan;
            } else {
                const float4 v = s_q[k];
                c = __float_as_int(v.x);
                m = v.z;
                clashes += c;
                clash_atoms += c > 0;
                contacts += __float_as_int(v.y);
                closest = m < closest ? m : closest;
            }
            ++k;
        }
        a.atom_clashes[size_t(b) * N + r] = c;
        a.atom_min_dist2[size_t(b) * N + r] = m;
    }
    clashes = block_sum(clashes, s_scan);
    clash_atoms = block_sum(clash_atoms, s_scan);
    contacts = block_sum(contacts, s_scan);
    closest = block_min(closest, s_min);
    if (tid == 0) {
        a.n_query[b] = dead ? 0 : nq;
        a.n_target[b] = dead ? 0 : n_target;
        a.n_clashes[b] = dead ? 0 : clashes;
        a.n_clash_atoms[b] = dead ? 0 : clash_atoms;
        a.n_contacts[b] = dead ? 0 : contacts;
        a.min_dist2[b] = dead ? nan : closest;
        a.status[b] = status;
    }
}

}  // namespace

extern "C" {

int32_t dl_clash_scores(const dl_clash_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->nf < 1 || a->nf > MAX_TYPES || a->M < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->query_mask || !a->threshold || !a->n_query || !a->n_target || !a->n_clashes ||
        !a->n_clash_atoms || !a->n_contacts || !a->min_dist2 || !a->status || !a->atom_clashes || !a->atom_min_dist2 ||
        (a->M > 0 && (!a->target_x || !a->target_type)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(clash_scores_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
