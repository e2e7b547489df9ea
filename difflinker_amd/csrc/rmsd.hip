// rmsd.hip — symmetry-aware RMSD of recovered molecules: for every (pred, true) pair of a list the smallest rigid-alignment
// RMSD over a table of atom correspondences (the graph isomorphisms metrics.isomorphisms enumerated), proper rotations
// only.  What the reference asks of RDKit in compute_metrics.py:366-402 (rdMolAlign.GetBestRMS), asked of the coordinates.
//
// One 256-thread workgroup per pair, ONE launch per list.  A pair with one map keeps one lane busy in the map loop and the
// whole workgroup in staging and in the final residual; a pair with thousands of maps gives every lane 16 and more.
//
//   stage     both coordinate sets into LDS as float4 (x, y, z, 0); centroids by an fp64 block sum; the sets are centred in
//             fp64, rounded to fp32 once and written back.  Ga = sum |a_k|^2 and Gb = sum |b_k|^2 are taken from the values
//             as stored.  None of this depends on the map: a map is a bijection over all n atoms.
//   maps      lane j takes maps j, j + 256, ...: S = sum_k a_k (x) b_image[k] in fp64 (image indices read from the table,
//             consecutive lanes consecutive 16-bit words; a_k is an LDS broadcast, b a 16-byte LDS gather), then the largest
//             eigenvalue lambda of Horn's symmetric 4x4 quaternion matrix N(S) by cyclic Jacobi sweeps.  The candidate is
//             Ga + Gb - 2 lambda (n times the mean square deviation).  Reflections never enter: every unit quaternion is a
//             proper rotation.  The lane keeps S of its best map.
//   reduce    (minimum, lowest index) over the wave by shuffles, over the four waves through LDS.  Equal maps give equal
//             bits (the same operations in the same order), so ties go to the lowest index on every run.
//   winner    the lane that owns the winning map repeats the Jacobi sweeps with the eigenvectors, turns the eigenvector of
//             lambda into the rotation R, and the workgroup sums |R a_k - b_image[k]|^2 directly.  The difference
//             Ga + Gb - 2 lambda cancels when the structures coincide; the direct sum does not.
//
// WHY fp64 WHERE IT IS.  The bar is 5e-4 A absolute on the RMSD, also when the RMSD is 0.  With S and lambda in fp32 a
// candidate n * msd carries an error of about 1e-7 (Ga + Gb), some 1e-5 A^2 in msd for a drug-sized molecule: two maps whose
// true msd are 0 and 1e-5 A^2 (a nearly symmetric structure on top of itself) could swap places and the answer would be
// 3e-3 A instead of 0.  In fp64 the same error is 1e-14 A^2.  The coordinates in LDS stay fp32: centring rounds each by at most half an ulp of a
// centred coordinate (5e-7 A at 8 A from the centroid), which moves every candidate and the final RMSD by no more than that.
//
// A table entry beyond the atom count is clamped to the last atom (no fault, a meaningless value for that map): the table is
// the caller's promise of bijections.  Offsets that leave the table give DL_RMSD_NO_MAP.
//
// Global memory is written with plain vector stores only; no global atomics of any kind.
#include <climits>
#include "workgroup.h"

namespace {

constexpr int RMSD_MAX_ATOMS = 1024;             // 2 x 16 bytes of LDS per atom: 32 KiB
constexpr int RED_DOUBLES = 16;                  // LDS scratch behind the coordinates: 4 wave partials, 4 wave indices, 9 of R
constexpr int MAX_SWEEPS = 16;                   // cyclic Jacobi on a symmetric 4x4 settles in 5 to 7

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                    // lane 0 holds the sum
}

// sum of one double per thread over the workgroup, the same value in every thread; the order of the additions is fixed
__device__ __forceinline__ double block_sum(double v, double* red /* [WG_WAVES] */) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < WG_WAVES; ++w) s += red[w];
    __syncthreads();
    return s;
}

// Horn's matrix of S = sum a (x) b, S[3 r + c] = sum a_r b_c: its largest eigenvalue is max over rotations of sum (R a) . b,
// its eigenvector (q0, qx, qy, qz) the quaternion of that rotation
__device__ __forceinline__ void horn_matrix(const double* S, double N[4][4]) {
    const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
    N[0][0] = xx + yy + zz;
    N[1][1] = xx - yy - zz;
    N[2][2] = -xx + yy - zz;
    N[3][3] = -xx - yy + zz;
    N[0][1] = N[1][0] = yz - zy;
    N[0][2] = N[2][0] = zx - xz;
    N[0][3] = N[3][0] = xy - yx;
    N[1][2] = N[2][1] = xy + yx;
    N[1][3] = N[3][1] = zx + xz;
    N[2][3] = N[3][2] = yz + zy;
}

// cyclic Jacobi on the symmetric 4x4 A (destroyed); returns the position of the largest eigenvalue on the diagonal, first of
// equals, and the eigenvalue through `lambda`.  With VEC the columns of V are the eigenvectors.  No division by anything that can be zero: a rotation is applied
// only to an off-diagonal element that is not, and the zero matrix (n = 1) leaves at once with V = 1.
template <bool VEC>
__device__ __forceinline__ int jacobi4(double A[4][4], double V[4][4], double& lambda) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            diag += A[i][i] * A[i][i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        }
        if (off <= 1e-34 * diag || off == 0.0) break;          // off-diagonal below fp64 rounding of the diagonal
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = A[p][r] = c * arp - s * arq;
                    A[r][q] = A[q][r] = s * arp + c * arq;
                }
                if (VEC) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double vrp = V[r][p], vrq = V[r][q];
                        V[r][p] = c * vrp - s * vrq;
                        V[r][q] = s * vrp + c * vrq;
                    }
                }
            }
        }
    }
    int top = 0;
    lambda = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > lambda) { lambda = A[i][i]; top = i; }
    return top;
}

__global__ __launch_bounds__(WG) void best_rmsd_kernel(dl_rmsd_args a, int atoms_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float4* s_a = reinterpret_cast<float4*>(lds_raw);
    float4* s_b = s_a + atoms_lds;
    double* s_red = reinterpret_cast<double*>(s_b + atoms_lds);      // [WG_WAVES]
    int* s_idx = reinterpret_cast<int*>(s_red + WG_WAVES);           // [WG_WAVES] (two doubles' room)
    double* s_rot = s_red + WG_WAVES + 2;                            // [9]

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n_atoms[p];
    const long long first = a.map_offsets[p], last = a.map_offsets[p + 1];
    int status = 0;
    if (n > a.n_max || n > RMSD_MAX_ATOMS) status |= DL_RMSD_TOO_LARGE;
    if (n < 1 || first < 0 || last <= first || last > a.maps_capacity) status |= DL_RMSD_NO_MAP;
    if (status) {                                // uniform over the workgroup
        if (tid == 0) {
            a.rmsd[p] = __builtin_nanf("");
            a.best[p] = -1;
            a.status[p] = status;
        }
        return;
    }
    const int m = int(last - first);

    // ---- stage: raw coordinates and their sums
    const float* xa = a.xa + size_t(p) * a.n_max * 3;
    const float* xb = a.xb + size_t(p) * a.n_max * 3;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int k = tid; k < n; k += WG) {
        const float4 va = make_float4(xa[3 * k], xa[3 * k + 1], xa[3 * k + 2], 0.0f);
        const float4 vb = make_float4(xb[3 * k], xb[3 * k + 1], xb[3 * k + 2], 0.0f);
        bad |= !(isfinite(va.x) && isfinite(va.y) && isfinite(va.z) && isfinite(vb.x) && isfinite(vb.y) && isfinite(vb.z));
        s_a[k] = va;
        s_b[k] = vb;
        sum[0] += va.x; sum[1] += va.y; sum[2] += va.z;
        sum[3] += vb.x; sum[4] += vb.y; sum[5] += vb.z;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            a.rmsd[p] = __builtin_nanf("");
            a.best[p] = -1;
            a.status[p] = DL_RMSD_NONFINITE;
        }
        return;
    }
    double centre[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) centre[c] = block_sum(sum[c], s_red) / n;

    // ---- centre (each thread its own atoms again), Ga + Gb of the values as stored
    double g = 0.0;
    for (int k = tid; k < n; k += WG) {
        float4 va = s_a[k], vb = s_b[k];
        va.x = float(double(va.x) - centre[0]); va.y = float(double(va.y) - centre[1]); va.z = float(double(va.z) - centre[2]);
        vb.x = float(double(vb.x) - centre[3]); vb.y = float(double(vb.y) - centre[4]); vb.z = float(double(vb.z) - centre[5]);
        s_a[k] = va;
        s_b[k] = vb;
        g += double(va.x) * va.x + double(va.y) * va.y + double(va.z) * va.z;
        g += double(vb.x) * vb.x + double(vb.y) * vb.y + double(vb.z) * vb.z;
    }
    const double G = block_sum(g, s_red);        // its barriers also publish the centred coordinates

    // ---- maps: entry (k, j) of this pair's block is tab[k * m + j]
    const uint16_t* tab = a.maps + size_t(first) * a.n_max;
    double best = __builtin_inf(), best_S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int best_j = INT_MAX;
    for (int j = tid; j < m; j += WG) {
        double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const uint16_t* col = tab + j;
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const int image = min(int(col[size_t(k) * m]), n - 1);
            const float4 va = s_a[k], vb = s_b[image];
            const double ax = va.x, ay = va.y, az = va.z, bx = vb.x, by = vb.y, bz = vb.z;
            S[0] += ax * bx; S[1] += ax * by; S[2] += ax * bz;
            S[3] += ay * bx; S[4] += ay * by; S[5] += ay * bz;
            S[6] += az * bx; S[7] += az * by; S[8] += az * bz;
        }
        double N[4][4];
        horn_matrix(S, N);
        double lambda;
        jacobi4<false>(N, N, lambda);
        const double cand = G - 2.0 * lambda;
        if (cand < best) {                       // j only grows: the lowest index of equal candidates stays
            best = cand;
            best_j = j;
#pragma unroll
            for (int c = 0; c < 9; ++c) best_S[c] = S[c];
        }
    }

    // ---- reduce (minimum, lowest index)
    double rv = best;
    int rj = best_j;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(rv, off, 64);
        const int oj = __shfl_down(rj, off, 64);
        if (ov < rv || (ov == rv && oj < rj)) { rv = ov; rj = oj; }
    }
    if (lane == 0) { s_red[w] = rv; s_idx[w] = rj; }
    __syncthreads();
    rv = s_red[0];
    rj = s_idx[0];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) {
        const double ov = s_red[k];
        const int oj = s_idx[k];
        if (ov < rv || (ov == rv && oj < rj)) { rv = ov; rj = oj; }
    }
    __syncthreads();
    if (rj == INT_MAX) {                         // no candidate compared below infinity: the sums overflowed
        if (tid == 0) {
            a.rmsd[p] = __builtin_nanf("");
            a.best[p] = -1;
            a.status[p] = DL_RMSD_NONFINITE;
        }
        return;
    }

    // ---- winner: the rotation from the eigenvector, then the residual itself
    if (tid == rj % WG) {
        double N[4][4], V[4][4];
        horn_matrix(best_S, N);
        double lambda;
        const int top = jacobi4<true>(N, V, lambda);
        double q0 = 1.0, qx = 0.0, qy = 0.0, qz = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)              // a selection, not an index: V stays in registers
            if (c == top) { q0 = V[0][c]; qx = V[1][c]; qy = V[2][c]; qz = V[3][c]; }
        const double len = sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);
        q0 /= len; qx /= len; qy /= len; qz /= len;
        s_rot[0] = q0 * q0 + qx * qx - qy * qy - qz * qz;
        s_rot[1] = 2.0 * (qx * qy - q0 * qz);
        s_rot[2] = 2.0 * (qx * qz + q0 * qy);
        s_rot[3] = 2.0 * (qy * qx + q0 * qz);
        s_rot[4] = q0 * q0 - qx * qx + qy * qy - qz * qz;
        s_rot[5] = 2.0 * (qy * qz - q0 * qx);
        s_rot[6] = 2.0 * (qz * qx - q0 * qy);
        s_rot[7] = 2.0 * (qz * qy + q0 * qx);
        s_rot[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
    }
    __syncthreads();
    double R[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = s_rot[c];
    const uint16_t* col = tab + rj;
    double res = 0.0;
    for (int k = tid; k < n; k += WG) {
        const int image = min(int(col[size_t(k) * m]), n - 1);
        const float4 va = s_a[k], vb = s_b[image];
        const double ax = va.x, ay = va.y, az = va.z;
        const double dx = R[0] * ax + R[1] * ay + R[2] * az - vb.x;
        const double dy = R[3] * ax + R[4] * ay + R[5] * az - vb.y;
        const double dz = R[6] * ax + R[7] * ay + R[8] * az - vb.z;
        res += dx * dx + dy * dy + dz * dz;
    }
    res = block_sum(res, s_red);
    if (tid == 0) {
        a.rmsd[p] = float(sqrt(res / n));
        a.best[p] = rj;
        a.status[p] = 0;
    }
}

}  // namespace

extern "C" {

int32_t dl_best_rmsd(const dl_rmsd_args* a, void* stream) {
    if (!a || a->P < 0 || a->n_max < 1 || a->n_max > 65536 || a->maps_capacity < 0) return DL_ERR_BAD_ARG;
    if (a->P == 0) return DL_OK;                 // an empty list has nothing to point at
    if (!a->xa || !a->xb || !a->n_atoms || !a->map_offsets || !a->rmsd || !a->best || !a->status ||
        (a->maps_capacity > 0 && !a->maps))
        return DL_ERR_BAD_ARG;
    const int atoms_lds = a->n_max < RMSD_MAX_ATOMS ? a->n_max : RMSD_MAX_ATOMS;
    const size_t lds = size_t(atoms_lds) * 2 * sizeof(float4) + RED_DOUBLES * sizeof(double);
    hipLaunchKernelGGL(best_rmsd_kernel, dim3(a->P), dim3(WG), lds, static_cast<hipStream_t>(stream), *a, atoms_lds);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
