// edm_loss.hip — the diffusion loss / variational lower bound of held-out data (reference EDM.forward, src/edm.py:41-124,
// and InpaintingEDM.forward, :467-548), around the unchanged denoiser forward of egnn_fc.hip / egnn_sparse.hip.
//
// Two kernels, one 256-thread workgroup per molecule each:
//
//   prologue  t_int (given, or drawn) -> t = t_int / T, gamma_t = table[round(t * timesteps)], gamma_s = table[round(s * timesteps)]
//             with s = (t_int - 1) / T (a negative index reads from the end of the table, as the reference's indexing does:
//             t_int = 0 reads gamma_s = table[timesteps]; the term it feeds is masked later but stays finite);
//             eps (given, or drawn) masked by the noise mask, with the centre of gravity of its x-part removed for inpainting
//             (utils.py:158-168); z_t = xh fragment_mask + (alpha_t xh + sigma_t eps) linker_mask   (EDM)
//                   z_t = alpha_t xh + sigma_t eps                                                  (InpaintingEDM)
//   epilogue  per molecule the row of DL_LOSS_ROW floats (include/difflinker_hip.h): error_t, |eps_hat|_F, kl_prior,
//             log p(x | z_0) and log p(h | z_0) without constants, the log constant of p(x | z_0), the SNR weight of the
//             middle term and the number of atoms under the noise mask.  The host forms the batch means of the reference.
//
// Noise: an explicit unmasked bank (noise_x [B,N,3], noise_h [B,N,nf]), or drawn in the kernels (both pointers NULL) by the
// Philox4x32-10 stream of pack_layout.h, key = noise_seed, counter = (mol_offset + b, atom, draw word, component / 4):
//   eps of component c (0..2: x, 3..3+nf-1: h) of atom i:  philox_normal(seed, mol_offset + b, i, 0x80000000, c)
//   t_int:  r = philox4x32_10(counter (mol_offset + b, 0, 0x80000001, 0), key (seed lo, seed hi)); t_int = mulhi(r[0], T + 1)
// The draw words have the top bit set: the sampling chains draw words 0 .. 2T + 2 (dl_philox_fill refuses a negative
// int32 draw), so no counter of the loss coincides with one of a chain of the same seed.  The epilogue regenerates eps
// instead of reading a stored copy; both kernels reduce the centre of gravity with the same code and the same workgroup
// size, so they agree bit for bit.
//
// Reductions: a thread owns atoms tid, tid + 256, ...; its partial sums go through a 64-lane xor butterfly (lane 0's value
// is taken), the four waves' values are added in a fixed order through LDS.  No atomics: a batch gives the same bits every
// run, and a molecule the same bits in any batch.  No NaN guards: a NaN input gives a NaN term, as in the reference.
#include "pack_layout.h"

namespace {

constexpr int LT = 256;                        // threads per molecule, both kernels (the same partition: the same eps bits)
constexpr unsigned DRAW_EPS = 0x80000000u;
constexpr unsigned DRAW_T = 0x80000001u;

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the workgroup of K values per thread; every thread gets the same bits
template <int K>
__device__ __forceinline__ void block_sum(float (&v)[K], float* lds /* [LT / 64][K] */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum64(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (lds[k] + lds[K + k]) + (lds[2 * K + k] + lds[3 * K + k]);
    __syncthreads();
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ int gamma_index(float t, int timesteps) {        // PredefinedNoiseSchedule.forward (noise.py:127-128)
    int k = int(rintf(t * float(timesteps)));
    if (k < 0) k += timesteps + 1;
    return min(max(k, 0), timesteps);
}

__device__ __forceinline__ float noise_mask(const dl_loss_args& a, size_t bi) {
    return a.inpainting ? a.node_mask[bi] : a.linker_mask[bi];
}

// unmasked standard normal of component c of atom i of molecule b
__device__ __forceinline__ float eps_raw(const dl_loss_args& a, int b, int i, int c) {
    const size_t bi = size_t(b) * a.N + i;
    if (a.noise_x != nullptr) return c < 3 ? a.noise_x[bi * 3 + c] : a.noise_h[bi * a.nf + (c - 3)];
    return philox_normal(a.noise_seed, unsigned(a.mol_offset + b), unsigned(i), DRAW_EPS, unsigned(c));
}

// inpainting: mean of the masked x-noise over the noise mask (utils.py:56-63, 158-168); zeros otherwise
__device__ void eps_mean(const dl_loss_args& a, int b, float* lds, float (&mean)[3]) {
    mean[0] = mean[1] = mean[2] = 0.0f;
    if (!a.inpainting) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = threadIdx.x; i < a.N; i += LT) {
        const float m = noise_mask(a, size_t(b) * a.N + i);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += eps_raw(a, b, i, c) * m;
        v[3] += m;
    }
    block_sum<4>(v, lds);
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = v[c] / v[3];
}

__device__ __forceinline__ float eps_of(const dl_loss_args& a, int b, int i, int c, float m, const float (&mean)[3]) {
    const float e = eps_raw(a, b, i, c) * m;
    return (a.inpainting && c < 3) ? e - mean[c] * m : e;
}

__global__ void __launch_bounds__(LT) loss_prologue_kernel(dl_loss_args a) {
#pragma clang fp contract(off)                  // the reference's elementwise ops, one rounding each
    __shared__ float lds[4 * 4];
    __shared__ float s_coef[2];
    const int b = blockIdx.x;
    const int D = 3 + a.nf;
    if (threadIdx.x == 0) {
        int ti;
        if (a.t_given) {
            ti = a.t_int[b];
        } else {
            unsigned r[4];
            philox4x32_10(unsigned(a.mol_offset + b), 0u, DRAW_T, 0u, unsigned(a.noise_seed), unsigned(a.noise_seed >> 32), r);
            ti = int(__umulhi(r[0], unsigned(a.T + 1)));
            a.t_int[b] = ti;
        }
        const float t = float(ti) / float(a.T), s = float(ti - 1) / float(a.T);
        const float gt = a.gamma_table[gamma_index(t, a.timesteps)], gs = a.gamma_table[gamma_index(s, a.timesteps)];
        a.t[b] = t;
        a.gamma[2 * b] = gt;
        a.gamma[2 * b + 1] = gs;
        s_coef[0] = sqrtf(sigmoidf_(-gt));       // alpha_t
        s_coef[1] = sqrtf(sigmoidf_(gt));        // sigma_t
    }
    __syncthreads();
    const float alpha_t = s_coef[0], sigma_t = s_coef[1];
    float mean[3];
    eps_mean(a, b, lds, mean);
    for (int i = threadIdx.x; i < a.N; i += LT) {
        const size_t bi = size_t(b) * a.N + i;
        const float m = noise_mask(a, bi);
        const float fm = a.inpainting ? 0.0f : a.fragment_mask[bi];
        for (int c = 0; c < D; ++c) {
            const float xv = a.xh[bi * D + c];
            const float z = alpha_t * xv + sigma_t * eps_of(a, b, i, c, m, mean);
            a.z_t[bi * D + c] = a.inpainting ? z : xv * fm + z * m;
        }
    }
}

__global__ void __launch_bounds__(LT) loss_epilogue_kernel(dl_loss_args a) {
#pragma clang fp contract(off)                  // the reference's elementwise ops, one rounding each: the KL prior is a sum of
                                                // terms log(1/sigma_T) + 0.5 (sigma_T^2 + mu^2) - 0.5 that cancel to ~1e-5 each
    __shared__ float lds[4 * 7];
    const int b = blockIdx.x;
    const int D = 3 + a.nf, nf = a.nf;
    const float gt = a.gamma[2 * b], gs = a.gamma[2 * b + 1];
    const float g0 = a.gamma_table[0];
    const float alpha_T = a.prior[3 * b], sigma_T = a.prior[3 * b + 1], log_inv_sigma_T = a.prior[3 * b + 2];
    const float s2_T = sigma_T * sigma_T;
    const float sigma0 = sqrtf(sigmoidf_(gt)) * a.norm_h;          // edm.py:298: sigma(gamma_t) rescaled to the integer scale
    const float sqrt2 = 1.41421356237309515f;                      // cdf_standard_gaussian: x / math.sqrt(2)
    float mean[3];
    eps_mean(a, b, lds, mean);
    // err, err_x, |eps_hat|^2, sum mu_T_x^2, kl of the h-part, log p(h | z_0), atoms under the mask
    float v[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = threadIdx.x; i < a.N; i += LT) {
        const size_t bi = size_t(b) * a.N + i;
        const float m = noise_mask(a, bi);
        const float lm = a.inpainting ? 1.0f : a.linker_mask[bi];
        for (int c = 0; c < D; ++c) {
            const float e = eps_of(a, b, i, c, m, mean);
            const float eh = a.eps_hat[bi * D + c] * lm;             // edm.py:86 (EDM only)
            const float d = e - eh;
            v[0] += d * d;
            if (c < 3) v[1] += d * d;
            v[2] += eh * eh;
            const float mu = alpha_T * a.xh[bi * D + c];
            if (c < 3) v[3] += mu * mu;
            else v[4] += log_inv_sigma_T + 0.5f * (s2_T + mu * mu) - 0.5f;
        }
        // categorical features (edm.py:300-321): integrals from -0.5 to 0.5 around the one-hot value, normalised over the
        // categories, the true category's log-probability selected by h * mask
        float lp[DMAX - 3];                      // (registers: every index below is a compile-time constant)
        float lmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < DMAX - 3; ++k) {
            if (k < nf) {
                const float cen = a.z_t[bi * D + 3 + k] * a.norm_h + a.bias_h - 1.0f;
                lp[k] = logf(0.5f * (1.0f + erff((cen + 0.5f) / sigma0 / sqrt2)) -
                             0.5f * (1.0f + erff((cen - 0.5f) / sigma0 / sqrt2)) + 1e-10f);
                lmax = fmaxf(lmax, lp[k]);
            }
        }
        float se = 0.0f;
#pragma unroll
        for (int k = 0; k < DMAX - 3; ++k)
            if (k < nf) se += expf(lp[k] - lmax);
        const float log_z = lmax + logf(se);     // torch.logsumexp
#pragma unroll
        for (int k = 0; k < DMAX - 3; ++k) {
            if (k < nf) {
                const float h = a.xh[bi * D + 3 + k] * a.norm_h + a.bias_h;
                v[5] += (lp[k] - log_z) * h * m;
            }
        }
        v[6] += m;
    }
    block_sum<7>(v, lds);
    if (threadIdx.x == 0) {
        const float d = a.inpainting ? (v[6] - 1.0f) * 3.0f : v[6] * 3.0f;        // dimensionality (edm.py:366-367, :729-730)
        const float kl_x = d * log_inv_sigma_T + 0.5f * (d * s2_T + v[3]) - 0.5f * d;
        float* row = a.rows + size_t(b) * DL_LOSS_ROW;
        row[0] = v[0];
        row[1] = sqrtf(v[2]);
        row[2] = kl_x + v[4];
        row[3] = -0.5f * v[1];
        row[4] = v[5];
        row[5] = d * (-(0.5f * g0) - 0.91893853320467274f);                          // 0.5 log(2 pi)
        row[6] = expf(-(gs - gt)) - 1.0f;
        row[7] = v[6];
    }
}

// d eps_hat of the loss terms (include/difflinker_hip.h, dl_edm_loss_grad): weights[b] = (w_err, w_noise, w_logpx)
__global__ void __launch_bounds__(LT) loss_grad_kernel(dl_loss_args a, const float* __restrict__ weights, float* __restrict__ g) {
    __shared__ float lds[4 * 4];
    const int b = blockIdx.x;
    const int D = 3 + a.nf;
    const float w_err = weights[3 * b], w_noise = weights[3 * b + 1], w_logpx = weights[3 * b + 2];
    const float norm = a.rows[size_t(b) * DL_LOSS_ROW + 1];
    float mean[3];
    eps_mean(a, b, lds, mean);
    for (int i = threadIdx.x; i < a.N; i += LT) {
        const size_t bi = size_t(b) * a.N + i;
        const float m = noise_mask(a, bi);
        const float lm = a.inpainting ? 1.0f : a.linker_mask[bi];
        for (int c = 0; c < D; ++c) {
            const float eh = a.eps_hat[bi * D + c] * lm;
            const float d = eps_of(a, b, i, c, m, mean) - eh;
            float v = -2.0f * d * w_err;
            if (w_noise != 0.0f) v += eh * (w_noise / norm);
            if (c < 3) v += d * w_logpx;
            g[bi * D + c] = v * lm;
        }
    }
}

int32_t check_loss_args(const dl_loss_args* a, bool epilogue) {
    if (!a || a->B < 0 || a->N < 1 || a->nf < 1 || 3 + a->nf > DMAX || a->T < 1 || a->timesteps < 1 || a->mol_offset < 0)
        return DL_ERR_BAD_ARG;
    if (!a->xh || !a->node_mask || !a->gamma_table || !a->t_int || !a->gamma || !a->z_t) return DL_ERR_BAD_ARG;
    if (!a->inpainting && (!a->fragment_mask || !a->linker_mask)) return DL_ERR_BAD_ARG;
    if ((a->noise_x == nullptr) != (a->noise_h == nullptr)) return DL_ERR_BAD_ARG;
    if (epilogue ? (!a->eps_hat || !a->rows || !a->prior) : !a->t) return DL_ERR_BAD_ARG;
    return DL_OK;
}

}  // namespace

extern "C" {

int32_t dl_edm_loss_prologue(const dl_loss_args* args, void* stream) {
    const int32_t st = check_loss_args(args, false);
    if (st != DL_OK) return st;
    if (args->B == 0) return DL_OK;
    hipLaunchKernelGGL(loss_prologue_kernel, dim3(args->B), dim3(LT), 0, static_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_edm_loss_epilogue(const dl_loss_args* args, void* stream) {
    const int32_t st = check_loss_args(args, true);
    if (st != DL_OK) return st;
    if (args->B == 0) return DL_OK;
    hipLaunchKernelGGL(loss_epilogue_kernel, dim3(args->B), dim3(LT), 0, static_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_edm_loss_grad(const dl_loss_args* args, const float* weights, float* d_eps_hat, void* stream) {
    const int32_t st = check_loss_args(args, true);
    if (st != DL_OK) return st;
    if (!weights || !d_eps_hat) return DL_ERR_BAD_ARG;
    if (args->B == 0) return DL_OK;
    hipLaunchKernelGGL(loss_grad_kernel, dim3(args->B), dim3(LT), 0, static_cast<hipStream_t>(stream), *args, weights, d_eps_hat);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
