// egnn_backward.hip — gradient of the fully-connected EGNN denoiser (reference Dynamics.forward, src/egnn.py:374-447) with
// respect to every parameter, for training (reference EDM.forward + loss.backward()).
//
// Scope: egnn_dynamics, hidden_nf = 128, SiLU, sum aggregation, no attention / tanh / sin_embedding (the released FC
// configurations); any n_layers, inv_sublayers 1..4, norm_constant, normalization_factor, context width, condition_time.
// Parameters come as ONE flat fp32 buffer in Dynamics.parameters() order (egnn.py: egnn_tensor_order) and the gradient
// leaves in the same layout.  fp32 arithmetic (plain FMA chains, no f16 split modes); the long sums are split or run in fp64 (SUMC).
//
// Two launches:
//   backward_mol_kernel   one 256-thread workgroup per molecule.  (1) a forward-with-save pass in fp32 writes the node state
//                         h of every sublayer, the aggregate of every GCL and x of every block to the molecule's workspace;
//                         (2) the blocks are walked in reverse.  Pair-level quantities (edge-MLP activations, r_ij, coord_diff)
//                         are never stored: every pass recomputes them tile by tile (one receiver i, 32 senders j) from the
//                         saved node state, so nothing of size N^2 x 128 exists.  Each molecule writes its full parameter
//                         gradient (every entry exactly once) to its own slice of the workspace.
//   reduce_kernel         grad[p] = sum over molecules b = 0 .. B-1 in that order.  No atomics anywhere: the same inputs give
//                         the same bits on every run.
//
// Per pair (i, j), per MLP: pre1 = W_a h_i + W_b h_j + w_r r_ij + w_d d0_ij + b1, m1 = silu(pre1), pre2 = W2 m1 + b2,
// m2 = silu(pre2).  The W_a h_i + b1 and W_b h_j parts are node-level products done once per pass; the 128x128 W2 product
// runs per pair from LDS.  Backward per tile: dpre2 -> dW2 (register accumulators), dm1 = W2^T dpre2 -> dpre1, whose row
// sums S_i and column sums T_j give dW_a = sum_i S_i h_i^T, dW_b = sum_j T_j h_j^T, db1 = sum_i S_i and the node gradient
// W_a^T S_i + W_b^T T_i; dpre1 . w_r gives dr_ij, which flows into x through r_ij = |x_i - x_j|^2 (later blocks see
// coordinates that earlier blocks' weights moved).  The edge mask multiplies as collate builds it (int8 0 / -1 / -2).
#include "backward_layout.h"

namespace {

constexpr int BT = 256;                        // threads per molecule
constexpr int WLD = H + 1;                     // LDS row stride of a staged 128x128 weight block (odd: conflict-free both ways)
constexpr int TP = 32;                         // pairs per tile (one receiver, 32 senders)
constexpr int BWD_MAX_ATOMS = 1024;
// No sum over the atoms or the pairs of a molecule is one chain of N or N^2 fp32 additions: the rounding error of such a chain
// grows with its length (the GCL's edge_mlp gradients were 4e-6 off the fp64 gradient at N = 257, eight times fp32 eager
// autograd's error).  Where a thread owns one number (a bias entry, S_i) it adds in fp64; where it owns 64 (a slice of a weight
// gradient) it adds partial sums - a receiver's row in the pair passes, SUMC node rows in outer_w - and then the partials.
// A padded row or pair adds an exact zero at every level, so padding changes no bit.
constexpr int SUMC = 16;

// per-molecule workspace (floats), each region rounded up to 16 floats
struct Ws {
    long hs, ag, xs, hin, a, bm, u, hn, du, dh, dh2, dagg, si, tj, dx, dxi, dxj, gpart, total;
};

__host__ __device__ inline long rnd16(long v) { return (v + 15) & ~15L; }

__host__ __device__ inline Ws ws_layout(int N, int L, int S, long P) {
    Ws w;
    long o = 0;
    const long nh = rnd16(long(N) * H), n4 = rnd16(long(N) * 4);
    w.hs = o;   o += nh * (long(L) * (S + 1) + 1);   // h_{k,s}, s = 0..S, then the final h
    w.ag = o;   o += nh * long(L) * S;               // aggregate (sum / normalization_factor) of every GCL
    w.xs = o;   o += n4 * (L + 1);                   // x of every block (x, y, z, pad)
    w.hin = o;  o += rnd16(long(N) * MAX_FIN);
    w.a = o;    o += nh;
    w.bm = o;   o += nh;
    w.u = o;    o += nh;
    w.hn = o;   o += nh;
    w.du = o;   o += nh;
    w.dh = o;   o += nh;
    w.dh2 = o;  o += nh;
    w.dagg = o; o += nh;
    w.si = o;   o += nh;
    w.tj = o;   o += nh;
    w.dx = o;   o += n4;
    w.dxi = o;  o += n4;
    w.dxj = o;  o += n4;
    w.gpart = o; o += rnd16(P);
    w.total = o;
    return w;
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float dsilu(float v) {             // d silu / dv
    const float s = 1.0f / (1.0f + expf(-v));
    return s * (1.0f + v * (1.0f - s));
}

struct Lds {
    float w[H * WLD];                          // staged 128x128 weight block
    float pre1[TP * H];                        // pre1, then dpre1
    float m1[TP * H];
    float t3[TP * H];                          // m2 (coordinate MLP) / dpre2
    float r[TP], d0[TP], e[TP], s[TP], ds[TP], dr[TP];
    float diff[TP * 3], cd[TP * 3], ddiff[TP * 3];
    float wr[H];
    float red[BT];
};

// Ws[o][k] = W[o * ld + col0 + k], o, k < 128
__device__ void stage(Lds& L, const float* W, long ld, long col0) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < H * H; idx += BT) {
        const int o = idx >> 7, k = idx & (H - 1);
        L.w[o * WLD + k] = W[o * ld + col0 + k];
    }
    __syncthreads();
}

// out[n][c] = (acc ? out[n][c] : 0) + bias[c] + sum_k W(c, k) in[n][k], W = staged block (trans: W(c, k) = Ws[k][c])
template <bool TRANS>
__device__ void node_mv(const Lds& L, float* out, const float* in, int N, const float* bias, bool acc, float scale = 1.0f) {
    const int c = threadIdx.x & (H - 1);
    for (int n = threadIdx.x >> 7; n < N; n += 2) {
        const float* x = in + long(n) * H;
        float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};              // four interleaved chains of 32, not one of 128
#pragma unroll 2
        for (int k = 0; k < H; k += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) s4[u] += (TRANS ? L.w[(k + u) * WLD + c] : L.w[c * WLD + k + u]) * x[k + u];
        float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        s *= scale;
        if (bias) s += bias[c];
        out[long(n) * H + c] = acc ? out[long(n) * H + c] + s : s;
    }
    __syncthreads();
}

// gW[o * ld + col0 + k] = sum_n G[n][o] In[n][k]  (o, k < 128; every entry written once)
__device__ void outer_w(float* gW, long ld, long col0, const float* G, const float* In, int N) {
    const int o = threadIdx.x >> 1, k0 = (threadIdx.x & 1) * 64;
    float acc[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) acc[k] = 0.0f;
    for (int n0 = 0; n0 < N; n0 += SUMC) {                     // partial sums of SUMC rows, then the sum of the partials
        float part[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) part[k] = 0.0f;
        const int n1 = n0 + SUMC < N ? n0 + SUMC : N;
        for (int n = n0; n < n1; ++n) {
            const float g = G[long(n) * H + o];
            const float* x = In + long(n) * H + k0;
#pragma unroll
            for (int k = 0; k < 64; ++k) part[k] += g * x[k];
        }
#pragma unroll
        for (int k = 0; k < 64; ++k) acc[k] += part[k];
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) gW[o * ld + col0 + k0 + k] = acc[k];
}

// gb[c] = sum_n G[n][c]
__device__ void col_sum(float* gb, const float* G, int N) {
    if (threadIdx.x < H) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += G[long(n) * H + threadIdx.x];
        gb[threadIdx.x] = float(s);
    }
}

struct Mol {
    int N, nf, fin, L, S, ctx, cond_t, centering;
    float nc, inv_norm;
    const float* nm;        // [N]
    const float* lm;        // [N] or null
    const int8_t* em;       // [N][N]
};

enum PassMode { GCL_FWD, COORD_FWD, GCL_BWD, COORD_BWD };

// One pass over the pairs of a molecule through one edge MLP (edge_mlp of a GCL or coord_mlp of the update).
//   P: that MLP's parameters (W1 [H, 2H+2], b1, W2 [H, H], b2, [w3 [H]]);  h: node state [N][H];  x: the block's x [N][4];
//   x0: input x [N][4] (d0);  GCL_FWD: out = aggregate [N][H] (sum / norm);  COORD_FWD: out = new x [N][4];
//   GCL_BWD: up = d aggregate [N][H], gP = gradient of P, dh += node gradient, dxi/dxj += gradient of x;
//   COORD_BWD: up = d x_new [N][4] (already masked).
template <PassMode MODE>
__device__ void pair_pass(Lds& L, const Mol& m, const float* P, const float* h, const float* x, const float* x0, float* out,
                          const float* up, float* gP, float* dh, float* wa, float* wb, float* si, float* tj, float* dxi,
                          float* dxj) {
    constexpr bool BWD = MODE == GCL_BWD || MODE == COORD_BWD;
    constexpr bool COORD = MODE == COORD_FWD || MODE == COORD_BWD;
    const int N = m.N, tid = threadIdx.x;
    const long ld1 = 2 * H + 2;
    const float* W1 = P;
    const float* b1 = P + long(H) * ld1;
    const float* W2 = b1 + H;
    const float* b2 = W2 + long(H) * H;
    const float* w3 = b2 + H;
    // node-level parts of the first layer
    stage(L, W1, ld1, 0);
    node_mv<false>(L, wa, h, N, b1, false);
    stage(L, W1, ld1, H);
    node_mv<false>(L, wb, h, N, nullptr, false);
    if (tid < H) L.wr[tid] = W1[tid * ld1 + 2 * H];
    stage(L, W2, H, 0);
    const int c = tid & (H - 1), ph = tid >> 7;                 // channel, pair half
    const float w_r = W1[c * ld1 + 2 * H], w_d = W1[c * ld1 + 2 * H + 1], b2c = b2[c];
    const float w3c = COORD ? w3[c] : 0.0f;
    // accumulators kept across the whole pass
    float gw2[64];                                               // dW2[o = tid >> 1][k0 + 0..63]
#pragma unroll
    for (int k = 0; k < 64; ++k) gw2[k] = 0.0f;
    double gb2 = 0.0, gwr = 0.0, gwd = 0.0, gb1 = 0.0, gw3 = 0.0;   // one number per thread each: summed in fp64
    if (BWD && tid < H)
        for (int j = 0; j < N; ++j) tj[long(j) * H + tid] = 0.0f;
    __syncthreads();
    for (int i = 0; i < N; ++i) {
        float row_acc = 0.0f;                                     // GCL_FWD: aggregate channel c (half ph); COORD: x sum / dx_i
        double row_si = 0.0;                                      // BWD: S_i[c]
        float rw2[64];                                            // BWD: the row's part of gw2
#pragma unroll
        for (int k = 0; k < 64; ++k) rw2[k] = 0.0f;
        float upc[3] = {0.0f, 0.0f, 0.0f};
        if (MODE == COORD_BWD) {
            const float lmi = m.lm ? m.lm[i] : 1.0f;
            for (int q = 0; q < 3; ++q) upc[q] = up[long(i) * 4 + q] * lmi * m.inv_norm;
        }
        const float gi = MODE == GCL_BWD ? up[long(i) * H + c] * m.inv_norm : 0.0f;
        for (int j0 = 0; j0 < N; j0 += TP) {
            // geometry of the tile
            if (tid < TP) {
                const int j = j0 + tid;
                float e = 0.0f, r = 0.0f, d0 = 0.0f, df[3] = {0.0f, 0.0f, 0.0f}, cd[3] = {0.0f, 0.0f, 0.0f};
                if (j < N) {
                    e = float(m.em[long(i) * N + j]);
                    float dd[3];
                    for (int q = 0; q < 3; ++q) {
                        df[q] = x[long(i) * 4 + q] - x[long(j) * 4 + q];
                        dd[q] = x0[long(i) * 4 + q] - x0[long(j) * 4 + q];
                    }
                    r = df[0] * df[0] + df[1] * df[1] + df[2] * df[2];
                    d0 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
                    const float den = sqrtf(r + 1e-8f) + m.nc;
                    for (int q = 0; q < 3; ++q) cd[q] = df[q] / den;
                }
                L.e[tid] = e; L.r[tid] = r; L.d0[tid] = d0;
                for (int q = 0; q < 3; ++q) { L.diff[tid * 3 + q] = df[q]; L.cd[tid * 3 + q] = cd[q]; L.ddiff[tid * 3 + q] = 0.0f; }
            }
            __syncthreads();
            // first layer
            const float ai = wa[long(i) * H + c];
            for (int p = ph; p < TP; p += 2) {
                const int j = j0 + p;
                const float bj = j < N ? wb[long(j) * H + c] : 0.0f;
                const float v = ai + bj + w_r * L.r[p] + w_d * L.d0[p];
                L.pre1[p * H + c] = v;
                L.m1[p * H + c] = silu(v);
            }
            __syncthreads();
            // second layer: channel c, pairs ph * 16 .. ph * 16 + 15
            float pre2[TP / 2];
#pragma unroll
            for (int q = 0; q < TP / 2; ++q) pre2[q] = b2c;
            for (int k = 0; k < H; k += 4) {
                const float w0 = L.w[c * WLD + k], w1 = L.w[c * WLD + k + 1], w2 = L.w[c * WLD + k + 2], w3_ = L.w[c * WLD + k + 3];
#pragma unroll
                for (int q = 0; q < TP / 2; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(&L.m1[(ph * (TP / 2) + q) * H + k]);
                    pre2[q] += w0 * v.x + w1 * v.y + w2 * v.z + w3_ * v.w;
                }
            }
            if (MODE == GCL_FWD) {
#pragma unroll
                for (int q = 0; q < TP / 2; ++q) row_acc += silu(pre2[q]) * L.e[ph * (TP / 2) + q];
            } else if (MODE == GCL_BWD) {
#pragma unroll
                for (int q = 0; q < TP / 2; ++q) {
                    const int p = ph * (TP / 2) + q;
                    L.t3[p * H + c] = gi * L.e[p] * dsilu(pre2[q]);
                }
            } else {                                                // coordinate MLP: s = w3 . m2 per pair
#pragma unroll
                for (int q = 0; q < TP / 2; ++q) L.t3[(ph * (TP / 2) + q) * H + c] = silu(pre2[q]);
                __syncthreads();
                {
                    const int p = tid >> 3, part = tid & 7;          // 8 threads per pair, 16 channels each
                    float s = 0.0f;
                    for (int k = part * 16; k < part * 16 + 16; ++k) s += w3[k] * L.t3[p * H + k];
                    s += __shfl_xor(s, 1, 64);
                    s += __shfl_xor(s, 2, 64);
                    s += __shfl_xor(s, 4, 64);
                    if (part == 0) {
                        L.s[p] = s;
                        if (MODE == COORD_BWD) {
                            const float e = L.e[p];
                            float dsv = 0.0f, dcd[3], dot = 0.0f;
                            for (int q = 0; q < 3; ++q) {
                                dsv += upc[q] * L.cd[p * 3 + q];
                                dcd[q] = upc[q] * s * e;
                            }
                            L.ds[p] = dsv * e;
                            // cd = diff / (sqrt(r + 1e-8) + nc): d diff = dcd / den - diff (dcd . diff) / (den^2 sqrt(r + 1e-8))
                            const float nr = sqrtf(L.r[p] + 1e-8f), den = nr + m.nc;
                            for (int q = 0; q < 3; ++q) dot += dcd[q] * L.diff[p * 3 + q];
                            for (int q = 0; q < 3; ++q)
                                L.ddiff[p * 3 + q] = dcd[q] / den - L.diff[p * 3 + q] * dot / (den * den * nr);
                        }
                    }
                }
                __syncthreads();
                if (MODE == COORD_FWD) {
                    if (tid < 3)                                      // sum over j in order
                        for (int p = 0; p < TP; ++p) row_acc += L.cd[p * 3 + tid] * L.s[p] * L.e[p];
                } else {
#pragma unroll
                    for (int q = 0; q < TP / 2; ++q) {
                        const int p = ph * (TP / 2) + q;
                        const float m2 = L.t3[p * H + c];
                        gw3 += L.ds[p] * m2;
                        pre2[q] = L.ds[p] * w3c * dsilu(pre2[q]);    // dpre2 (kept in registers until t3 is free)
                    }
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < TP / 2; ++q) L.t3[(ph * (TP / 2) + q) * H + c] = pre2[q];
                }
            }
            if (BWD) {
                __syncthreads();
                // dW2 += dpre2^T m1, db2
                {
                    const int o = tid >> 1, k0 = (tid & 1) * 64;
                    for (int p = 0; p < TP; ++p) {
                        const float g = L.t3[p * H + o];
#pragma unroll
                        for (int k = 0; k < 64; k += 4) {
                            const float4 v = *reinterpret_cast<const float4*>(&L.m1[p * H + k0 + k]);
                            rw2[k] += g * v.x; rw2[k + 1] += g * v.y; rw2[k + 2] += g * v.z; rw2[k + 3] += g * v.w;
                        }
                        if ((tid & 1) == 0) gb2 += g;
                    }
                }
                // dm1 = W2^T dpre2, dpre1 = dm1 silu'(pre1)  (channel c = k of the first layer)
                for (int q = 0; q < TP / 2; ++q) {
                    const int p = ph * (TP / 2) + q;
                    float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
                    for (int o = 0; o < H; o += 4)
#pragma unroll
                        for (int u = 0; u < 4; ++u) s4[u] += L.w[(o + u) * WLD + c] * L.t3[p * H + o + u];
                    L.pre1[p * H + c] = ((s4[0] + s4[1]) + (s4[2] + s4[3])) * dsilu(L.pre1[p * H + c]);
                }
                __syncthreads();
                if (tid < H) {
                    for (int p = 0; p < TP; ++p) {
                        const int j = j0 + p;
                        if (j >= N) break;
                        const float g = L.pre1[p * H + tid];
                        row_si += g;
                        gwr += g * L.r[p];
                        gwd += g * L.d0[p];
                        tj[long(j) * H + tid] += g;
                    }
                } else {                                                // dr = dpre1 . w_r, 4 threads per pair
                    const int u = tid - H, p = u >> 2, part = u & 3;
                    float s = 0.0f;
                    for (int k = part * 32; k < part * 32 + 32; ++k) s += L.pre1[p * H + k] * L.wr[k];
                    s += __shfl_xor(s, 1, 64);
                    s += __shfl_xor(s, 2, 64);
                    if (part == 0) L.dr[p] = s;
                }
                __syncthreads();
                if (tid < TP * 3) {                                     // x gradient of the tile's senders
                    const int p = tid / 3, q = tid % 3, j = j0 + p;
                    // x_i - x_i is zero whatever x is: the self pair (live in collate's mask, with 1 / den = 1e4 at
                    // norm_constant <= 1e-6) has no x gradient; added to dxi and taken off dxj it would cost them four digits
                    const float g = j == i ? 0.0f : L.ddiff[p * 3 + q] + 2.0f * L.diff[p * 3 + q] * L.dr[p];
                    L.ddiff[p * 3 + q] = g;
                    if (j < N) dxj[long(j) * 4 + q] -= g;
                }
                __syncthreads();
                if (tid < 3)
                    for (int p = 0; p < TP; ++p) row_acc += L.ddiff[p * 3 + tid];
            }
            __syncthreads();
        }
        // end of the receiver row
        if (MODE == GCL_FWD) {
            L.red[tid] = row_acc;
            __syncthreads();
            if (tid < H) out[long(i) * H + tid] = (L.red[tid] + L.red[tid + H]) * m.inv_norm;
            __syncthreads();
        } else if (MODE == COORD_FWD) {
            if (tid < 3) {
                const float lmi = m.lm ? m.lm[i] : 1.0f;
                out[long(i) * 4 + tid] = (x[long(i) * 4 + tid] + row_acc * m.inv_norm * lmi) * m.nm[i];
            }
        } else {
            if (tid < H) { si[long(i) * H + tid] = float(row_si); gb1 += row_si; }
            if (tid < 3) dxi[long(i) * 4 + tid] += row_acc;
#pragma unroll
            for (int k = 0; k < 64; ++k) gw2[k] += rw2[k];
        }
    }
    __syncthreads();
    if (!BWD) return;
    // parameter gradients of the pass
    float* gW1 = gP;
    float* gb1p = gP + long(H) * ld1;
    float* gW2 = gb1p + H;
    float* gb2p = gW2 + long(H) * H;
    {
        const int o = tid >> 1, k0 = (tid & 1) * 64;
#pragma unroll
        for (int k = 0; k < 64; ++k) gW2[o * H + k0 + k] = gw2[k];
        if ((tid & 1) == 0) gb2p[o] = float(gb2);
    }
    if (tid < H) {
        gW1[tid * ld1 + 2 * H] = float(gwr);
        gW1[tid * ld1 + 2 * H + 1] = float(gwd);
        gb1p[tid] = float(gb1);
    }
    if (COORD) {                                                       // combine the two pair halves of dw3
        L.red[tid] = float(gw3);
        __syncthreads();
        if (tid < H) gP[C_4W + tid] = L.red[tid] + L.red[tid + H];
    }
    __syncthreads();
    outer_w(gW1, ld1, 0, si, h, N);
    outer_w(gW1, ld1, H, tj, h, N);
    // node gradient: dh += W_a^T S + W_b^T T
    stage(L, W1, ld1, 0);
    node_mv<true>(L, dh, si, N, nullptr, true);
    stage(L, W1, ld1, H);
    node_mv<true>(L, dh, tj, N, nullptr, true);
}

struct Args {
    int B, N, nf, ctx, cond_t, L, S, centering, t_scalar;
    float nc, norm;
    const float* params;
    const float* xh; const float* t; const float* nm; const float* lm; const int8_t* em; const float* context;
    const float* grad_out;
    float* ws;
    long ws_stride, P;
};

__global__ void __launch_bounds__(BT) backward_mol_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, D = 3 + nf;
    Mol m;
    m.N = N; m.nf = nf; m.fin = nf + a.cond_t + a.ctx; m.L = a.L; m.S = a.S; m.ctx = a.ctx; m.cond_t = a.cond_t;
    m.centering = a.centering; m.nc = a.nc; m.inv_norm = 1.0f / a.norm;
    m.nm = a.nm + long(b) * N;
    m.lm = a.lm ? a.lm + long(b) * N : nullptr;
    m.em = a.em + long(b) * N * N;
    const int fin = m.fin;
    const Ws w = ws_layout(N, a.L, a.S, a.P);
    float* ws = a.ws + long(b) * a.ws_stride;
    const long nh = rnd16(long(N) * H), n4 = rnd16(long(N) * 4);
    auto HS = [&](int k, int s) { return ws + w.hs + nh * (long(k) * (a.S + 1) + s); };
    auto AG = [&](int k, int s) { return ws + w.ag + nh * (long(k) * a.S + s); };
    auto XS = [&](int k) { return ws + w.xs + n4 * k; };
    float *hin = ws + w.hin, *A = ws + w.a, *Bm = ws + w.bm, *U = ws + w.u, *HN = ws + w.hn, *DU = ws + w.du,
          *DH = ws + w.dh, *DH2 = ws + w.dh2, *DAGG = ws + w.dagg, *SI = ws + w.si, *TJ = ws + w.tj, *DX = ws + w.dx,
          *DXI = ws + w.dxi, *DXJ = ws + w.dxj, *G = ws + w.gpart;
    const Offs off = param_offsets(fin, a.S);
    const float* P = a.params;
    const float* xh = a.xh + long(b) * N * D;

    // ---- inputs (egnn.py:385-407): x, h masked, time and context appended
    for (int n = tid; n < N; n += BT) {
        const float nmv = m.nm[n];
        for (int q = 0; q < 3; ++q) XS(0)[n * 4 + q] = xh[long(n) * D + q] * nmv;
        XS(0)[n * 4 + 3] = 0.0f;
        for (int k = 0; k < nf; ++k) hin[long(n) * MAX_FIN + k] = xh[long(n) * D + 3 + k] * nmv;
        if (a.cond_t) hin[long(n) * MAX_FIN + nf] = a.t_scalar ? a.t[0] : a.t[b];
        for (int k = 0; k < a.ctx; ++k) hin[long(n) * MAX_FIN + nf + a.cond_t + k] = a.context[(long(b) * N + n) * a.ctx + k];
    }
    __syncthreads();
    // ---- forward with save (fp32)
    {
        const int c = tid & (H - 1);
        for (int n = tid >> 7; n < N; n += 2) {
            float s = P[off.emb_b + c];
            for (int k = 0; k < fin; ++k) s += P[off.emb_w + long(c) * fin + k] * hin[long(n) * MAX_FIN + k];
            HS(0, 0)[long(n) * H + c] = s;
        }
        __syncthreads();
    }
    for (int k = 0; k < a.L; ++k) {
        const float* blk = P + off.blk0 + off.blk_stride * k;
        for (int s = 0; s < a.S; ++s) {
            const float* g = blk + off.gcl_stride * s;
            const float* h = HS(k, s);
            pair_pass<GCL_FWD>(L, m, g + G_E0W, h, XS(k), XS(0), AG(k, s), nullptr, nullptr, nullptr, A, Bm, nullptr,
                               nullptr, nullptr, nullptr);
            stage(L, g + G_N0W, 2 * H, 0);
            node_mv<false>(L, U, h, N, g + G_N0B, false);
            stage(L, g + G_N0W, 2 * H, H);
            node_mv<false>(L, U, AG(k, s), N, nullptr, true);
            for (long idx = tid; idx < long(N) * H; idx += BT) HN[idx] = silu(U[idx]);
            stage(L, g + G_N2W, H, 0);
            float* hnext = HS(k, s + 1);
            node_mv<false>(L, hnext, HN, N, g + G_N2B, false);
            for (long idx = tid; idx < long(N) * H; idx += BT) hnext[idx] = (h[idx] + hnext[idx]) * m.nm[idx >> 7];
            __syncthreads();
        }
        pair_pass<COORD_FWD>(L, m, blk + off.equiv, HS(k, a.S), XS(k), XS(0), XS(k + 1), nullptr, nullptr, nullptr, A, Bm,
                             nullptr, nullptr, nullptr, nullptr);
        float* hn0 = k + 1 < a.L ? HS(k + 1, 0) : HS(a.L, 0);
        for (long idx = tid; idx < long(N) * H; idx += BT) hn0[idx] = HS(k, a.S)[idx] * m.nm[idx >> 7];
        __syncthreads();
    }
    const float* hL = HS(a.L, 0);

    // ---- output layer and velocity (egnn.py:420-447)
    const float* go = a.grad_out + long(b) * N * D;
    {
        float dmean[3] = {0.0f, 0.0f, 0.0f};
        if (a.centering) {                                    // vel_c = vel - nm sum(vel) / count (utils.py:56-63)
            if (tid == 0) {
                float s[3] = {0.0f, 0.0f, 0.0f}, cnt = 0.0f;
                for (int n = 0; n < N; ++n) {
                    for (int q = 0; q < 3; ++q) s[q] += m.nm[n] * go[long(n) * D + q];
                    cnt += m.nm[n];
                }
                for (int q = 0; q < 3; ++q) L.red[q] = s[q] / cnt;
            }
            __syncthreads();
            for (int q = 0; q < 3; ++q) dmean[q] = L.red[q];
            __syncthreads();
        }
        for (int n = tid; n < N; n += BT)
            for (int q = 0; q < 4; ++q) DX[n * 4 + q] = q < 3 ? (go[long(n) * D + q] - dmean[q]) * m.nm[n] : 0.0f;
        // dpre_out[n][c] = dh_final (zero for the time / context columns) * nm, kept in DU
        for (int idx = tid; idx < N * MAX_FIN; idx += BT) {
            const int n = idx / MAX_FIN, c = idx % MAX_FIN;
            DU[idx] = c < nf ? go[long(n) * D + 3 + c] * m.nm[n] : 0.0f;
        }
        __syncthreads();
        for (int idx = tid; idx < fin * H; idx += BT) {      // dW_out [fin, H]
            const int c = idx / H, kk = idx % H;
            float s = 0.0f;
            for (int n = 0; n < N; ++n) s += DU[n * MAX_FIN + c] * hL[long(n) * H + kk];
            G[off.out_w + idx] = s;
        }
        for (int c = tid; c < fin; c += BT) {
            float s = 0.0f;
            for (int n = 0; n < N; ++n) s += DU[n * MAX_FIN + c];
            G[off.out_b + c] = s;
        }
        const int c = tid & (H - 1);
        for (int n = tid >> 7; n < N; n += 2) {               // dh_L = W_out^T dpre_out
            float s = 0.0f;
            for (int q = 0; q < fin; ++q) s += P[off.out_w + long(q) * H + c] * DU[n * MAX_FIN + q];
            DH[long(n) * H + c] = s;
        }
        __syncthreads();
    }

    // ---- blocks in reverse
    for (int k = a.L - 1; k >= 0; --k) {
        const float* blk = P + off.blk0 + off.blk_stride * k;
        float* gblk = G + off.blk0 + off.blk_stride * k;
        // h_{k+1,0} = h_{k,S} nm;  x_{k+1} = (x_k + agg lm) nm
        for (long idx = tid; idx < long(N) * H; idx += BT) DH[idx] *= m.nm[idx >> 7];
        for (int idx = tid; idx < N * 4; idx += BT) {
            DX[idx] *= m.nm[idx >> 2];
            DXI[idx] = 0.0f;
            DXJ[idx] = 0.0f;
        }
        __syncthreads();
        pair_pass<COORD_BWD>(L, m, blk + off.equiv, HS(k, a.S), XS(k), XS(0), nullptr, DX, gblk + off.equiv, DH, A, Bm, SI,
                             TJ, DXI, DXJ);
        for (int s = a.S - 1; s >= 0; --s) {
            const float* g = blk + off.gcl_stride * s;
            float* gg = gblk + off.gcl_stride * s;
            const float* h = HS(k, s);
            const float* agg = AG(k, s);
            // node MLP recompute: U, HN
            stage(L, g + G_N0W, 2 * H, 0);
            node_mv<false>(L, U, h, N, g + G_N0B, false);
            stage(L, g + G_N0W, 2 * H, H);
            node_mv<false>(L, U, agg, N, nullptr, true);
            for (long idx = tid; idx < long(N) * H; idx += BT) {
                HN[idx] = silu(U[idx]);
                DH[idx] *= m.nm[idx >> 7];                    // h' = (h + node_mlp) nm
            }
            __syncthreads();
            col_sum(gg + G_N2B, DH, N);
            outer_w(gg + G_N2W, H, 0, DH, HN, N);
            stage(L, g + G_N2W, H, 0);
            node_mv<true>(L, DU, DH, N, nullptr, false);      // d HN
            for (long idx = tid; idx < long(N) * H; idx += BT) DU[idx] *= dsilu(U[idx]);
            __syncthreads();
            col_sum(gg + G_N0B, DU, N);
            outer_w(gg + G_N0W, 2 * H, 0, DU, h, N);
            outer_w(gg + G_N0W, 2 * H, H, DU, agg, N);
            for (long idx = tid; idx < long(N) * H; idx += BT) DH2[idx] = DH[idx];   // residual
            stage(L, g + G_N0W, 2 * H, 0);
            node_mv<true>(L, DH2, DU, N, nullptr, true);
            stage(L, g + G_N0W, 2 * H, H);
            node_mv<true>(L, DAGG, DU, N, nullptr, false);
            pair_pass<GCL_BWD>(L, m, g + G_E0W, h, XS(k), XS(0), nullptr, DAGG, gg + G_E0W, DH2, A, Bm, SI, TJ, DXI, DXJ);
            for (long idx = tid; idx < long(N) * H; idx += BT) DH[idx] = DH2[idx];
            __syncthreads();
        }
        for (int idx = tid; idx < N * 4; idx += BT) DX[idx] += DXI[idx] + DXJ[idx];
        __syncthreads();
    }
    // ---- embedding (no mask on its output, egnn.py:223)
    for (int idx = tid; idx < H * fin; idx += BT) {
        const int c = idx / fin, q = idx % fin;
        float s = 0.0f;
        for (int n = 0; n < N; ++n) s += DH[long(n) * H + c] * hin[long(n) * MAX_FIN + q];
        G[off.emb_w + idx] = s;
    }
    col_sum(G + off.emb_b, DH, N);
}

__global__ void __launch_bounds__(256) reduce_kernel(const float* __restrict__ ws, long stride, long goff, int B, long P,
                                                     float* __restrict__ grad) {
    const long p = long(blockIdx.x) * 256 + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += ws[long(b) * stride + goff + p];
    grad[p] = float(s);
}

bool scope_ok(const dl_backward_args* a) {
    return a->hidden_nf == H && a->n_layers >= 1 && a->inv_sublayers >= 1 && a->inv_sublayers <= 4 && a->in_node_nf >= 1 &&
           3 + a->in_node_nf <= DMAX && a->context_node_nf >= 0 && (a->condition_time == 0 || a->condition_time == 1) &&
           a->in_node_nf + a->condition_time + a->context_node_nf <= MAX_FIN && a->normalization_factor != 0.0f;
}

size_t ws_bytes(int B, int N, int L, int S, long P) {
    return size_t(B) * size_t(ws_layout(N, L, S, P).total) * sizeof(float);
}

}  // namespace

extern "C" {

int32_t dl_egnn_backward_max_atoms(void) { return BWD_MAX_ATOMS; }

int64_t dl_egnn_backward_fc_num_params(const dl_backward_args* a) {
    if (!a || !scope_ok(a)) return -1;
    return param_count(a->in_node_nf + a->condition_time + a->context_node_nf, a->n_layers, a->inv_sublayers);
}

size_t dl_egnn_backward_fc_workspace_bytes(const dl_backward_args* a) {
    if (!a || !scope_ok(a) || a->B < 0 || a->N < 1 || a->N > BWD_MAX_ATOMS) return 0;
    const long P = param_count(a->in_node_nf + a->condition_time + a->context_node_nf, a->n_layers, a->inv_sublayers);
    return ws_bytes(a->B, a->N, a->n_layers, a->inv_sublayers, P);
}

int32_t dl_egnn_backward_fc(const dl_backward_args* a, void* stream) {
    if (!a) return DL_ERR_BAD_ARG;
    if (!scope_ok(a)) return DL_ERR_UNSUPPORTED;
    if (a->B < 0 || a->N < 1 || a->N > BWD_MAX_ATOMS) return DL_ERR_BAD_ARG;
    const int fin = a->in_node_nf + a->condition_time + a->context_node_nf;
    const long P = param_count(fin, a->n_layers, a->inv_sublayers);
    if (a->n_params != P) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;
    if (!a->params || !a->xh || !a->node_mask || !a->edge_mask || !a->grad_out || !a->grad_params || !a->workspace)
        return DL_ERR_BAD_ARG;
    if (a->condition_time && !a->t) return DL_ERR_BAD_ARG;
    if (a->context_node_nf > 0 && !a->context) return DL_ERR_BAD_ARG;
    const size_t need = ws_bytes(a->B, a->N, a->n_layers, a->inv_sublayers, P);
    if (a->workspace_bytes < need) return DL_ERR_BAD_ARG;
    Args k;
    k.B = a->B; k.N = a->N; k.nf = a->in_node_nf; k.ctx = a->context_node_nf; k.cond_t = a->condition_time;
    k.L = a->n_layers; k.S = a->inv_sublayers; k.centering = a->centering; k.t_scalar = a->t_is_scalar;
    k.nc = a->norm_constant; k.norm = a->normalization_factor;
    k.params = a->params; k.xh = a->xh; k.t = a->t; k.nm = a->node_mask; k.lm = a->linker_mask; k.em = a->edge_mask;
    k.context = a->context; k.grad_out = a->grad_out; k.ws = static_cast<float*>(a->workspace);
    k.ws_stride = ws_layout(a->N, a->n_layers, a->inv_sublayers, P).total; k.P = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(backward_mol_kernel, dim3(a->B), dim3(BT), 0, s, k);
    if (hipGetLastError() != hipSuccess) return DL_ERR_HIP;
    const long goff = ws_layout(a->N, a->n_layers, a->inv_sublayers, P).gpart;
    hipLaunchKernelGGL(reduce_kernel, dim3(unsigned((P + 255) / 256)), dim3(256), 0, s, k.ws, k.ws_stride, goff, a->B, P,
                       a->grad_params);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
