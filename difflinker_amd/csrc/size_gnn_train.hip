// size_gnn_train.hip — training of the linker-size predictor: the forward of SizeGNN with BatchNorm in training mode, with
// the state it needs saved, and the gradient of every parameter (reference SizeClassifier.forward + loss.backward(),
// src/linker_size_lightning.py:83-117, src/linker_size.py:45-91, GCL src/egnn.py:9-80).
//
// Scope: hidden_nf = 128, ReLU, one edge attribute (the squared distance), normalization_factor 1, 'sum', normalization
// None or 'batch_norm' (eps 1e-5), any n_layers, at most NF_MAX fragment atoms per molecule.  Parameters and gradient are ONE
// flat fp32 buffer each in SizeGNN.parameters() order (raw weights, BatchNorm affine weight / bias included).  fp32.
//
// Rows.  A molecule's rows are its compacted fragment atoms (as in size_gnn.hip).  BatchNorm in training mode normalises over
// ALL B*N rows, and every row with fragment_mask = 0 holds the same value at every layer (h = embedding_in.bias before gcl1,
// h = 0 after any GCL, aggregate 0: none of its edges is kept).  Those rows are one GHOST row, processed as an extra
// molecule (block index B) with one row, no edge and node mask 0, and weighted by its multiplicity G = B*N - sum n_b in every
// batch reduction and in the final gradient sum.  Its upstream gradient from h is 0 (node mask) but not after a BatchNorm
// backward (d x depends on the batch sums), so it reaches node_mlp.0 and, in gcl1, embedding_in.bias.
//
// Launches.  Every per-molecule kernel runs one 256-thread workgroup per molecule (B + 1 of them).  A BatchNorm splits a
// layer at its batch reduction:
//   forward, per layer:  gcl_a (finish the previous layer, edge pass, node_mlp.0, BN1 partials) -> stats ->
//                        gcl_b (BN1, ReLU, node_mlp.<last>, BN2 partials) -> stats;  then logits (finish the last layer)
//   backward, per layer: bwd_b (BN2 partials of dy) -> bsum -> bwd_mid (BN2 backward, node_mlp.<last>, BN1 partials) -> bsum
//                        -> bwd_a (BN1 backward, node_mlp.0, edge pass backward, embedding_in for gcl1);  then reduce
// With normalization None the same kernels run with the BatchNorm steps skipped (gcl_a finishes the layer itself; no stats).
// Batch statistics: per molecule mean and centred sum of squares (two passes over its rows), merged over b = 0..B-1 and
// then the ghost row in that order (Chan's formula, fp64).  Gradient sums of the backward: per-molecule partials in the
// molecule's gradient slice, summed in the same fixed order.  No atomics: the gradient is bitwise repeatable.
//
// Pair work runs over the KEPT edges only (edge_mask != 0 and squared distance < 6, self loops included), listed once per
// molecule in (i, j) order by the first launch.  Pair and node products are 64 x 128 x 128 tiles: a thread owns 8 rows x 4
// channels (float4 reads of both operands, 12 reads per 128 FMAs), the weights come pre-transposed from the shared part of
// the workspace (L2-resident), the activations from LDS.  Weight gradients: a thread owns 4 x 16 outputs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/difflinker_hip.h"

namespace {

constexpr int H = 128;
constexpr int NF = 64;                    // fragment atoms per molecule (= dl_size_max_fragment_atoms)
constexpr int EMAX = NF * NF;             // kept edges per molecule, at most
constexpr int IN_MAX = 16;
constexpr int OUT_MAX = 64;
constexpr int BT = 256;
constexpr int T = 64;                     // pairs per tile
constexpr int MAT = H * H;
constexpr float BN_EPS = 1e-5f;

__host__ __device__ inline long rnd16(long v) { return (v + 15) & ~15L; }

// ---- raw parameter layout (SizeGNN.parameters() order)
struct POffs {
    long emb_w, emb_b, g0, gsize, out_w, out_b, total;
    // within a GCL
    long e0w, e0b, e2w, e2b, n0w, n0b, bn1w, bn1b, n3w, n3b, bn2w, bn2b;
};

__host__ __device__ inline POffs param_offsets(int in, int out, int L, int bn) {
    POffs o;
    o.emb_w = 0;
    o.emb_b = long(H) * in;
    o.g0 = o.emb_b + H;
    long q = 0;
    o.e0w = q; q += long(H) * (2 * H + 1);
    o.e0b = q; q += H;
    o.e2w = q; q += MAT;
    o.e2b = q; q += H;
    o.n0w = q; q += long(H) * 2 * H;
    o.n0b = q; q += H;
    o.bn1w = q; o.bn1b = q + H; if (bn) q += 2 * H;
    o.n3w = q; q += MAT;
    o.n3b = q; q += H;
    o.bn2w = q; o.bn2b = q + H; if (bn) q += 2 * H;
    o.gsize = q;
    o.out_w = o.g0 + q * L;
    o.out_b = o.out_w + long(out) * H;
    o.total = o.out_b + out;
    return o;
}

// ---- workspace.  Shared part: packed weights (12 [128][128] matrices per layer), per-BatchNorm statistics, the ghost count.
// Per-molecule part (B + 1 slices): the saved state and the molecule's gradient slice.
enum { PK_W1AT, PK_W1BT, PK_W1A, PK_W1B, PK_W2T, PK_W2, PK_W3AT, PK_W3BT, PK_W3A, PK_W3B, PK_W4T, PK_W4, PK_N };
// statistics of one BatchNorm: mean, biased var, 1/sqrt(var + eps), sum dy, sum dy*xhat   ([5][128] floats)
constexpr int ST_MEAN = 0, ST_VAR = H, ST_INV = 2 * H, ST_SDY = 3 * H, ST_SDX = 4 * H, ST_SIZE = 5 * H;

struct Ws {
    long pack, stats, ghost, shared;                                             // shared part (floats)
    long meta, idx, x, hin, pairs, r, hs, ag, t1, t2, p, q, dh, dy, pmean, pm2, grad, mol;   // per molecule
};

__host__ __device__ inline Ws ws_layout(int L, long P) {
    Ws w;
    long o = 0;
    w.pack = o;  o += long(L) * PK_N * MAT;
    w.stats = o; o += long(L) * 2 * ST_SIZE;
    w.ghost = o; o += 16;
    w.shared = o;
    const long nh = long(NF) * H;
    o = 0;
    w.meta = o;  o += 16;                     // n, E, overflow
    w.idx = o;   o += NF;
    w.x = o;     o += NF * 4;
    w.hin = o;   o += NF * IN_MAX;
    w.pairs = o; o += EMAX;
    w.r = o;     o += EMAX;
    w.hs = o;    o += nh * (L + 1);           // input h of every layer, then the final h
    w.ag = o;    o += nh * L;
    w.t1 = o;    o += nh * L;                 // node_mlp.0 output (pre BN1)
    w.t2 = o;    o += nh * L;                 // node_mlp.<last> output (pre BN2)
    w.p = o;     o += nh;
    w.q = o;     o += nh;
    w.dh = o;    o += nh;
    w.dy = o;    o += nh;
    w.pmean = o; o += H;
    w.pm2 = o;   o += H;
    w.grad = o;  o += rnd16(P);
    w.mol = o;
    return w;
}

struct Args {
    int B, N, in, out, L, bn;
    POffs po;
    Ws wl;
    const float* params;
    const float* one_hot;
    const float* positions;
    const float* fragment_mask;
    const float* edge_mask;
    float* logits;
    float* batch_stats;
    int* flags;
    const float* grad_logits;
    float* grad;
    float* ws;
};

struct Lds {
    float a[NF * H];                          // node operand / pair tile U
    float b[NF * H];                          // node operand / pair tile D
    float c[NF * H];                          // aggregate / S
    float d[NF * H];                          // T / scratch
    int pairs[T];
    float r[T];
};

__device__ __forceinline__ float* mol_ws(const Args& a, int b) { return a.ws + a.wl.shared + long(b) * a.wl.mol; }
__device__ __forceinline__ const float* packed(const Args& a, int l, int m) { return a.ws + a.wl.pack + (long(l) * PK_N + m) * MAT; }
__device__ __forceinline__ float* stats(const Args& a, int l, int which) { return a.ws + a.wl.stats + (long(l) * 2 + which) * ST_SIZE; }
__device__ __forceinline__ const float* gcl_params(const Args& a, int l) { return a.params + a.po.g0 + a.po.gsize * l; }

// acc[r][e] += sum_k A[(8 pg + r) * H + k] * B[k * H + 4 cq + e],  pg = tid >> 5, cq = tid & 31; A in LDS, B in global
__device__ __forceinline__ void mm64(float (&acc)[8][4], const float* A, const float* __restrict__ B) {
    const int cq = threadIdx.x & 31, pg = threadIdx.x >> 5;
    const float* a0 = A + pg * 8 * H;
#pragma unroll 2
    for (int k = 0; k < H; k += 4) {
        float4 bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[q] = *reinterpret_cast<const float4*>(B + (k + q) * H + 4 * cq);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float4 av = *reinterpret_cast<const float4*>(a0 + r * H + k);
            const float as[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[r][0] = fmaf(as[q], bv[q].x, acc[r][0]);
                acc[r][1] = fmaf(as[q], bv[q].y, acc[r][1]);
                acc[r][2] = fmaf(as[q], bv[q].z, acc[r][2]);
                acc[r][3] = fmaf(as[q], bv[q].w, acc[r][3]);
            }
        }
    }
}

__device__ __forceinline__ void zero_acc(float (&acc)[8][4]) {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = 0.0f;
}

// acc[e][f] += sum_{p < np} X[p * H + 4 cq + e] * Y[p * H + 16 kg + f]  (a weight gradient: rows of X are output channels)
__device__ __forceinline__ void mmT(float (&acc)[4][16], const float* X, const float* Y, int np) {
    const int cq = threadIdx.x & 31, kg = threadIdx.x >> 5;
    for (int p = 0; p < np; ++p) {
        const float4 xv = *reinterpret_cast<const float4*>(X + p * H + 4 * cq);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int f4 = 0; f4 < 4; ++f4) {
            const float4 yv = *reinterpret_cast<const float4*>(Y + p * H + 16 * kg + 4 * f4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e][4 * f4 + 0] = fmaf(xs[e], yv.x, acc[e][4 * f4 + 0]);
                acc[e][4 * f4 + 1] = fmaf(xs[e], yv.y, acc[e][4 * f4 + 1]);
                acc[e][4 * f4 + 2] = fmaf(xs[e], yv.z, acc[e][4 * f4 + 2]);
                acc[e][4 * f4 + 3] = fmaf(xs[e], yv.w, acc[e][4 * f4 + 3]);
            }
        }
    }
}

// G[(4 cq + e) * ld + col0 + 16 kg + f] = acc[e][f]
__device__ __forceinline__ void store_wgrad(float* G, long ld, long col0, const float (&acc)[4][16]) {
    const int cq = threadIdx.x & 31, kg = threadIdx.x >> 5;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 16; ++f) G[long(4 * cq + e) * ld + col0 + 16 * kg + f] = acc[e][f];
}

__device__ void wgrad(float* G, long ld, long col0, const float* X, const float* Y, int np) {
    float acc[4][16];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 16; ++f) acc[e][f] = 0.0f;
    mmT(acc, X, Y, np);
    store_wgrad(G, ld, col0, acc);
}

// copy n rows of a [NF][H] array (global) to LDS, zero the rest
__device__ void load_rows(float* dst, const float* src, int n) {
    for (int e = threadIdx.x; e < NF * H; e += BT) dst[e] = e < n * H ? src[e] : 0.0f;
    __syncthreads();
}

// G[c] = sum_{p < n} X[p][c]  (column sums, p ascending)
__device__ void col_sum(float* G, const float* X, int n) {
    for (int c = threadIdx.x; c < H; c += BT) {
        float s = 0.0f;
        for (int p = 0; p < n; ++p) s += X[p * H + c];
        G[c] = s;
    }
}

// per-molecule partial statistics of X (rows < n): mean and centred sum of squares
__device__ void partial_stats(const Args& a, float* M, const float* X, int n) {
    for (int c = threadIdx.x; c < H; c += BT) {
        float s = 0.0f;
        for (int p = 0; p < n; ++p) s += X[p * H + c];
        const float mean = n > 0 ? s / float(n) : 0.0f;
        float m2 = 0.0f;
        for (int p = 0; p < n; ++p) { const float d = X[p * H + c] - mean; m2 = fmaf(d, d, m2); }
        M[a.wl.pmean + c] = mean;
        M[a.wl.pm2 + c] = m2;
    }
}

__device__ __forceinline__ float bn_apply(const float* st, const float* gb, int c, float t) {     // gb: weight, bias
    return (t - st[ST_MEAN + c]) * st[ST_INV + c] * gb[c] + gb[H + c];
}

// ---- packing: transposed and plain copies of every 128 x 128 block of the GCLs (one block per matrix)
__global__ void __launch_bounds__(BT) pack_kernel(Args a) {
    const int l = blockIdx.x / PK_N, m = blockIdx.x % PK_N;
    const POffs& o = a.po;
    const float* g = gcl_params(a, l);
    long src, ld, col0;
    bool tr;
    switch (m) {
        case PK_W1AT: src = o.e0w; ld = 2 * H + 1; col0 = 0; tr = true; break;
        case PK_W1BT: src = o.e0w; ld = 2 * H + 1; col0 = H; tr = true; break;
        case PK_W1A:  src = o.e0w; ld = 2 * H + 1; col0 = 0; tr = false; break;
        case PK_W1B:  src = o.e0w; ld = 2 * H + 1; col0 = H; tr = false; break;
        case PK_W2T:  src = o.e2w; ld = H; col0 = 0; tr = true; break;
        case PK_W2:   src = o.e2w; ld = H; col0 = 0; tr = false; break;
        case PK_W3AT: src = o.n0w; ld = 2 * H; col0 = 0; tr = true; break;
        case PK_W3BT: src = o.n0w; ld = 2 * H; col0 = H; tr = true; break;
        case PK_W3A:  src = o.n0w; ld = 2 * H; col0 = 0; tr = false; break;
        case PK_W3B:  src = o.n0w; ld = 2 * H; col0 = H; tr = false; break;
        case PK_W4T:  src = o.n3w; ld = H; col0 = 0; tr = true; break;
        default:      src = o.n3w; ld = H; col0 = 0; tr = false; break;
    }
    float* dst = a.ws + a.wl.pack + (long(l) * PK_N + m) * MAT;
    for (int e = threadIdx.x; e < MAT; e += BT) {
        const int r = e >> 7, c = e & (H - 1);                     // dst[r][c]
        dst[e] = tr ? g[src + long(c) * ld + col0 + r] : g[src + long(r) * ld + col0 + c];
    }
}

// ---- forward, first launch: compaction, masked inputs, the kept-edge list, embedding_in
__global__ void __launch_bounds__(BT) embed_kernel(Args a) {
    __shared__ int sIdx[NF];
    __shared__ float sX[NF * 4];
    __shared__ int sCount;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    float* M = mol_ws(a, b);
    int* meta = reinterpret_cast<int*>(M + a.wl.meta);
    float* H0 = M + a.wl.hs;
    const float* We = a.params + a.po.emb_w;
    const float* be = a.params + a.po.emb_b;
    if (b == a.B) {                                                // the ghost row: h = embedding_in.bias, no edge
        if (tid == 0) { meta[0] = 1; meta[1] = 0; meta[2] = 0; }
        for (int c = tid; c < H; c += BT) H0[c] = be[c];
        return;
    }
    if (tid < 64) {
        int count = 0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + tid;
            const bool real = (i < N) && (a.fragment_mask[long(b) * N + i] != 0.0f);
            const unsigned long long bal = __ballot(real);
            const int pos = count + __popcll(bal & ((1ull << tid) - 1ull));
            if (real && pos < NF) sIdx[pos] = i;
            count += __popcll(bal);
        }
        if (tid == 0) sCount = count;
    }
    __syncthreads();
    const int total = sCount;
    const int n = total > NF ? 0 : total;                          // overflow: flagged, the molecule contributes no row
    if (tid == 0) { meta[0] = n; meta[2] = total > NF; a.flags[b] = total > NF ? 4 : 0; }
    if (tid < 4 * n) {
        const int i = tid >> 2, k = tid & 3;
        const long row = long(b) * N + sIdx[i];
        const float v = k < 3 ? a.positions[row * 3 + k] * a.fragment_mask[row] : 0.0f;
        sX[tid] = v;
        M[a.wl.x + tid] = v;
    }
    if (tid < n) reinterpret_cast<int*>(M + a.wl.idx)[tid] = sIdx[tid];
    for (int e = tid; e < n * IN_MAX; e += BT) {
        const int i = e / IN_MAX, q = e % IN_MAX;
        const long row = long(b) * N + sIdx[i];
        M[a.wl.hin + e] = q < a.in ? a.one_hot[row * a.in + q] * a.fragment_mask[row] : 0.0f;
    }
    __syncthreads();
    // kept edges, (i, j) ascending: wave 0, one receiver per step, senders on the lanes
    if (tid < 64) {
        int count = 0;
        int* pairs = reinterpret_cast<int*>(M + a.wl.pairs);
        for (int i = 0; i < n; ++i) {
            const int j = tid;
            bool keep = false;
            float r = 0.0f;
            if (j < n) {
                const float d0 = sX[4 * i] - sX[4 * j], d1 = sX[4 * i + 1] - sX[4 * j + 1], d2 = sX[4 * i + 2] - sX[4 * j + 2];
                r = d0 * d0 + d1 * d1 + d2 * d2;                    // coord2diff `radial` (egnn.py:298)
                keep = (a.edge_mask[(long(b) * N + sIdx[i]) * N + sIdx[j]] != 0.0f) && (r < 6.0f);
            }
            const unsigned long long bal = __ballot(keep);
            const int pos = count + __popcll(bal & ((1ull << tid) - 1ull));
            if (keep) { pairs[pos] = i | (j << 8); M[a.wl.r + pos] = r; }
            count += __popcll(bal);
        }
        if (tid == 0) meta[1] = count;
    }
    // embedding_in on the masked one-hot
    const int c = tid & (H - 1);
    for (int i = tid >> 7; i < n; i += 2) {
        float s = be[c];
        for (int q = 0; q < a.in; ++q) s = fmaf(M[a.wl.hin + i * IN_MAX + q], We[long(c) * a.in + q], s);
        H0[i * H + c] = s;
    }
}

// h_{l+1} = (h_l + BN2(t2_l)) * nm, rows < n (the ghost row: 0)
__device__ void finish_layer(const Args& a, float* M, int l, int n, bool ghost) {
    const float* h = M + a.wl.hs + long(l) * NF * H;
    const float* t2 = M + a.wl.t2 + long(l) * NF * H;
    float* hn = M + a.wl.hs + long(l + 1) * NF * H;
    const float* st = stats(a, l, 1);
    const float* gb = gcl_params(a, l) + a.po.bn2w;
    for (int e = threadIdx.x; e < n * H; e += BT) hn[e] = ghost ? 0.0f : h[e] + bn_apply(st, gb, e & (H - 1), t2[e]);
    __syncthreads();
}

// P = H W1a^T + b1, Q = H W1b^T (rows of the molecule), to the workspace; H in L.a
__device__ void node_pq(const Args& a, Lds& L, float* M, int l) {
    const int cq = threadIdx.x & 31, pg = threadIdx.x >> 5;
    const float* g = gcl_params(a, l);
    for (int which = 0; which < 2; ++which) {
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.a, packed(a, l, which == 0 ? PK_W1AT : PK_W1BT));
        float* out = M + (which == 0 ? a.wl.p : a.wl.q);
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * cq + e;
                out[(8 * pg + r) * H + c] = acc[r][e] + (which == 0 ? g[a.po.e0b + c] : 0.0f);
            }
    }
    __syncthreads();
}

// U[p][c] = relu(P[i_p][c] + Q[j_p][c] + r_p wd[c]) for the pairs of tile [p0, p0 + np) in L.a (rows >= np zero)
__device__ void build_u(const Args& a, Lds& L, const float* M, int l, int p0, int np) {
    const int* pairs = reinterpret_cast<const int*>(M + a.wl.pairs);
    if (threadIdx.x < T) {
        L.pairs[threadIdx.x] = threadIdx.x < np ? pairs[p0 + threadIdx.x] : 0;
        L.r[threadIdx.x] = threadIdx.x < np ? M[a.wl.r + p0 + threadIdx.x] : 0.0f;
    }
    __syncthreads();
    const float* w1 = gcl_params(a, l) + a.po.e0w;
    const int c = threadIdx.x & (H - 1);
    const float wd = w1[long(c) * (2 * H + 1) + 2 * H];
    for (int p = threadIdx.x >> 7; p < T; p += 2) {
        float v = 0.0f;
        if (p < np) {
            const int i = L.pairs[p] & 255, j = L.pairs[p] >> 8;
            v = fmaxf(M[a.wl.p + i * H + c] + M[a.wl.q + j * H + c] + L.r[p] * wd, 0.0f);
        }
        L.a[p * H + c] = v;
    }
    __syncthreads();
}

// ---- forward, per layer, first launch
__global__ void __launch_bounds__(BT) gcl_a_kernel(Args a, int l) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    const int* meta = reinterpret_cast<const int*>(M + a.wl.meta);
    const int n = meta[0], E = meta[1];
    if (l > 0 && a.bn) finish_layer(a, M, l - 1, n, ghost);
    const float* g = gcl_params(a, l);
    const float* h = M + a.wl.hs + long(l) * NF * H;
    float* agg = M + a.wl.ag + long(l) * NF * H;
    float* t1 = M + a.wl.t1 + long(l) * NF * H;
    const int cq = tid & 31, pg = tid >> 5;

    load_rows(L.a, h, n);
    node_pq(a, L, M, l);
    for (int e = tid; e < NF * H; e += BT) L.c[e] = 0.0f;           // aggregate
    // edge pass over the kept pairs
    for (int p0 = 0; p0 < E; p0 += T) {
        const int np = min(T, E - p0);
        build_u(a, L, M, l, p0, np);
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.a, packed(a, l, PK_W2T));
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * cq + e;
                L.b[(8 * pg + r) * H + c] = fmaxf(acc[r][e] + g[a.po.e2b + c], 0.0f);
            }
        __syncthreads();
        if (tid < H)                                               // agg_i += m_ij, pairs in list order
            for (int p = 0; p < np; ++p) L.c[(L.pairs[p] & 255) * H + tid] += L.b[p * H + tid];
        __syncthreads();
    }
    for (int e = tid; e < n * H; e += BT) agg[e] = L.c[e];
    load_rows(L.a, h, n);
    // t1 = W3a h + W3b agg + b3
    {
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.a, packed(a, l, PK_W3AT));
        mm64(acc, L.c, packed(a, l, PK_W3BT));
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 8 * pg + r, c = 4 * cq + e;
                const float v = acc[r][e] + g[a.po.n0b + c];
                L.b[p * H + c] = v;
                if (p < n) t1[p * H + c] = v;
            }
        __syncthreads();
    }
    if (a.bn) {
        partial_stats(a, M, L.b, n);
        return;
    }
    // normalization None: relu, node_mlp.2, residual, node mask
    for (int e = tid; e < NF * H; e += BT) L.d[e] = fmaxf(L.b[e], 0.0f);
    __syncthreads();
    float acc[8][4];
    zero_acc(acc);
    mm64(acc, L.d, packed(a, l, PK_W4T));
    float* t2 = M + a.wl.t2 + long(l) * NF * H;
    float* hn = M + a.wl.hs + long(l + 1) * NF * H;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 8 * pg + r, c = 4 * cq + e;
            if (p < n) {
                const float v = acc[r][e] + g[a.po.n3b + c];
                t2[p * H + c] = v;
                hn[p * H + c] = ghost ? 0.0f : L.a[p * H + c] + v;
            }
        }
}

// ---- forward, per layer, second launch (BatchNorm only): BN1, relu, node_mlp.3, BN2 partials
__global__ void __launch_bounds__(BT) gcl_b_kernel(Args a, int l) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    float* M = mol_ws(a, b);
    const int n = reinterpret_cast<const int*>(M + a.wl.meta)[0];
    const float* g = gcl_params(a, l);
    const float* st = stats(a, l, 0);
    const float* t1 = M + a.wl.t1 + long(l) * NF * H;
    for (int e = tid; e < NF * H; e += BT) L.a[e] = e < n * H ? fmaxf(bn_apply(st, g + a.po.bn1w, e & (H - 1), t1[e]), 0.0f) : 0.0f;
    __syncthreads();
    const int cq = tid & 31, pg = tid >> 5;
    float acc[8][4];
    zero_acc(acc);
    mm64(acc, L.a, packed(a, l, PK_W4T));
    float* t2 = M + a.wl.t2 + long(l) * NF * H;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 8 * pg + r, c = 4 * cq + e;
            const float v = acc[r][e] + g[a.po.n3b + c];
            L.b[p * H + c] = v;
            if (p < n) t2[p * H + c] = v;
        }
    __syncthreads();
    partial_stats(a, M, L.b, n);
}

// ---- the ghost row's multiplicity G = B*N - sum_b n_b
__global__ void __launch_bounds__(64) ghost_kernel(Args a) {
    if (threadIdx.x != 0) return;
    long nsum = 0;
    for (int b = 0; b < a.B; ++b) nsum += reinterpret_cast<const int*>(mol_ws(a, b) + a.wl.meta)[0];
    a.ws[a.wl.ghost] = float(long(a.B) * a.N - nsum);
}

// ---- batch statistics of one BatchNorm: merge the per-molecule (n_b, mean_b, M2_b), b = 0..B-1, then the ghost row (G, x, 0)
__global__ void __launch_bounds__(H) stats_kernel(Args a, int l, int which) {
    const int c = threadIdx.x;
    const double G = a.ws[a.wl.ghost];
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int b = 0; b <= a.B; ++b) {
        const float* M = mol_ws(a, b);
        const double nb = b == a.B ? G : double(reinterpret_cast<const int*>(M + a.wl.meta)[0]);
        if (nb <= 0.0) continue;
        const double mb = M[a.wl.pmean + c], m2b = b == a.B ? 0.0 : double(M[a.wl.pm2 + c]);
        const double tot = cnt + nb, d = mb - mean;
        mean += d * nb / tot;
        m2 += m2b + d * d * cnt * nb / tot;
        cnt = tot;
    }
    const double var = m2 / cnt;
    float* st = stats(a, l, which);
    st[ST_MEAN + c] = float(mean);
    st[ST_VAR + c] = float(var);
    st[ST_INV + c] = float(1.0 / sqrt(var + double(BN_EPS)));
    float* out = a.batch_stats + ((long(l) * 2 + which) * 2) * H;
    out[c] = float(mean);
    out[H + c] = float(var);
}

// ---- forward, last launch: finish the last layer, embedding_out, mean over the N padded rows
__global__ void __launch_bounds__(BT) logits_kernel(Args a) {
    const int b = blockIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    const int n = reinterpret_cast<const int*>(M + a.wl.meta)[0];
    if (a.bn) finish_layer(a, M, a.L - 1, n, ghost);
    if (ghost) return;
    const float* hL = M + a.wl.hs + long(a.L) * NF * H;
    const float* Wo = a.params + a.po.out_w;
    const float* bo = a.params + a.po.out_b;
    for (int o = threadIdx.x; o < a.out; o += BT) {
        float sum = 0.0f;
        for (int i = 0; i < n; ++i) {
            float acc = bo[o];
            for (int k = 0; k < H; ++k) acc = fmaf(hL[i * H + k], Wo[long(o) * H + k], acc);
            sum += acc;
        }
        sum += float(a.N - n) * bo[o];
        a.logits[long(b) * a.out + o] = sum / float(a.N);
    }
}

// ---- backward, first launch: embedding_out and the mean
__global__ void __launch_bounds__(BT) bwd_out_kernel(Args a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    float* G = M + a.wl.grad;
    const int n = reinterpret_cast<const int*>(M + a.wl.meta)[0];
    const float* hL = M + a.wl.hs + long(a.L) * NF * H;
    const float* Wo = a.params + a.po.out_w;
    const float* dl = a.grad_logits + long(ghost ? 0 : b) * a.out;
    const float invN = 1.0f / float(a.N);
    for (int e = tid; e < a.out * H; e += BT) {                   // dW_out[o][k] = dl[o] / N * sum_i h_i[k]
        const int o = e / H, k = e % H;
        float s = 0.0f;
        if (!ghost)
            for (int i = 0; i < n; ++i) s += hL[i * H + k];
        G[a.po.out_w + e] = ghost ? 0.0f : dl[o] * invN * s;
    }
    for (int o = tid; o < a.out; o += BT) G[a.po.out_b + o] = ghost ? 0.0f : dl[o];
    float* dh = M + a.wl.dh;
    const int c = tid & (H - 1);
    float s = 0.0f;
    if (!ghost)
        for (int o = 0; o < a.out; ++o) s = fmaf(Wo[long(o) * H + c], dl[o] * invN, s);
    for (int i = tid >> 7; i < n; i += 2) dh[i * H + c] = ghost ? 0.0f : s;
}

// ---- backward, BatchNorm only: the per-molecule sums of dy and dy * xhat of BN2, into the slice's weight / bias entries
__global__ void __launch_bounds__(BT) bwd_b_kernel(Args a, int l) {
    const int b = blockIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    const int n = reinterpret_cast<const int*>(M + a.wl.meta)[0];
    float* G = M + a.wl.grad + a.po.g0 + a.po.gsize * l;
    const float* st = stats(a, l, 1);
    const float* t2 = M + a.wl.t2 + long(l) * NF * H;
    const float* dh = M + a.wl.dh;
    for (int c = threadIdx.x; c < H; c += BT) {
        float sdy = 0.0f, sdx = 0.0f;
        if (!ghost)                                                // do = dh * nm: zero on the ghost row
            for (int p = 0; p < n; ++p) {
                const float dy = dh[p * H + c];
                sdy += dy;
                sdx = fmaf(dy, (t2[p * H + c] - st[ST_MEAN + c]) * st[ST_INV + c], sdx);
            }
        G[a.po.bn2w + c] = sdx;
        G[a.po.bn2b + c] = sdy;
    }
}

// totals of sum dy, sum dy * xhat over the batch: molecules in order, then G x the ghost row (the same order as reduce)
__global__ void __launch_bounds__(H) bsum_kernel(Args a, int l, int which) {
    const int c = threadIdx.x;
    const double G = a.ws[a.wl.ghost];
    const long gw = a.po.g0 + a.po.gsize * l + (which == 0 ? a.po.bn1w : a.po.bn2w);
    double sdx = 0.0, sdy = 0.0;
    for (int b = 0; b <= a.B; ++b) {
        const float* S = mol_ws(a, b) + a.wl.grad + gw;
        const double w = b == a.B ? G : 1.0;
        sdx += w * S[c];
        sdy += w * S[H + c];
    }
    float* st = stats(a, l, which);
    st[ST_SDX + c] = float(sdx);
    st[ST_SDY + c] = float(sdy);
}

// BatchNorm backward of one entry: dx = gamma / sigma (dy - sum dy / R - xhat sum dy xhat / R)
__device__ __forceinline__ float bn_back(const float* st, const float* gamma, int c, float x, float dy, float invR) {
    const float xh = (x - st[ST_MEAN + c]) * st[ST_INV + c];
    return gamma[c] * st[ST_INV + c] * (dy - st[ST_SDY + c] * invR - xh * st[ST_SDX + c] * invR);
}

// ---- backward, per layer: BN2 backward, node_mlp.<last>, the BN1 partials
__global__ void __launch_bounds__(BT) bwd_mid_kernel(Args a, int l) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    const int n = reinterpret_cast<const int*>(M + a.wl.meta)[0];
    const float* g = gcl_params(a, l);
    float* G = M + a.wl.grad + a.po.g0 + a.po.gsize * l;
    const float invR = 1.0f / float(long(a.B) * a.N);
    const float* t1 = M + a.wl.t1 + long(l) * NF * H;
    const float* t2 = M + a.wl.t2 + long(l) * NF * H;
    const float* dh = M + a.wl.dh;
    const float* st1 = stats(a, l, 0);
    const float* st2 = stats(a, l, 1);
    // L.b = dt2, L.a = a (relu of BN1(t1) / of t1), L.d = y1 (pre-relu)
    for (int e = tid; e < NF * H; e += BT) {
        const int p = e >> 7, c = e & (H - 1);
        float dt2 = 0.0f, act = 0.0f, y1 = 0.0f;
        if (p < n) {
            const float dout = ghost ? 0.0f : dh[e];
            dt2 = a.bn ? bn_back(st2, g + a.po.bn2w, c, t2[e], dout, invR) : dout;
            y1 = a.bn ? bn_apply(st1, g + a.po.bn1w, c, t1[e]) : t1[e];
            act = fmaxf(y1, 0.0f);
        }
        L.b[e] = dt2;
        L.a[e] = act;
        L.d[e] = y1;
    }
    __syncthreads();
    wgrad(G + a.po.n3w, H, 0, L.b, L.a, n);
    col_sum(G + a.po.n3b, L.b, n);
    // da = dt2 W4, dy1 = da (y1 > 0)
    const int cq = tid & 31, pg = tid >> 5;
    float acc[8][4];
    zero_acc(acc);
    mm64(acc, L.b, packed(a, l, PK_W4));
    float* dy = M + a.wl.dy;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 8 * pg + r, c = 4 * cq + e;
            if (p < n) dy[p * H + c] = L.d[p * H + c] > 0.0f ? acc[r][e] : 0.0f;
        }
    __syncthreads();
    if (!a.bn) return;
    for (int c = tid; c < H; c += BT) {
        float sdy = 0.0f, sdx = 0.0f;
        for (int p = 0; p < n; ++p) {
            const float v = dy[p * H + c];
            sdy += v;
            sdx = fmaf(v, (t1[p * H + c] - st1[ST_MEAN + c]) * st1[ST_INV + c], sdx);
        }
        G[a.po.bn1w + c] = sdx;
        G[a.po.bn1b + c] = sdy;
    }
}

// ---- backward, per layer: BN1 backward, node_mlp.0, the edge pass, embedding_in for gcl1
__global__ void __launch_bounds__(BT) bwd_a_kernel(Args a, int l) {
    __shared__ Lds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ghost = b == a.B;
    float* M = mol_ws(a, b);
    const int* meta = reinterpret_cast<const int*>(M + a.wl.meta);
    const int n = meta[0], E = meta[1];
    const float* g = gcl_params(a, l);
    float* G = M + a.wl.grad + a.po.g0 + a.po.gsize * l;
    const float invR = 1.0f / float(long(a.B) * a.N);
    const float* h = M + a.wl.hs + long(l) * NF * H;
    const float* agg = M + a.wl.ag + long(l) * NF * H;
    const float* t1 = M + a.wl.t1 + long(l) * NF * H;
    const float* st1 = stats(a, l, 0);
    float* dh = M + a.wl.dh;
    const float* dy = M + a.wl.dy;
    const int cq = tid & 31, pg = tid >> 5;
    // L.b = dt1, L.a = h, L.c = agg
    for (int e = tid; e < NF * H; e += BT) {
        const int p = e >> 7, c = e & (H - 1);
        float v = 0.0f;
        if (p < n) v = a.bn ? bn_back(st1, g + a.po.bn1w, c, t1[e], dy[e], invR) : dy[e];
        L.b[e] = v;
    }
    load_rows(L.a, h, n);
    load_rows(L.c, agg, n);
    wgrad(G + a.po.n0w, 2 * H, 0, L.b, L.a, n);
    wgrad(G + a.po.n0w, 2 * H, H, L.b, L.c, n);
    col_sum(G + a.po.n0b, L.b, n);
    // dh_new = dh nm (residual) + dt1 W3a (to the workspace, L.d = dagg = dt1 W3b)
    {
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.b, packed(a, l, PK_W3A));
        float acc2[8][4];
        zero_acc(acc2);
        mm64(acc2, L.b, packed(a, l, PK_W3B));
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 8 * pg + r, c = 4 * cq + e;
                if (p < n) dh[p * H + c] = (ghost ? 0.0f : dh[p * H + c]) + acc[r][e];
                L.d[p * H + c] = acc2[r][e];
            }
        __syncthreads();
    }
    // edge pass: recompute P, Q (L.a holds h), then per tile u, pre2, dpre2, dW2, dpre1; S_i = sum_j dpre1_ij in L.c,
    // T_j = sum_i dpre1_ij in L.d, both summed in pair-list order
    node_pq(a, L, M, l);
    float* dagg = M + a.wl.dy;                                     // dy is consumed: reuse for dagg
    for (int e = tid; e < n * H; e += BT) dagg[e] = L.d[e];
    for (int e = tid; e < NF * H; e += BT) { L.c[e] = 0.0f; L.d[e] = 0.0f; }   // S, T
    // dW2, db2 and dwd sum over all kept pairs (up to 4096): each tile's sum is formed on its own and then added to the
    // total, so a sum is two short chains rather than one long one (fp32 rounding of a plain chain grows with its length)
    float wtot[4][16];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 16; ++f) wtot[e][f] = 0.0f;
    float sb2 = 0.0f, swd = 0.0f, sb1 = 0.0f;                       // threads < 128: db2[c], dwd[c], db1[c]
    __syncthreads();
    for (int p0 = 0; p0 < E; p0 += T) {
        const int np = min(T, E - p0);
        build_u(a, L, M, l, p0, np);
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.a, packed(a, l, PK_W2T));
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 8 * pg + r, c = 4 * cq + e;
                float v = 0.0f;
                if (p < np && acc[r][e] + g[a.po.e2b + c] > 0.0f) v = dagg[(L.pairs[p] & 255) * H + c];
                L.b[p * H + c] = v;                                 // dpre2
            }
        __syncthreads();
        {
            float wacc[4][16];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int f = 0; f < 16; ++f) wacc[e][f] = 0.0f;
            mmT(wacc, L.b, L.a, np);                                 // dW2 += dpre2^T u
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int f = 0; f < 16; ++f) wtot[e][f] += wacc[e][f];
        }
        zero_acc(acc);
        mm64(acc, L.b, packed(a, l, PK_W2));                         // du = dpre2 W2
        if (tid < H) {
            float t = 0.0f;
            for (int p = 0; p < np; ++p) t += L.b[p * H + tid];
            sb2 += t;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 8 * pg + r, c = 4 * cq + e;
                L.b[p * H + c] = L.a[p * H + c] > 0.0f ? acc[r][e] : 0.0f;   // dpre1
            }
        __syncthreads();
        if (tid < H) {
            float t = 0.0f;
            for (int p = 0; p < np; ++p) {
                const float v = L.b[p * H + tid];
                L.c[(L.pairs[p] & 255) * H + tid] += v;
                t = fmaf(v, L.r[p], t);
            }
            swd += t;
        } else {
            const int c = tid - H;
            for (int p = 0; p < np; ++p) L.d[(L.pairs[p] >> 8) * H + c] += L.b[p * H + c];
        }
        __syncthreads();
    }
    store_wgrad(G + a.po.e2w, H, 0, wtot);
    if (tid < H) {
        G[a.po.e2b + tid] = sb2;
        G[a.po.e0w + long(tid) * (2 * H + 1) + 2 * H] = swd;
        for (int p = 0; p < n; ++p) sb1 += L.c[p * H + tid];
        G[a.po.e0b + tid] = sb1;
    }
    load_rows(L.a, h, n);
    wgrad(G + a.po.e0w, 2 * H + 1, 0, L.c, L.a, n);                 // dW1a = S^T h
    wgrad(G + a.po.e0w, 2 * H + 1, H, L.d, L.a, n);                 // dW1b = T^T h
    {
        float acc[8][4];
        zero_acc(acc);
        mm64(acc, L.c, packed(a, l, PK_W1A));
        mm64(acc, L.d, packed(a, l, PK_W1B));
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 8 * pg + r, c = 4 * cq + e;
                if (p < n) dh[p * H + c] += acc[r][e];
            }
        __syncthreads();
    }
    if (l > 0) {
        // h_l = (h_{l-1} + o) nm: the ghost row's dh stops here, the molecules' flows on through bwd_b / bwd_mid
        if (ghost)
            for (int e = tid; e < n * H; e += BT) dh[e] = 0.0f;
        return;
    }
    // embedding_in: dW[c][q] = sum_i dh_i[c] hin_i[q], db = sum_i dh_i
    float* GE = M + a.wl.grad;
    for (int e = tid; e < H * a.in; e += BT) {
        const int c = e / a.in, q = e % a.in;
        float s = 0.0f;
        for (int i = 0; i < n; ++i) s = fmaf(dh[i * H + c], ghost ? 0.0f : M[a.wl.hin + i * IN_MAX + q], s);
        GE[a.po.emb_w + e] = s;
    }
    for (int c = tid; c < H; c += BT) {
        float s = 0.0f;
        for (int i = 0; i < n; ++i) s += dh[i * H + c];
        GE[a.po.emb_b + c] = s;
    }
}

// grad[p] = sum_{b < B} slice_b[p] + G slice_ghost[p], b ascending
__global__ void __launch_bounds__(256) reduce_kernel(Args a) {
    const long p = long(blockIdx.x) * 256 + threadIdx.x;
    if (p >= a.po.total) return;
    float s = 0.0f;
    for (int b = 0; b < a.B; ++b) s += mol_ws(a, b)[a.wl.grad + p];
    s = fmaf(a.ws[a.wl.ghost], mol_ws(a, a.B)[a.wl.grad + p], s);
    a.grad[p] = s;
}

bool scope_ok(const dl_size_train_args* a) {
    return a->hidden_nf == H && a->n_layers >= 1 && a->n_layers <= 64 && a->in_node_nf >= 1 && a->in_node_nf <= IN_MAX &&
           a->out_node_nf >= 1 && a->out_node_nf <= OUT_MAX && (a->batch_norm == 0 || a->batch_norm == 1);
}

size_t ws_bytes(const dl_size_train_args* a) {
    const POffs po = param_offsets(a->in_node_nf, a->out_node_nf, a->n_layers, a->batch_norm);
    const Ws w = ws_layout(a->n_layers, po.total);
    return size_t(w.shared + (long(a->B) + 1) * w.mol) * sizeof(float);
}

int32_t prepare(const dl_size_train_args* a, Args& k) {
    if (!a) return DL_ERR_BAD_ARG;
    if (!scope_ok(a)) return DL_ERR_UNSUPPORTED;
    if (a->B < 1 || a->N < 1) return DL_ERR_BAD_ARG;
    if (a->batch_norm && long(a->B) * a->N < 2) return DL_ERR_BAD_ARG;       // BatchNorm1d refuses one row in training mode
    k.po = param_offsets(a->in_node_nf, a->out_node_nf, a->n_layers, a->batch_norm);
    if (a->n_params != k.po.total) return DL_ERR_BAD_ARG;
    if (!a->params || !a->workspace || a->workspace_bytes < ws_bytes(a)) return DL_ERR_BAD_ARG;
    k.B = a->B; k.N = a->N; k.in = a->in_node_nf; k.out = a->out_node_nf; k.L = a->n_layers; k.bn = a->batch_norm;
    k.wl = ws_layout(a->n_layers, k.po.total);
    k.params = a->params; k.one_hot = a->one_hot; k.positions = a->positions; k.fragment_mask = a->fragment_mask;
    k.edge_mask = a->edge_mask; k.logits = a->logits; k.batch_stats = a->batch_stats; k.flags = a->flags;
    k.grad_logits = a->grad_logits; k.grad = a->grad_params; k.ws = static_cast<float*>(a->workspace);
    return DL_OK;
}

}  // namespace

extern "C" {

int64_t dl_size_train_num_params(const dl_size_train_args* a) {
    if (!a || !scope_ok(a)) return -1;
    return param_offsets(a->in_node_nf, a->out_node_nf, a->n_layers, a->batch_norm).total;
}

size_t dl_size_train_workspace_bytes(const dl_size_train_args* a) {
    if (!a || !scope_ok(a) || a->B < 1) return 0;
    return ws_bytes(a);
}

int32_t dl_size_train_forward(const dl_size_train_args* a, void* stream) {
    Args k;
    const int32_t st = prepare(a, k);
    if (st != DL_OK) return st;
    if (!a->one_hot || !a->positions || !a->fragment_mask || !a->edge_mask || !a->logits || !a->batch_stats || !a->flags)
        return DL_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 mols(unsigned(a->B + 1));
    hipLaunchKernelGGL(pack_kernel, dim3(unsigned(k.L * PK_N)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(embed_kernel, mols, dim3(BT), 0, s, k);
    hipLaunchKernelGGL(ghost_kernel, dim3(1), dim3(64), 0, s, k);
    for (int l = 0; l < k.L; ++l) {
        hipLaunchKernelGGL(gcl_a_kernel, mols, dim3(BT), 0, s, k, l);
        if (!k.bn) continue;
        hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(H), 0, s, k, l, 0);
        hipLaunchKernelGGL(gcl_b_kernel, mols, dim3(BT), 0, s, k, l);
        hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(H), 0, s, k, l, 1);
    }
    hipLaunchKernelGGL(logits_kernel, mols, dim3(BT), 0, s, k);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_size_train_backward(const dl_size_train_args* a, void* stream) {
    Args k;
    const int32_t st = prepare(a, k);
    if (st != DL_OK) return st;
    if (!a->grad_logits || !a->grad_params) return DL_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 mols(unsigned(a->B + 1));
    hipLaunchKernelGGL(bwd_out_kernel, mols, dim3(BT), 0, s, k);
    for (int l = k.L - 1; l >= 0; --l) {
        if (k.bn) {
            hipLaunchKernelGGL(bwd_b_kernel, mols, dim3(BT), 0, s, k, l);
            hipLaunchKernelGGL(bsum_kernel, dim3(1), dim3(H), 0, s, k, l, 1);
        }
        hipLaunchKernelGGL(bwd_mid_kernel, mols, dim3(BT), 0, s, k, l);
        if (k.bn) hipLaunchKernelGGL(bsum_kernel, dim3(1), dim3(H), 0, s, k, l, 0);
        hipLaunchKernelGGL(bwd_a_kernel, mols, dim3(BT), 0, s, k, l);
    }
    hipLaunchKernelGGL(reduce_kernel, dim3(unsigned((k.po.total + 255) / 256)), dim3(256), 0, s, k);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
