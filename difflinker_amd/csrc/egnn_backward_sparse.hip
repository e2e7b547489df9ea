// egnn_backward_sparse.hip — gradient of the pocket-conditioned EGNN denoiser (reference DynamicsWithPockets.forward,
// src/egnn.py:470-552, on the radius graph of get_dist_edges :554-596, EGNN with edge_mask=None) with respect to every
// parameter, for training.  Same scope and the same flat parameter layout as egnn_backward.hip (backward_layout.h).
//
// Unlike the fully-connected backward (one workgroup per molecule, every pair), the work here follows the EDGE LIST:
//   graph      rebuilt from z_t's masked coordinates by the rule and the fp32 arithmetic of egnn_sparse.hip's pk_edges_kernel
//              (one wave per atom: count -> scan -> fill), as a CSR neighbour list sorted by sender, plus for every edge the
//              slot of its reverse edge (the graph is symmetric).  The distance test carries no gradient.
//   node ops   (projections W_a h + b1, W_b h, node MLP, their transposes and weight gradients) are small kernels over all
//              B*N atoms.
//   edge pass  k_edge: a molecule's edges are cut into tiles of 32; molecule b's tiles are dealt round-robin to G workgroups
//              (G depends on N only), so B*G workgroups cover the chip.  Per tile pre1 / m1 are recomputed from the saved node
//              state, then the three pair GEMMs run on v_mfma_f32_32x32x2_f32 with fp32 accumulation: pre2 = m1 W2^T,
//              dW2 += dpre2^T m1 (accumulators live in registers across the workgroup's tiles) and dm1 = dpre2 W2.
//              Per-edge results (the forward message m2, then dpre1, and the x gradient of the receiver) go to a per-edge
//              buffer; receivers sum their own contiguous edge range and, through the reverse-edge slots, the sender side.
//   reductions no float atomics.  A workgroup writes its weight-gradient partial; k_edge_reduce sums a molecule's G partials
//              in order into the molecule's gradient slice; k_final_reduce sums the slices b = 0 .. B-1 in order.  A
//              molecule's slice depends on that molecule alone.
// The per-edge buffers are sized for the worst case B*N*(N-1) edges (the host cannot know the count without a sync);
// only the first E rows are ever touched.
#include "backward_layout.h"

namespace {

constexpr int LDT = 132;                       // LDS row stride of a [32][128] / [128][128] fp32 tile
constexpr int TE = 32;                         // edges per tile
constexpr int ET = 256;                        // threads of the edge kernel (4 waves)
constexpr int WLD = H + 1;
constexpr int PK_BWD_MAX_ATOMS = 2048;
constexpr int EPS = H * H + 4 * H;             // floats of a workgroup's partial: dW2, db2, dw_r, dw_d, dw3
constexpr int F_REAL = 1, F_LIG = 2, F_POCK = 4;

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float dsilu(float v) {
    const float s = 1.0f / (1.0f + expf(-v));
    return s * (1.0f + v * (1.0f - s));
}

__host__ __device__ inline size_t rnd64(size_t v) { return (v + 63) & ~size_t(63); }

inline int groups_per_molecule(int N) {        // workgroups per molecule of the edge pass: a function of N alone
    const long g = long(N) * N / 2560;
    return int(g < 1 ? 1 : g > 64 ? 64 : g);
}

struct Ws {                                    // offsets in 4-byte words
    size_t hs, ag, xs, hin, a, bm, u, du, dh, dh2, dagg, si, tj, dx, dxacc, dmean, gp, ep, eb, ex;
    size_t flags, deg, off, col, rev, total;
};

inline Ws ws_layout(int B, int N, int L, int S, long P) {
    Ws w;
    size_t o = 0;
    const size_t V = size_t(B) * N, vh = rnd64(V * H), v4 = rnd64(V * 4);
    const size_t emax = rnd64(V * size_t(N > 1 ? N - 1 : 1));
    auto take = [&](size_t n) { const size_t r = o; o += rnd64(n); return r; };
    w.hs = take(vh * (size_t(L) * (S + 1) + 1));
    w.ag = take(vh * size_t(L) * S);
    w.xs = take(v4 * (L + 1));
    w.hin = take(V * MAX_FIN);
    w.a = take(vh); w.bm = take(vh); w.u = take(vh); w.du = take(vh); w.dh = take(vh); w.dh2 = take(vh);
    w.dagg = take(vh); w.si = take(vh); w.tj = take(vh);
    w.dx = take(v4); w.dxacc = take(v4);
    w.dmean = take(size_t(B) * 4);
    w.gp = take(size_t(B) * P);
    w.ep = take(size_t(B) * groups_per_molecule(N) * EPS);
    w.eb = take(emax * H);
    w.ex = take(emax * 4);
    w.flags = take(V); w.deg = take(V); w.off = take(V + 1);
    w.col = take(emax); w.rev = take(emax);
    w.total = o;
    return w;
}

// ---- inputs and graph ----------------------------------------------------------------------------------------------------
struct InitArgs {
    int V, N, nf, ctx, cond_t, t_scalar;
    const float *xh, *t, *nm, *lm, *context;
    float *x0, *hin;
    int* flags;
};

// masked coordinates and features, time and context appended (egnn.py:480-512); role flags as pk_init_kernel sets them
__global__ void k_init(InitArgs a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.V) return;
    const int D = 3 + a.nf, b = v / a.N;
    const bool real = a.nm[v] != 0.0f;
    const float nm = real ? 1.0f : 0.0f;
    const float* z = a.xh + size_t(v) * D;
    for (int q = 0; q < 4; ++q) a.x0[4 * size_t(v) + q] = q < 3 ? z[q] * nm : 0.0f;
    float* hin = a.hin + size_t(v) * MAX_FIN;
    for (int k = 0; k < a.nf; ++k) hin[k] = z[3 + k] * nm;
    if (a.cond_t) hin[a.nf] = a.t_scalar ? a.t[0] : a.t[b];
    for (int k = 0; k < a.ctx; ++k) hin[a.nf + a.cond_t + k] = a.context[size_t(v) * a.ctx + k];
    for (int k = a.nf + a.cond_t + a.ctx; k < MAX_FIN; ++k) hin[k] = 0.0f;
    const bool lig = real && ((a.lm && a.lm[v] != 0.0f) || a.context[size_t(v) * a.ctx + a.ctx - 2] != 0.0f);
    const bool pock = real && a.context[size_t(v) * a.ctx + a.ctx - 1] != 0.0f;
    a.flags[v] = (real ? F_REAL : 0) | (lig ? F_LIG : 0) | (pock ? F_POCK : 0);
}

// edge predicate of get_dist_edges / get_dist_edges_4A (egnn.py:554-596), i != j, same molecule (pk_adjacent of egnn_sparse.hip)
__device__ __forceinline__ bool adjacent(int gt, int fi, int fj, float d2) {
    if (!(fi & F_REAL) || !(fj & F_REAL)) return false;
    if (gt == 0) return d2 <= 16.0f;
    const bool li = fi & F_LIG, lj = fj & F_LIG, pi = fi & F_POCK, pj = fj & F_POCK;
    const float cut2 = (gt == 1) ? 16.0f : 100.0f;
    return (li && lj) || (pi && pj && d2 <= 16.0f) || (((li && pj) || (pi && lj)) && d2 <= cut2);
}

// one wave per atom: count the neighbours (FILL = false) or write the list, senders in increasing order (FILL = true)
template <bool FILL>
__global__ void k_edges(int V, int N, int gt, const float* __restrict__ X, const int* __restrict__ flags,
                        int* __restrict__ deg, const int* __restrict__ off, int* __restrict__ col) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (v >= V) return;
    const int b = v / N;
    const int fi = flags[v];
    const float4 xi = *reinterpret_cast<const float4*>(X + 4 * size_t(v));
    int count = 0;
    const int base = FILL ? off[v] : 0;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int jn = j0 + lane;
        const int u = b * N + jn;
        bool adj = false;
        if (jn < N && u != v) {
            const float4 xj = *reinterpret_cast<const float4*>(X + 4 * size_t(u));
            const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            adj = adjacent(gt, fi, flags[u], dx * dx + dy * dy + dz * dz);
        }
        const unsigned long long bal = __ballot(adj);
        if (FILL && adj) col[base + count + __popcll(bal & ((1ull << lane) - 1ull))] = u;
        count += __popcll(bal);
    }
    if (!FILL && lane == 0) deg[v] = count;
}

// exclusive scan of deg[0..V) -> off[0..V] (single workgroup)
__global__ void k_scan(int V, const int* __restrict__ deg, int* __restrict__ off) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int per = (V + nth - 1) / nth;
    const int lo = min(tid * per, V), hi = min(lo + per, V);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += deg[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < nth; o <<= 1) {
        const int add = (tid >= o) ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = lo; i < hi; ++i) { off[i] = run; run += deg[i]; }
    if (tid == nth - 1) off[V] = part[tid];
}

// rev[e] for e = (v <- u): the slot of v in u's list (binary search: lists are sorted).  One wave per atom.
__global__ void k_rev(int V, const int* __restrict__ off, const int* __restrict__ col, int* __restrict__ rev) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (v >= V) return;
    for (int e = off[v] + lane; e < off[v + 1]; e += 64) {
        const int u = col[e];
        int lo = off[u], hi = off[u + 1] - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (col[mid] < v) lo = mid + 1; else hi = mid;
        }
        rev[e] = lo;
    }
}

// ---- node-level kernels ----------------------------------------------------------------------------------------------------
// out[v][c] = ((acc ? out : 0) + res + (bias[c] + sum_k W(c, k) f(in[v][k])) * dsilu(dact[v][c])) * nm[v], c < 128, k < K <= 128
//   W(c, k) = W[c * ld + col0 + k], transposed: W[k * ld + col0 + c];  f = SiLU when in_silu
struct LinArgs {
    float* out; const float* in; int ldi, K; const float* W; int ld, col0, trans; const float* bias; int acc;
    const float* res; const float* nm; const float* dact; int in_silu, V;
};

__global__ void __launch_bounds__(256) k_lin(LinArgs a) {
    __shared__ float Wl[H * WLD];
    __shared__ float inl[32 * H];
    const int tid = threadIdx.x, K = a.K, v0 = blockIdx.x * 32;
    for (int idx = tid; idx < K * H; idx += 256) {
        if (a.trans) { const int k = idx >> 7, c = idx & (H - 1); Wl[k * WLD + c] = a.W[size_t(k) * a.ld + a.col0 + c]; }
        else { const int c = idx / K, k = idx - c * K; Wl[k * WLD + c] = a.W[size_t(c) * a.ld + a.col0 + k]; }
    }
    for (int idx = tid; idx < 32 * K; idx += 256) {
        const int n = idx / K, k = idx - n * K, v = v0 + n;
        float x = v < a.V ? a.in[size_t(v) * a.ldi + k] : 0.0f;
        if (a.in_silu) x = silu(x);
        inl[n * K + k] = x;
    }
    __syncthreads();
    const int c = tid & (H - 1), half = tid >> 7;
    float s[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float w = Wl[k * WLD + c];
#pragma unroll
        for (int q = 0; q < 16; ++q) s[q] += w * inl[(half * 16 + q) * K + k];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int v = v0 + half * 16 + q;
        if (v >= a.V) break;
        const size_t at = size_t(v) * H + c;
        float val = s[q];
        if (a.bias) val += a.bias[c];
        if (a.dact) val *= dsilu(a.dact[at]);
        if (a.res) val += a.res[at];
        if (a.acc) val += a.out[at];
        if (a.nm) val *= a.nm[v];
        a.out[at] = val;
    }
}

// molecule b's slice: gW[o * ld + col0 + k] = sum_n G[n][o] f(In[n][k]), gb[o] = sum_n G[n][o]  (o < O, k < K <= 128), nodes in order
struct OuterArgs {
    const float* G; int ldg, O; const float* In; int ldi, K, in_silu; float* gp; long P, woff; int ld, col0; long boff; int N;
};

__global__ void __launch_bounds__(256) k_outer(OuterArgs a) {
    __shared__ float Gl[32 * 16];
    __shared__ float Il[32 * H];
    const int tid = threadIdx.x, b = blockIdx.x, o0 = blockIdx.y * 16, oo = tid >> 4, kk = tid & 15, K = a.K;
    float acc[8], gs = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
    for (int n0 = 0; n0 < a.N; n0 += 32) {
        __syncthreads();
        for (int idx = tid; idx < 32 * 16; idx += 256) {
            const int n = idx >> 4, o = o0 + (idx & 15);
            Gl[idx] = (n0 + n < a.N && o < a.O) ? a.G[(size_t(b) * a.N + n0 + n) * a.ldg + o] : 0.0f;
        }
        for (int idx = tid; idx < 32 * K; idx += 256) {
            const int n = idx / K, k = idx - n * K;
            float x = n0 + n < a.N ? a.In[(size_t(b) * a.N + n0 + n) * a.ldi + k] : 0.0f;
            if (a.in_silu) x = silu(x);
            Il[n * H + k] = x;
        }
        __syncthreads();
        for (int n = 0; n < 32; ++n) {
            const float g = Gl[n * 16 + oo];
            gs += g;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (kk + 16 * q < K) acc[q] += g * Il[n * H + kk + 16 * q];
        }
    }
    const int o = o0 + oo;
    if (o >= a.O) return;
    float* g = a.gp + size_t(b) * a.P;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (kk + 16 * q < K) g[a.woff + size_t(o) * a.ld + a.col0 + kk + 16 * q] = acc[q];
    if (a.boff >= 0 && kk == 0) g[a.boff + o] = gs;
}

// out = in * nm (out may alias in)
__global__ void k_mask(float* out, const float* in, const float* nm, size_t n) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = in[i] * nm[i >> 7];
}

// start of a block's backward: dh *= nm, dx *= nm, dxacc = 0
__global__ void k_blockprep(float* dh, float* dx, float* dxacc, const float* nm, size_t V) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < V * H) dh[i] *= nm[i >> 7];
    if (i < V * 4) { dx[i] *= nm[i >> 2]; dxacc[i] = 0.0f; }
}

__global__ void k_addx(float* dx, const float* dxacc, size_t n) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) dx[i] += dxacc[i];
}

// output layer: d velocity (mean removed with centering, utils.py:56-63) -> dx, d h_final -> du [V][MAX_FIN]; one workgroup per molecule
__global__ void __launch_bounds__(256) k_outprep(int N, int nf, int centering, const float* go_, const float* nm_, float* dx_, float* du_) {
    __shared__ float mean[3];
    const int b = blockIdx.x, tid = threadIdx.x, D = 3 + nf;
    const float* go = go_ + size_t(b) * N * D;
    const float* nm = nm_ + size_t(b) * N;
    float* dx = dx_ + size_t(b) * N * 4;
    float* du = du_ + size_t(b) * N * MAX_FIN;
    if (tid < 3) {
        float s = 0.0f, cnt = 0.0f;
        if (centering) {
            for (int n = 0; n < N; ++n) { s += nm[n] * go[size_t(n) * D + tid]; cnt += nm[n]; }
            s /= cnt;
        }
        mean[tid] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < N * 4; idx += 256) {
        const int n = idx >> 2, q = idx & 3;
        dx[idx] = q < 3 ? (go[size_t(n) * D + q] - mean[q]) * nm[n] : 0.0f;
    }
    for (int idx = tid; idx < N * MAX_FIN; idx += 256) {
        const int n = idx / MAX_FIN, c = idx % MAX_FIN;
        du[idx] = c < nf ? go[size_t(n) * D + 3 + c] * nm[n] : 0.0f;
    }
}

// ---- receiver-side sums over the neighbour lists (fixed order) ---------------------------------------------------------------
__global__ void __launch_bounds__(H) k_gather_agg(const int* __restrict__ off, const float* __restrict__ eb, float inv_norm, float* __restrict__ agg) {
    const int v = blockIdx.x, c = threadIdx.x;
    float s = 0.0f;
    for (int e = off[v]; e < off[v + 1]; ++e) s += eb[size_t(e) * H + c];
    agg[size_t(v) * H + c] = s * inv_norm;
}

// S_v = sum over v's edges of dpre1, T_v = the same over the reverse edges (the edges v sends on)
__global__ void __launch_bounds__(2 * H) k_gather_st(const int* __restrict__ off, const int* __restrict__ rev, const float* __restrict__ eb,
                                                     float* __restrict__ si, float* __restrict__ tj) {
    const int v = blockIdx.x, c = threadIdx.x & (H - 1);
    const bool sender = threadIdx.x >= H;
    float s = 0.0f;
    for (int e = off[v]; e < off[v + 1]; ++e) s += eb[size_t(sender ? rev[e] : e) * H + c];
    (sender ? tj : si)[size_t(v) * H + c] = s;
}

// x_new = (x + sum_e ex[e] / norm * lm) * nm (egnn.py:101-125)
__global__ void k_xupdate(int V, const int* __restrict__ off, const float* __restrict__ ex, const float* __restrict__ x, const float* __restrict__ lm,
                          const float* __restrict__ nm, float inv_norm, float* __restrict__ xn) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, v = gid >> 2, q = gid & 3;
    if (v >= V) return;
    float s = 0.0f;
    for (int e = off[v]; e < off[v + 1]; ++e) s += ex[size_t(e) * 4 + q];
    const float l = lm ? lm[v] : 1.0f;
    xn[gid] = q < 3 ? (x[gid] + s * inv_norm * l) * nm[v] : 0.0f;
}

// dxacc[v] += sum_e ex[e] - sum_e ex[rev e]  (diff = x_receiver - x_sender)
__global__ void k_gather_dx(int V, const int* __restrict__ off, const int* __restrict__ rev, const float* __restrict__ ex, float* __restrict__ dxacc) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, v = gid >> 2, q = gid & 3;
    if (v >= V) return;
    float s = 0.0f, r = 0.0f;
    for (int e = off[v]; e < off[v + 1]; ++e) { s += ex[size_t(e) * 4 + q]; r += ex[size_t(rev[e]) * 4 + q]; }
    dxacc[gid] += s - r;
}

// ---- the edge pass -----------------------------------------------------------------------------------------------------------
enum PassMode { GCL_FWD, COORD_FWD, GCL_BWD, COORD_BWD };

struct EdgeArgs {
    const float* P;                            // the MLP's parameters: W1 [H, 2H+2], b1, W2 [H, H], b2, (w3 [H])
    const float *wa, *wb;                      // [V][H]: W_a h + b1, W_b h
    const float *x, *x0;                       // [V][4]: the block's x, the input x
    const float* up;                           // GCL_BWD: d aggregate [V][H];  COORD_BWD: d x_new [V][4]
    const float* lm;                           // [V] or null
    const int *off, *col;
    float *eb, *ex, *ep;
    int N, G;
    float nc, inv_norm;
};

struct EdgeLds {
    float w[H * LDT];                          // W2[o][k]
    float p1[TE * LDT];                        // pre1, then dpre1
    float m1[TE * LDT];
    float t3[TE * LDT];                        // m2 (coordinate MLP), then dpre2
    float r[TE], d0[TE], s[TE], ds[TE], diff[TE * 4], cd[TE * 4], up[TE * 4], dd[TE * 4];
    float wr[H], w3[H];
    int row[TE], col[TE], moves[TE];
};

template <int MODE>
__global__ void __launch_bounds__(ET) k_edge(EdgeArgs a) {
    constexpr bool BWD = MODE == GCL_BWD || MODE == COORD_BWD;
    constexpr bool COORD = MODE == COORD_FWD || MODE == COORD_BWD;
    __shared__ __attribute__((aligned(16))) EdgeLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, hh = lane >> 5;
    const int b = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int e0 = a.off[size_t(b) * a.N], e1 = a.off[size_t(b + 1) * a.N];
    const int ntiles = (e1 - e0 + TE - 1) / TE;
    constexpr long ld1 = 2 * H + 2;
    const float* W1 = a.P;
    const float* W2 = a.P + long(H) * ld1 + H;
    const float* b2 = W2 + long(H) * H;
    const float* w3 = b2 + H;
    for (int idx = tid; idx < H * H; idx += ET) L.w[(idx >> 7) * LDT + (idx & (H - 1))] = W2[idx];
    if (tid < H) {
        L.wr[tid] = W1[tid * ld1 + 2 * H];
        L.w3[tid] = COORD ? w3[tid] : 0.0f;
    }
    const int c128 = tid & (H - 1), half = tid >> 7;
    const float w_r = W1[c128 * ld1 + 2 * H], w_d = W1[c128 * ld1 + 2 * H + 1];
    const int oc = 32 * wv + c;                                  // the output column this lane owns in the pre2 / dm1 products
    const float b2c = b2[oc], w3c = COORD ? w3[oc] : 0.0f;
    floatx16 gw[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) gw[kb] = splat16(0.0f);
    float gb2 = 0.0f, gwr = 0.0f, gwd = 0.0f, gw3 = 0.0f;
    __syncthreads();

    for (int t = g; t < ntiles; t += a.G) {
        const int base = e0 + t * TE;
        const int nvalid = min(TE, e1 - base);
        if (tid < TE) {                                          // geometry of the tile's edges
            const int p = tid;
            int i = 0, j = 0, mv = 0;
            float r = 0.0f, d0 = 0.0f, df[3] = {0.0f, 0.0f, 0.0f}, cd[3] = {0.0f, 0.0f, 0.0f}, upc[3] = {0.0f, 0.0f, 0.0f};
            if (p < nvalid) {
                j = a.col[base + p];
                int lo = b * a.N, hi = (b + 1) * a.N - 1;        // the receiver: the atom whose list holds the slot
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (a.off[mid] <= base + p) lo = mid; else hi = mid - 1;
                }
                i = lo;
                float dd[3];
                for (int q = 0; q < 3; ++q) {
                    df[q] = a.x[size_t(i) * 4 + q] - a.x[size_t(j) * 4 + q];
                    dd[q] = a.x0[size_t(i) * 4 + q] - a.x0[size_t(j) * 4 + q];
                }
                r = df[0] * df[0] + df[1] * df[1] + df[2] * df[2];
                d0 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
                const float den = sqrtf(r + 1e-8f) + a.nc;
                for (int q = 0; q < 3; ++q) cd[q] = df[q] / den;
                const float lmi = a.lm ? a.lm[i] : 1.0f;
                mv = lmi != 0.0f;
                if (MODE == COORD_BWD)
                    for (int q = 0; q < 3; ++q) upc[q] = a.up[size_t(i) * 4 + q] * lmi * a.inv_norm;
            }
            L.row[p] = i; L.col[p] = j; L.moves[p] = mv; L.r[p] = r; L.d0[p] = d0;
            for (int q = 0; q < 3; ++q) { L.diff[p * 4 + q] = df[q]; L.cd[p * 4 + q] = cd[q]; L.up[p * 4 + q] = upc[q]; L.dd[p * 4 + q] = 0.0f; }
        }
        __syncthreads();
        if (COORD) {                                             // only receivers in the linker mask move (egnn.py:113-116)
            int any = 0;
            for (int p = 0; p < TE; ++p) any |= L.moves[p];
            if (!any) {                                          // the tile's results are exact zeros
                if (MODE == COORD_BWD)
                    for (int idx = tid; idx < nvalid * H; idx += ET) a.eb[size_t(base) * H + idx] = 0.0f;
                for (int idx = tid; idx < nvalid * 4; idx += ET) a.ex[size_t(base) * 4 + idx] = 0.0f;
                __syncthreads();
                continue;
            }
        }
        // first layer: pre1 = (W_a h_i + b1) + W_b h_j + w_r r + w_d d0
        for (int p = half * 16; p < half * 16 + 16; ++p) {
            float v = 0.0f, m = 0.0f;
            if (p < nvalid) {
                v = a.wa[size_t(L.row[p]) * H + c128] + a.wb[size_t(L.col[p]) * H + c128] + w_r * L.r[p] + w_d * L.d0[p];
                m = silu(v);
            }
            L.p1[p * LDT + c128] = v;
            L.m1[p * LDT + c128] = m;
        }
        __syncthreads();
        // pre2[e][o] = b2[o] + sum_k m1[e][k] W2[o][k]: wave wv owns o = 32 wv .. + 31, lane (c, hh) supplies k = 64 hh + s
        floatx16 acc = splat16(b2c);
        {
            const float4* ap = reinterpret_cast<const float4*>(&L.m1[c * LDT + 64 * hh]);
            const float4* bp = reinterpret_cast<const float4*>(&L.w[oc * LDT + 64 * hh]);
#pragma unroll
            for (int sg = 0; sg < 16; ++sg) {
                const float4 av = ap[sg], bv = bp[sg];
                acc = mfma32(av.x, bv.x, acc);
                acc = mfma32(av.y, bv.y, acc);
                acc = mfma32(av.z, bv.z, acc);
                acc = mfma32(av.w, bv.w, acc);
            }
        }
        // accumulator register q holds edge p = (q & 3) + 8 (q >> 2) + 4 hh, column oc
        if (MODE == GCL_FWD) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = (q & 3) + 8 * (q >> 2) + 4 * hh;
                if (p < nvalid) a.eb[size_t(base + p) * H + oc] = silu(acc[q]);
            }
        } else if (MODE == GCL_BWD) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = (q & 3) + 8 * (q >> 2) + 4 * hh;
                L.t3[p * LDT + oc] = p < nvalid ? a.up[size_t(L.row[p]) * H + oc] * a.inv_norm * dsilu(acc[q]) : 0.0f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = (q & 3) + 8 * (q >> 2) + 4 * hh;
                L.t3[p * LDT + oc] = silu(acc[q]);
            }
            __syncthreads();
            {
                const int p = tid >> 3, part = tid & 7;          // s = w3 . m2: 8 threads per edge, 16 channels each
                float s = 0.0f;
                for (int k = part * 16; k < part * 16 + 16; ++k) s += L.w3[k] * L.t3[p * LDT + k];
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                if (part == 0) {
                    if (MODE == COORD_FWD) {
                        if (p < nvalid)
                            for (int q = 0; q < 4; ++q) a.ex[size_t(base + p) * 4 + q] = q < 3 ? L.cd[p * 4 + q] * s : 0.0f;
                    } else {
                        float dsv = 0.0f, dcd[3], dot = 0.0f;
                        for (int q = 0; q < 3; ++q) {
                            dsv += L.up[p * 4 + q] * L.cd[p * 4 + q];
                            dcd[q] = L.up[p * 4 + q] * s;
                        }
                        L.ds[p] = dsv;
                        // cd = diff / (sqrt(r + 1e-8) + nc): d diff = dcd / den - diff (dcd . diff) / (den^2 sqrt(r + 1e-8))
                        const float nr = sqrtf(L.r[p] + 1e-8f), den = nr + a.nc;
                        for (int q = 0; q < 3; ++q) dot += dcd[q] * L.diff[p * 4 + q];
                        for (int q = 0; q < 3; ++q) L.dd[p * 4 + q] = dcd[q] / den - L.diff[p * 4 + q] * dot / (den * den * nr);
                    }
                }
            }
            if (MODE == COORD_BWD) {
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int p = (q & 3) + 8 * (q >> 2) + 4 * hh;
                    const float dsp = L.ds[p];
                    gw3 += dsp * L.t3[p * LDT + oc];
                    L.t3[p * LDT + oc] = dsp * w3c * dsilu(acc[q]);      // dpre2 (this lane is the only reader and writer of the slot)
                }
            }
        }
        if (BWD) {
            __syncthreads();
            if (tid < H)
                for (int p = 0; p < TE; ++p) gb2 += L.t3[p * LDT + tid];
            // dW2[o][k] += sum_e dpre2[e][o] m1[e][k]: wave wv owns o = 32 wv .. + 31 (rows), four column blocks; lane supplies e = 16 hh + s
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int e = 16 * hh + s;
                const float av = L.t3[e * LDT + oc];
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) gw[kb] = mfma32(av, L.m1[e * LDT + 32 * kb + c], gw[kb]);
            }
            // dm1[e][k] = sum_o dpre2[e][o] W2[o][k]: wave wv owns k = 32 wv .. + 31, lane supplies o = 64 hh + s
            floatx16 dm = splat16(0.0f);
            {
                const float4* ap = reinterpret_cast<const float4*>(&L.t3[c * LDT + 64 * hh]);
#pragma unroll
                for (int sg = 0; sg < 16; ++sg) {
                    const float4 av = ap[sg];
                    const float* bp = &L.w[(64 * hh + 4 * sg) * LDT + oc];
                    dm = mfma32(av.x, bp[0], dm);
                    dm = mfma32(av.y, bp[LDT], dm);
                    dm = mfma32(av.z, bp[2 * LDT], dm);
                    dm = mfma32(av.w, bp[3 * LDT], dm);
                }
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int p = (q & 3) + 8 * (q >> 2) + 4 * hh;
                const float dp = dm[q] * dsilu(L.p1[p * LDT + oc]);     // invalid edges: dpre2 = 0, so dm = 0
                L.p1[p * LDT + oc] = dp;
                gwr += dp * L.r[p];
                gwd += dp * L.d0[p];
                if (p < nvalid) a.eb[size_t(base + p) * H + oc] = dp;
            }
            __syncthreads();
            {
                const int p = tid >> 3, part = tid & 7;          // dr = dpre1 . w_r
                float s = 0.0f;
                for (int k = part * 16; k < part * 16 + 16; ++k) s += L.p1[p * LDT + k] * L.wr[k];
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                if (part == 0 && p < nvalid)
                    for (int q = 0; q < 4; ++q)
                        a.ex[size_t(base + p) * 4 + q] = q < 3 ? L.dd[p * 4 + q] + 2.0f * L.diff[p * 4 + q] * s : 0.0f;
            }
        }
        __syncthreads();
    }
    if (!BWD) return;
    float* ep = a.ep + size_t(blockIdx.x) * EPS;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int o = 32 * wv + (q & 3) + 8 * (q >> 2) + 4 * hh;
            ep[o * H + 32 * kb + c] = gw[kb][q];
        }
    if (tid < H) ep[H * H + tid] = gb2;
    gwr += __shfl_xor(gwr, 32, 64);
    gwd += __shfl_xor(gwd, 32, 64);
    gw3 += __shfl_xor(gw3, 32, 64);
    if (hh == 0) {
        ep[H * H + H + oc] = gwr;
        ep[H * H + 2 * H + oc] = gwd;
        ep[H * H + 3 * H + oc] = gw3;
    }
}

// molecule b's slice of the pass's gradient: the sum of its G workgroup partials in order
__global__ void k_edge_reduce(const float* __restrict__ ep, int G, float* __restrict__ gp, long P, long poff, int coord) {
    const int b = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= EPS) return;
    float s = 0.0f;
    for (int g = 0; g < G; ++g) s += ep[(size_t(b) * G + g) * EPS + idx];
    constexpr long ld1 = 2 * H + 2, W2o = long(H) * ld1 + H;
    float* out = gp + size_t(b) * P + poff;
    if (idx < H * H) out[W2o + idx] = s;
    else if (idx < H * H + H) out[W2o + idx] = s;                                // b2 follows W2
    else if (idx < H * H + 2 * H) out[(idx - H * H - H) * ld1 + 2 * H] = s;
    else if (idx < H * H + 3 * H) out[(idx - H * H - 2 * H) * ld1 + 2 * H + 1] = s;
    else if (coord) out[W2o + long(H) * H + H + (idx - H * H - 3 * H)] = s;
}

__global__ void k_final_reduce(const float* __restrict__ gp, int B, long P, float* __restrict__ grad) {
    const long p = long(blockIdx.x) * 256 + threadIdx.x;
    if (p >= P) return;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s += gp[size_t(b) * P + p];
    grad[p] = s;
}

bool scope_ok(const dl_backward_args* a) {
    return a->hidden_nf == H && a->n_layers >= 1 && a->inv_sublayers >= 1 && a->inv_sublayers <= 4 && a->in_node_nf >= 1 &&
           3 + a->in_node_nf <= DMAX && a->context_node_nf >= 2 && (a->condition_time == 0 || a->condition_time == 1) &&
           a->in_node_nf + a->condition_time + a->context_node_nf <= MAX_FIN && a->normalization_factor != 0.0f;
}

bool size_ok(const dl_backward_args* a) {      // the edge slots are 32-bit
    return a->N <= PK_BWD_MAX_ATOMS && double(a->B) * a->N * a->N < 2147483647.0;
}

}  // namespace

extern "C" {

size_t dl_egnn_backward_pocket_workspace_bytes(const dl_backward_args* a, int32_t graph_type) {
    if (!a || !scope_ok(a) || graph_type < 0 || graph_type > 2 || a->B < 0 || a->N < 1 || !size_ok(a)) return 0;
    const long P = param_count(a->in_node_nf + a->condition_time + a->context_node_nf, a->n_layers, a->inv_sublayers);
    return ws_layout(a->B, a->N, a->n_layers, a->inv_sublayers, P).total * 4;
}

int32_t dl_egnn_backward_pocket(const dl_backward_args* a, int32_t graph_type, void* stream) {
    if (!a) return DL_ERR_BAD_ARG;
    if (!scope_ok(a)) return DL_ERR_UNSUPPORTED;
    if (graph_type < 0 || graph_type > 2 || a->B < 0 || a->N < 1) return DL_ERR_BAD_ARG;
    if (!size_ok(a)) return DL_ERR_TOO_MANY_ATOMS;
    const int fin = a->in_node_nf + a->condition_time + a->context_node_nf;
    const long P = param_count(fin, a->n_layers, a->inv_sublayers);
    if (a->n_params != P) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;
    if (!a->params || !a->xh || !a->node_mask || !a->context || !a->grad_out || !a->grad_params || !a->workspace)
        return DL_ERR_BAD_ARG;
    if (a->condition_time && !a->t) return DL_ERR_BAD_ARG;
    const int B = a->B, N = a->N, V = B * N, Lr = a->n_layers, S = a->inv_sublayers, G = groups_per_molecule(N);
    const Ws w = ws_layout(B, N, Lr, S, P);
    if (a->workspace_bytes < w.total * 4) return DL_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(a->workspace);
    int* wi = static_cast<int*>(a->workspace);
    const size_t vh = rnd64(size_t(V) * H), v4 = rnd64(size_t(V) * 4);
    auto HS = [&](int k, int s) { return ws + w.hs + vh * (size_t(k) * (S + 1) + s); };
    auto AG = [&](int k, int s) { return ws + w.ag + vh * (size_t(k) * S + s); };
    auto XS = [&](int k) { return ws + w.xs + v4 * k; };
    float *hin = ws + w.hin, *A = ws + w.a, *Bm = ws + w.bm, *U = ws + w.u, *DU = ws + w.du, *DH = ws + w.dh, *DH2 = ws + w.dh2,
          *DAGG = ws + w.dagg, *SI = ws + w.si, *TJ = ws + w.tj, *DX = ws + w.dx, *DXACC = ws + w.dxacc, *GP = ws + w.gp,
          *EP = ws + w.ep, *EB = ws + w.eb, *EX = ws + w.ex;
    int *flags = wi + w.flags, *deg = wi + w.deg, *off = wi + w.off, *col = wi + w.col, *rev = wi + w.rev;
    const float *nm = a->node_mask, *lm = a->linker_mask, *Pm = a->params;
    const Offs o = param_offsets(fin, S);
    const float inv_norm = 1.0f / a->normalization_factor;
    const unsigned vblocks = unsigned((size_t(V) * H + 255) / 256), row_tiles = unsigned((V + 31) / 32);

    auto lin = [&](float* out, const float* in, int ldi, int K, const float* W, int ld, int col0, bool trans, const float* bias,
                   bool acc, const float* res = nullptr, const float* mask = nullptr, const float* dact = nullptr, bool in_silu = false) {
        LinArgs l{out, in, ldi, K, W, ld, col0, trans ? 1 : 0, bias, acc ? 1 : 0, res, mask, dact, in_silu ? 1 : 0, V};
        hipLaunchKernelGGL(k_lin, dim3(row_tiles), dim3(256), 0, st, l);
    };
    auto outer = [&](const float* Gm, int ldg, int O, const float* In, int ldi, int K, bool in_silu, long woff, int ld, int col0, long boff) {
        OuterArgs q{Gm, ldg, O, In, ldi, K, in_silu ? 1 : 0, GP, P, woff, ld, col0, boff, N};
        hipLaunchKernelGGL(k_outer, dim3(B, (O + 15) / 16), dim3(256), 0, st, q);
    };
    auto edge = [&](int mode, const float* Pp, const float* x, const float* up) {
        EdgeArgs e{Pp, A, Bm, x, XS(0), up, lm, off, col, EB, EX, EP, N, G, a->norm_constant, inv_norm};
        const dim3 grid(B * G), blk(ET);
        if (mode == GCL_FWD) hipLaunchKernelGGL(k_edge<GCL_FWD>, grid, blk, 0, st, e);
        else if (mode == COORD_FWD) hipLaunchKernelGGL(k_edge<COORD_FWD>, grid, blk, 0, st, e);
        else if (mode == GCL_BWD) hipLaunchKernelGGL(k_edge<GCL_BWD>, grid, blk, 0, st, e);
        else hipLaunchKernelGGL(k_edge<COORD_BWD>, grid, blk, 0, st, e);
    };
    constexpr int ld1 = 2 * H + 2;
    // projections of the edge MLP's first layer: A = W_a h + b1, Bm = W_b h
    auto project = [&](const float* Pp, const float* h) {
        lin(A, h, H, H, Pp, ld1, 0, false, Pp + long(H) * ld1, false);
        lin(Bm, h, H, H, Pp, ld1, H, false, nullptr, false);
    };
    // after a backward edge pass: the pass's weight gradients and dh += W_a^T S + W_b^T T, dxacc += the x gradient
    auto edge_backward_tail = [&](const float* Pp, long poff, const float* h, float* dh, bool coord) {
        hipLaunchKernelGGL(k_edge_reduce, dim3((EPS + 255) / 256, B), dim3(256), 0, st, EP, G, GP, P, poff, coord ? 1 : 0);
        hipLaunchKernelGGL(k_gather_st, dim3(V), dim3(2 * H), 0, st, off, rev, EB, SI, TJ);
        hipLaunchKernelGGL(k_gather_dx, dim3((V * 4 + 255) / 256), dim3(256), 0, st, V, off, rev, EX, DXACC);
        outer(SI, H, H, h, H, H, false, poff, ld1, 0, poff + long(H) * ld1);
        outer(TJ, H, H, h, H, H, false, poff, ld1, H, -1);
        lin(dh, SI, H, H, Pp, ld1, 0, true, nullptr, true);
        lin(dh, TJ, H, H, Pp, ld1, H, true, nullptr, true);
    };

    // ---- inputs and graph
    {
        InitArgs i{V, N, a->in_node_nf, a->context_node_nf, a->condition_time, a->t_is_scalar, a->xh, a->t, nm, lm, a->context,
                   XS(0), hin, flags};
        hipLaunchKernelGGL(k_init, dim3((V + 255) / 256), dim3(256), 0, st, i);
        hipLaunchKernelGGL(k_edges<false>, dim3((V + 3) / 4), dim3(256), 0, st, V, N, graph_type, XS(0), flags, deg, off, col);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, V, deg, off);
        hipLaunchKernelGGL(k_edges<true>, dim3((V + 3) / 4), dim3(256), 0, st, V, N, graph_type, XS(0), flags, deg, off, col);
        hipLaunchKernelGGL(k_rev, dim3((V + 3) / 4), dim3(256), 0, st, V, off, col, rev);
    }
    // ---- forward with save (fp32)
    lin(HS(0, 0), hin, MAX_FIN, fin, Pm + o.emb_w, fin, 0, false, Pm + o.emb_b, false);
    for (int k = 0; k < Lr; ++k) {
        const float* blk = Pm + o.blk0 + o.blk_stride * k;
        for (int s = 0; s < S; ++s) {
            const float* g = blk + o.gcl_stride * s;
            const float* h = HS(k, s);
            project(g + G_E0W, h);
            edge(GCL_FWD, g + G_E0W, XS(k), nullptr);
            hipLaunchKernelGGL(k_gather_agg, dim3(V), dim3(H), 0, st, off, EB, inv_norm, AG(k, s));
            lin(U, h, H, H, g + G_N0W, 2 * H, 0, false, g + G_N0B, false);
            lin(U, AG(k, s), H, H, g + G_N0W, 2 * H, H, false, nullptr, true);
            lin(HS(k, s + 1), U, H, H, g + G_N2W, H, 0, false, g + G_N2B, false, h, nm, nullptr, true);   // (h + node_mlp) nm
        }
        project(blk + o.equiv, HS(k, S));
        edge(COORD_FWD, blk + o.equiv, XS(k), nullptr);
        hipLaunchKernelGGL(k_xupdate, dim3((V * 4 + 255) / 256), dim3(256), 0, st, V, off, EX, XS(k), lm, nm, inv_norm, XS(k + 1));
        hipLaunchKernelGGL(k_mask, dim3(vblocks), dim3(256), 0, st, k + 1 < Lr ? HS(k + 1, 0) : HS(Lr, 0), HS(k, S), nm, size_t(V) * H);
    }
    const float* hL = HS(Lr, 0);
    // ---- output layer and velocity (egnn.py:526-552)
    hipLaunchKernelGGL(k_outprep, dim3(B), dim3(256), 0, st, N, a->in_node_nf, a->centering, a->grad_out, nm, DX, DU);
    outer(DU, MAX_FIN, fin, hL, H, H, false, o.out_w, H, 0, o.out_b);
    lin(DH, DU, MAX_FIN, fin, Pm + o.out_w, H, 0, true, nullptr, false);
    // ---- blocks in reverse
    for (int k = Lr - 1; k >= 0; --k) {
        const float* blk = Pm + o.blk0 + o.blk_stride * k;
        const long gblk = o.blk0 + o.blk_stride * k;
        hipLaunchKernelGGL(k_blockprep, dim3(vblocks), dim3(256), 0, st, DH, DX, DXACC, nm, size_t(V));
        project(blk + o.equiv, HS(k, S));
        edge(COORD_BWD, blk + o.equiv, XS(k), DX);
        edge_backward_tail(blk + o.equiv, gblk + o.equiv, HS(k, S), DH, true);
        for (int s = S - 1; s >= 0; --s) {
            const float* g = blk + o.gcl_stride * s;
            const long gg = gblk + o.gcl_stride * s;
            const float* h = HS(k, s);
            const float* agg = AG(k, s);
            lin(U, h, H, H, g + G_N0W, 2 * H, 0, false, g + G_N0B, false);
            lin(U, agg, H, H, g + G_N0W, 2 * H, H, false, nullptr, true);
            hipLaunchKernelGGL(k_mask, dim3(vblocks), dim3(256), 0, st, DH, DH, nm, size_t(V) * H);        // h' = (h + node_mlp) nm
            outer(DH, H, H, U, H, H, true, gg + G_N2W, H, 0, gg + G_N2B);
            lin(DU, DH, H, H, g + G_N2W, H, 0, true, nullptr, false, nullptr, nullptr, U);               // d pre-activation
            outer(DU, H, H, h, H, H, false, gg + G_N0W, 2 * H, 0, gg + G_N0B);
            outer(DU, H, H, agg, H, H, false, gg + G_N0W, 2 * H, H, -1);
            lin(DH2, DU, H, H, g + G_N0W, 2 * H, 0, true, nullptr, false, DH);                           // residual + W_h^T du
            lin(DAGG, DU, H, H, g + G_N0W, 2 * H, H, true, nullptr, false);
            project(g + G_E0W, h);
            edge(GCL_BWD, g + G_E0W, XS(k), DAGG);
            edge_backward_tail(g + G_E0W, gg + G_E0W, h, DH2, false);
            float* tmp = DH; DH = DH2; DH2 = tmp;
        }
        hipLaunchKernelGGL(k_addx, dim3((V * 4 + 255) / 256), dim3(256), 0, st, DX, DXACC, size_t(V) * 4);
    }
    // ---- embedding (no mask on its output, egnn.py:223)
    outer(DH, H, H, hin, MAX_FIN, fin, false, o.emb_w, fin, 0, o.emb_b);
    hipLaunchKernelGGL(k_final_reduce, dim3(unsigned((P + 255) / 256)), dim3(256), 0, st, GP, B, P, a->grad_params);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
