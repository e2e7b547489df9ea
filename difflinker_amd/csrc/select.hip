// select.hip — which few of a set of sampled molecules to look at: Taylor-Butina clusters (dl_tanimoto_cluster) and MaxMin
// diverse subsets (dl_tanimoto_pick) of every group of a fingerprint set, on the rows fingerprint.hip left on the device and
// with the similarity of its tanimoto_kernel (c / u in integers, compared by cross-multiplication).  Both rules are this
// project's own statements, with fixed tie rules: the definitions are in include/difflinker_hip.h, tests/select_ref.py
// restates them.
//
// Both are sequential-greedy: many rounds of "compare every row with one chosen row, then take an arg-extreme".  ONE 256-lane
// workgroup per group keeps the rounds on chip; lane t owns the rows t, t + 256, t + 512, ... of its group (at most 16), and
// a row's state lives in LDS, one word per row, read and written by its owner alone, so the state itself needs no barrier.
//
// CLUSTER.  Phase 1 counts every row's neighbours the way tanimoto_kernel scores pairs: the lane's own row in registers, the
// group's rows streamed through an LDS tile (16-byte coalesced loads, broadcast reads, two rows per turn in two register
// buffers), once per 256 own rows.  Phase 2 needs neither a sort nor an n x n matrix: a block arg-max of
// (n_neighbours, lowest index) over the unassigned rows, packed into one int, visits the rows in exactly the order the rule
// states; the centroid's row is broadcast through LDS and every lane tests its own unassigned rows against it, reading them
// from global memory (the set stays in L2: at most 1 MiB per group).  A centroid without neighbours skips the pass.
// LDS: the tile (TILE x W words, 32 KiB at W = 64) + 16 KiB of state.
//
// PICK.  The same loop with an arg-min: the state word of a row is m(i) as (c << 16) | u, the arg-min compares fractions
// exactly and carries (m, index) through the wave shuffles and four LDS words.  LDS: 16 KiB of state.
//
// Nothing is combined across workgroups; plain stores; every output element is written exactly once.
#include "workgroup.h"

namespace {

constexpr int TILE = DL_TANIMOTO_TILE;
constexpr int MAX_ROWS = DL_SELECT_MAX_ROWS;
constexpr int INDEX_BITS = 12;                   // a group-local row index
static_assert(MAX_ROWS == 1 << INDEX_BITS, "the arg-max key packs (n_neighbours, index) into 2 x 12 bits");
constexpr unsigned PICKED = 0xFFFFFFFFu;         // pick's state word of a picked row; no (c << 16) | u reaches it

// the first row of the first group and one past the last row of the last: the rows outside [first, last) are in no group
struct Span {
    int first, last;
};

__device__ __forceinline__ Span grouped_rows(const int32_t* offsets, int G, int M) {
    if (G == 0) return {M, M};
    return {clamp_offset(offsets[0], M), clamp_offset(offsets[G], M)};
}

// c = popcount(cv & row) and p = popcount(row) of one row in global memory
template <int W>
__device__ __forceinline__ void pair_counts(const unsigned (&cv)[W], const uint4* row, unsigned& c, unsigned& p) {
    unsigned c0 = 0, c1 = 0, p0 = 0, p1 = 0;     // two chains each: a popcount never waits for the one before it
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
        const uint4 v = row[q];
        c0 = popc_add(cv[4 * q] & v.x, c0);
        c1 = popc_add(cv[4 * q + 1] & v.y, c1);
        c0 = popc_add(cv[4 * q + 2] & v.z, c0);
        c1 = popc_add(cv[4 * q + 3] & v.w, c1);
        p0 = popc_add(v.x, p0);
        p1 = popc_add(v.y, p1);
        p0 = popc_add(v.z, p0);
        p1 = popc_add(v.w, p1);
    }
    c = c0 + c1;
    p = p0 + p1;
}

// Row `row` of the set into every lane's registers through `s_row`, and its popcount.  Uniform control flow only; one
// barrier.  The caller puts a barrier between the last use of the registers' source and the next call (the block reductions
// of both loops do).
template <int W>
__device__ __forceinline__ unsigned broadcast_row(const uint4* bits4, int row, uint4* s_row, unsigned (&cv)[W]) {
    constexpr int Q = W / 4;
    if (threadIdx.x < Q) s_row[threadIdx.x] = bits4[size_t(row) * Q + threadIdx.x];
    __syncthreads();
    unsigned p = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const uint4 v = s_row[q];                // every lane the same address: an LDS broadcast
        cv[4 * q] = v.x; cv[4 * q + 1] = v.y; cv[4 * q + 2] = v.z; cv[4 * q + 3] = v.w;
        p += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    return p;
}

template <int W>
__global__ __launch_bounds__(WG) void cluster_kernel(dl_cluster_args a) {
    constexpr int Q = W / 4;                     // 16-byte pieces per row
    __shared__ uint4 s_tile[TILE * Q];
    __shared__ int s_pop[TILE];
    __shared__ int s_nn[MAX_ROWS];               // n_neighbours of an unassigned row, -1 once it is assigned
    __shared__ uint4 s_row[Q];
    __shared__ int s_red[WG_WAVES];

    const int tid = threadIdx.x, g = blockIdx.x;
    if (g == 0) {                                // the rows in no group
        const Span span = grouped_rows(a.offsets, a.G, a.M);
        for (int i = tid; i < a.M; i += WG)
            if (i < span.first || i >= span.last) {
                a.cluster[i] = -1;
                a.centroid[i] = -1;
                a.n_neighbours[i] = 0;
            }
    }
    if (g >= a.G) return;                        // (G == 0: one workgroup for the rows alone)
    const int lo = clamp_offset(a.offsets[g], a.M), hi = clamp_offset(a.offsets[g + 1], a.M);
    const int n = max(hi - lo, 0);
    if (n > MAX_ROWS) {                          // uniform over the workgroup; the rows are not looked at
        for (int i = lo + tid; i < hi; i += WG) {
            a.cluster[i] = -1;
            a.centroid[i] = -1;
            a.n_neighbours[i] = 0;
        }
        if (tid == 0) {
            a.n_clusters[g] = 0;
            a.status[g] = DL_SELECT_TOO_LARGE;
        }
        return;
    }
    const uint4* bits4 = reinterpret_cast<const uint4*>(a.bits);
    const unsigned num = unsigned(a.num), den = unsigned(a.den);

    // ---- phase 1: n_neighbours, 256 own rows at a time
    for (int base = 0; base < n; base += WG) {
        const int il = base + tid;
        const bool real = il < n;
        unsigned av[W];
        int pa = 0;
        {
            const uint4* src = bits4 + size_t(lo + (real ? il : 0)) * Q;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const uint4 v = real ? src[q] : make_uint4(0, 0, 0, 0);
                av[4 * q] = v.x; av[4 * q + 1] = v.y; av[4 * q + 2] = v.z; av[4 * q + 3] = v.w;
                pa += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
            }
        }
        int nn = 0;
        for (int t = 0; t < n; t += TILE) {
            const int rows = min(TILE, n - t);
            __syncthreads();                     // the tile before this one has been walked
            for (int q = tid; q < rows * Q; q += WG) {                               // the Q lanes of a row enter together
                const uint4 v = bits4[size_t(lo + t) * Q + q];
                s_tile[q] = v;
                int p = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
#pragma unroll
                for (int off = 1; off < Q; off <<= 1) p += __shfl_xor(p, off, 64);
                if (q % Q == 0) s_pop[q / Q] = p;
            }
            __syncthreads();
            // as in tanimoto_kernel: two rows per turn in two register buffers; reads past the last row stay inside the tile
            // (the index is clamped) and their row is masked
            const auto fetch = [&](uint4 (&dst)[Q], int r) {
                const uint4* row = s_tile + min(r, TILE - 1) * Q;
#pragma unroll
                for (int q = 0; q < Q; ++q) dst[q] = row[q];
            };
            const auto count = [&](const uint4 (&v)[Q], int r) {
                unsigned c = 0, c1 = 0;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    c = popc_add(av[4 * q] & v[q].x, c);
                    c1 = popc_add(av[4 * q + 1] & v[q].y, c1);
                    c = popc_add(av[4 * q + 2] & v[q].z, c);
                    c1 = popc_add(av[4 * q + 3] & v[q].w, c1);
                }
                c += c1;
                const unsigned u = unsigned(pa + s_pop[min(r, TILE - 1)]) - c;
                // c * den and num * u stay below 2^28: exact in 32 bits.  u == 0 (c is 0 then) passes: two empty rows are neighbours
                nn += real && r < rows && t + r != il && c * den >= num * u;
            };
            uint4 even[Q], odd[Q];
            fetch(even, 0);
            for (int r = 0; r < rows; r += 2) {
                fetch(odd, r + 1);
                count(even, r);
                fetch(even, r + 2);
                count(odd, r + 1);
            }
        }
        if (real) {
            s_nn[il] = nn;
            a.n_neighbours[lo + il] = nn;
        }
    }

    // ---- phase 2: the unassigned row of the most neighbours, the lowest of equal ones, takes its unassigned neighbours
    int n_clusters = 0;
    for (;;) {
        int key = -1;
        for (int il = tid; il < n; il += WG) {
            const int s = s_nn[il];
            if (s >= 0) key = max(key, (s << INDEX_BITS) | (MAX_ROWS - 1 - il));
        }
        key = block_max(key, s_red);
        if (key < 0) break;                      // every row is assigned
        const int cl = MAX_ROWS - 1 - (key & (MAX_ROWS - 1)), centroid = lo + cl;
        const auto assign = [&](int il) {
            s_nn[il] = -1;
            a.cluster[lo + il] = n_clusters;
            a.centroid[lo + il] = centroid;
        };
        if (key >> INDEX_BITS) {                 // it has neighbours (uniform: the key is the same in every lane)
            unsigned cv[W];
            const unsigned pc = broadcast_row<W>(bits4, centroid, s_row, cv);
            for (int il = tid; il < n; il += WG) {
                if (s_nn[il] < 0) continue;
                unsigned c, p;
                pair_counts<W>(cv, bits4 + size_t(lo + il) * Q, c, p);
                const unsigned u = pc + p - c;
                if (il == cl || c * den >= num * u) assign(il);
            }
        } else if (tid == (cl & (WG - 1))) {     // a singleton: its owner alone
            assign(cl);
        }
        ++n_clusters;
    }
    if (tid == 0) {
        a.n_clusters[g] = n_clusters;
        a.status[g] = 0;
    }
}

// ---- pick

// is the fraction of state word x smaller than that of y?  (c << 16) | u, u == 0 counts as 1 / 1; products below 2^24
__device__ __forceinline__ bool fraction_less(unsigned x, unsigned y) {
    const unsigned cx = x >> 16, ux = x & 0xFFFF, cy = y >> 16, uy = y & 0xFFFF;
    const unsigned nx = ux ? cx : 1u, dx = ux ? ux : 1u, ny = uy ? cy : 1u, dy = uy ? uy : 1u;
    return nx * dy < ny * dx;
}

// does candidate (m, i) come before candidate (om, oi) in the arg-min: the smaller fraction, the lower index of equal ones;
// m == PICKED is no candidate
__device__ __forceinline__ bool comes_before(unsigned m, int i, unsigned om, int oi) {
    if (m == PICKED) return false;
    if (om == PICKED) return true;
    if (fraction_less(m, om)) return true;
    if (fraction_less(om, m)) return false;
    return i < oi;
}

// the arg-min of one candidate per thread over the workgroup, the same in every thread; `lds` as the block_* functions of
// workgroup.h take it, but 2 * WG_WAVES words
__device__ __forceinline__ void block_arg_min(unsigned& m, int& i, int* lds /* [2 * WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned om = __shfl_xor(m, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (comes_before(om, oi, m, i)) { m = om; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) {
        lds[threadIdx.x >> 6] = int(m);
        lds[WG_WAVES + (threadIdx.x >> 6)] = i;
    }
    __syncthreads();
    m = unsigned(lds[0]);
    i = lds[WG_WAVES];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) {
        const unsigned om = unsigned(lds[k]);
        const int oi = lds[WG_WAVES + k];
        if (comes_before(om, oi, m, i)) { m = om; i = oi; }
    }
    __syncthreads();
}

template <int W>
__global__ __launch_bounds__(WG) void pick_kernel(dl_pick_args a) {
    constexpr int Q = W / 4;
    __shared__ unsigned s_m[MAX_ROWS];           // m(i) of an unpicked row as (c << 16) | u; PICKED
    __shared__ uint4 s_row[Q];
    __shared__ int s_red[2 * WG_WAVES];

    const int tid = threadIdx.x, g = blockIdx.x, K = a.K;
    if (g == 0) {                                // the rows in no group
        const Span span = grouped_rows(a.offsets, a.G, a.M);
        for (int i = tid; i < a.M; i += WG)
            if (i < span.first || i >= span.last) a.pick_rank[i] = -1;
    }
    if (g >= a.G) return;
    const int lo = clamp_offset(a.offsets[g], a.M), hi = clamp_offset(a.offsets[g + 1], a.M);
    const int n = max(hi - lo, 0);
    int status = 0, pl = 0;                      // pl: the pick, group-local
    if (n > MAX_ROWS) {
        status = DL_SELECT_TOO_LARGE;
    } else if (n > 0 && a.first) {               // an empty group does not look at its first
        const int f = a.first[g];
        if (f < lo || f >= hi) status = DL_SELECT_BAD_FIRST;
        else pl = f - lo;
    }
    const int n_picks = status ? 0 : min(K, n);  // uniform over the workgroup
    int32_t* picks = a.picks + size_t(g) * K;
    int32_t* pick_common = a.pick_common + size_t(g) * K;
    int32_t* pick_union = a.pick_union + size_t(g) * K;
    for (int k = n_picks + tid; k < K; k += WG) {
        picks[k] = -1;
        pick_common[k] = -1;
        pick_union[k] = -1;
    }
    if (tid == 0) {
        a.n_picked[g] = n_picks;
        a.status[g] = status;
    }
    if (status) {
        for (int i = lo + tid; i < hi; i += WG) a.pick_rank[i] = -1;
        return;
    }
    const uint4* bits4 = reinterpret_cast<const uint4*>(a.bits);
    for (int il = tid; il < n; il += WG) s_m[il] = 0;            // not PICKED; the first round overwrites it

    for (int r = 0; r < n_picks; ++r) {
        unsigned m = PICKED;
        if (r > 0) {                             // the unpicked row of the smallest m(i), the lowest of equal ones
            int best = 0x7FFFFFFF;
            for (int il = tid; il < n; il += WG) {               // rising il: a strict comparison keeps the lowest
                const unsigned v = s_m[il];
                if (v != PICKED && (m == PICKED || fraction_less(v, m))) { m = v; best = il; }
            }
            block_arg_min(m, best, s_red);       // r < n: there is an unpicked row
            pl = best;
        }
        if (tid == 0) {
            picks[r] = lo + pl;
            pick_common[r] = r ? int(m >> 16) : -1;
            pick_union[r] = r ? int(m & 0xFFFF) : -1;
        }
        const bool last = r + 1 == n_picks;      // nothing reads m(i) after the last pick
        unsigned cv[W];
        unsigned pc = 0;
        if (!last) pc = broadcast_row<W>(bits4, lo + pl, s_row, cv);
        for (int il = tid; il < n; il += WG) {
            const unsigned old = s_m[il];
            if (old == PICKED) continue;
            if (il == pl) {
                s_m[il] = PICKED;
                a.pick_rank[lo + il] = r;
                continue;
            }
            if (last) continue;
            unsigned c, p;
            pair_counts<W>(cv, bits4 + size_t(lo + il) * Q, c, p);
            const unsigned now = (c << 16) | (pc + p - c);
            if (r == 0 || fraction_less(old, now)) s_m[il] = now;                    // of equal ones the earliest pick stays
        }
    }
    for (int il = tid; il < n; il += WG)
        if (s_m[il] != PICKED) a.pick_rank[lo + il] = -1;
}

bool bad_set(int M, int W, int G, const void* bits, const void* offsets) {
    if (M < 0 || G < 0 || (W != 16 && W != 32 && W != 64)) return true;
    if ((M > 0 && !bits) || (G > 0 && !offsets)) return true;
    return (reinterpret_cast<uintptr_t>(bits) & 15) != 0;
}

}  // namespace

extern "C" {

int32_t dl_tanimoto_cluster(const dl_cluster_args* a) {
    if (!a || bad_set(a->M, a->W, a->G, a->bits, a->offsets)) return DL_ERR_BAD_ARG;
    if (a->num < 1 || a->num > a->den || a->den > 65536) return DL_ERR_BAD_ARG;
    if (a->M == 0 && a->G == 0) return DL_OK;
    if ((a->M > 0 && (!a->cluster || !a->centroid || !a->n_neighbours)) || (a->G > 0 && (!a->n_clusters || !a->status)))
        return DL_ERR_BAD_ARG;
    const hipStream_t stream = static_cast<hipStream_t>(a->stream);
    const dim3 grid(unsigned(a->G > 0 ? a->G : 1)), block(WG);
    if (a->W == 16) hipLaunchKernelGGL(cluster_kernel<16>, grid, block, 0, stream, *a);
    else if (a->W == 32) hipLaunchKernelGGL(cluster_kernel<32>, grid, block, 0, stream, *a);
    else hipLaunchKernelGGL(cluster_kernel<64>, grid, block, 0, stream, *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_tanimoto_pick(const dl_pick_args* a) {
    if (!a || bad_set(a->M, a->W, a->G, a->bits, a->offsets)) return DL_ERR_BAD_ARG;
    if (a->K < 1 || a->K > DL_SELECT_MAX_ROWS) return DL_ERR_BAD_ARG;
    if (a->M == 0 && a->G == 0) return DL_OK;
    if ((a->M > 0 && !a->pick_rank) ||
        (a->G > 0 && (!a->picks || !a->pick_common || !a->pick_union || !a->n_picked || !a->status)))
        return DL_ERR_BAD_ARG;
    const hipStream_t stream = static_cast<hipStream_t>(a->stream);
    const dim3 grid(unsigned(a->G > 0 ? a->G : 1)), block(WG);
    if (a->W == 16) hipLaunchKernelGGL(pick_kernel<16>, grid, block, 0, stream, *a);
    else if (a->W == 32) hipLaunchKernelGGL(pick_kernel<32>, grid, block, 0, stream, *a);
    else hipLaunchKernelGGL(pick_kernel<64>, grid, block, 0, stream, *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
