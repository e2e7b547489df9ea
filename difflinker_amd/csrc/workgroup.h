// workgroup.h — what every analysis kernel with one 256-thread workgroup per molecule (or pair) needs: the workgroup size, the
// scan and the reductions over one value per thread, the atom type of a one-hot row, the pm distance of the bond rule, and the rule that
// says which rows of a molecule a thread owns.  mol_graph.h adds what the kernels that read a bond list share.
//
// THE WORKGROUP FUNCTIONS (block_*) take `lds`, one word per wave (WG_WAVES words) of LDS that they alone use while they
// run; each has two barriers, the second after its last read of `lds`, so the same words can serve the next call at once;
// and each may only be called from uniform control flow: every thread of the workgroup calls it, or none.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/difflinker_hip.h"

namespace {

constexpr int WG = 256;                          // threads per workgroup
constexpr int WG_WAVES = WG / 64;                // waves

// exclusive prefix sum of one int per thread over the workgroup; `total` is the sum, the same in every thread
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds /* [WG_WAVES] */, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k) {
        if (k < w) base += lds[k];
        sum += lds[k];
    }
    __syncthreads();
    total = sum;
    return base + incl - v;
}

// sum of one int per thread over the workgroup, the same in every thread (a butterfly: fewer shuffles than the scan)
__device__ __forceinline__ int block_sum(int v, int* lds /* [WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k) s += lds[k];
    __syncthreads();
    return s;
}

// minimum of one int per thread over the workgroup, the same in every thread
__device__ __forceinline__ int block_min(int v, int* lds /* [WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = lds[0];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) s = min(s, lds[k]);
    __syncthreads();
    return s;
}

// maximum of one int per thread over the workgroup, the same in every thread
__device__ __forceinline__ int block_max(int v, int* lds /* [WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = lds[0];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) s = max(s, lds[k]);
    __syncthreads();
    return s;
}

// the same for floats.  `o < v ? o : v` and no fminf: the comparison decides what a NaN does (it never wins against the
// value a thread holds), and clash.hip's contract for non-finite coordinates is written against exactly this
__device__ __forceinline__ float block_min(float v, float* lds /* [WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = lds[0];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) m = lds[k] < m ? lds[k] : m;
    __syncthreads();
    return m;
}

// sum of one 64-bit integer per thread over the workgroup, the same in every thread (the fixed-point sums of interaction.hip)
__device__ __forceinline__ long long block_sum(long long v, long long* lds /* [WG_WAVES] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k) s += lds[k];
    __syncthreads();
    return s;
}

// The fp64 sum whose ORDER is part of a rule (relax.hip): the balanced tree over adjacent elements, T'[i] = T[2i] + T[2i+1].
// Within a wave that is the xor-butterfly with offsets 1, 2, 4 ... 32, because an fp addition gives the same bits with its
// operands exchanged; every lane ends with the tree's value.  (The integer sums above go 32 ... 1: their order is free.)
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// the tree over the workgroup's 256 values by thread: the waves' trees, then (w0 + w1) + (w2 + w3); the same in every thread
__device__ __forceinline__ double block_tree_sum(double v, double* lds /* [WG_WAVES] */) {
    v = wave_tree_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return s;
}

// maximum of one double per thread: `o > v ? o : v`, so a NaN never wins against the value a thread holds
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double block_max(double v, double* lds /* [WG_WAVES] */) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = lds[0];
#pragma unroll
    for (int k = 1; k < WG_WAVES; ++k) m = lds[k] > m ? lds[k] : m;
    __syncthreads();
    return m;
}

// an offset into a set of m rows, as the fingerprint kernels read every offset: clamped to [0, m]
__device__ __forceinline__ int clamp_offset(int v, int m) { return min(max(v, 0), m); }

// popcount(x) + acc in ONE instruction.  Written as `__popc(x) + acc` the compiler re-associates the 64 sums of a row into
// popcounts onto zero and a tree of three-operand adds: 2.5 W instructions per pair where 2 W do.
__device__ __forceinline__ unsigned popc_add(unsigned x, unsigned acc) {
    unsigned out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(x), "v"(acc));
    return out;
}

// the distance in pm that bond perception compares with its table (bonds.hip's rule `100 |x_i - x_j| < T`, strict): the one
// place the arithmetic is written, so that every kernel that asks "are these two bonded?" rounds as bonds.hip does
__device__ __forceinline__ float bond_distance_pm(float dx, float dy, float dz) {
    return 100.0f * sqrtf(dx * dx + dy * dy + dz * dz);
}

// the atom type of a one-hot row: the index of its FIRST largest entry (include/difflinker_hip.h quotes this rule for every
// entry point that reads one_hot)
__device__ __forceinline__ int first_maximum(const float* row, int nf) {
    int best = 0;
    float vmax = row[0];
    for (int c = 1; c < nf; ++c) {
        const float v = row[c];
        if (v > vmax) { vmax = v; best = c; }
    }
    return best;
}

// Thread t owns the contiguous rows [t * per, t * per + per) of a molecule's n_rows, per = ceil(n_rows / WG), cut off at
// n_rows: rows in row order fall to threads in thread order, so a scan over the threads' counts numbers them in row order
struct Rows {
    int per, r0, r1;
};

__device__ __forceinline__ Rows own_rows(int n_rows) {
    const int per = (n_rows + WG - 1) / WG;
    const int r0 = min(int(threadIdx.x) * per, n_rows);
    return {per, r0, min(r0 + per, n_rows)};
}

// how many of this thread's rows have mask != 0
__device__ __forceinline__ int count_rows(const Rows& rows, const float* mask) {
    int mine = 0;
    for (int r = rows.r0; r < rows.r1; ++r) mine += mask[r] != 0.0f;
    return mine;
}

}  // namespace
