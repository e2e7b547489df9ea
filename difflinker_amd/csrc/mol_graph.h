// mol_graph.h — what the kernels that read a perceived bond list with 256 threads per molecule share (mol_keys.hip,
// fingerprint.hip): the 64-bit mixing function of the colour refinement, the workgroup scan that numbers the real rows, and
// the test that says whether a list entry is a bond.  The definitions are quoted in include/difflinker_hip.h.
#pragma once
#include "pack_layout.h"

namespace {

using u64 = uint64_t;

constexpr int KT = 256;                          // threads per molecule
constexpr int KW = KT / 64;                      // waves

constexpr u64 SEED_COLOUR = 0x243F6A8885A308D3ull, SEED_KEY = 0x13198A2E03707344ull, MIX_B = 0xD6E8FEB86659FD93ull;

__device__ __forceinline__ u64 mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u64 mix2(u64 a, u64 b) { return mix64(a + b * MIX_B); }

// exclusive prefix sum of one int per thread over the workgroup; returns the total through `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds /* [KW] */, int& total) {
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
    for (int k = 0; k < KW; ++k) {
        if (k < w) base += lds[k];
        sum += lds[k];
    }
    __syncthreads();
    total = sum;
    return base + incl - v;
}

__device__ __forceinline__ int block_sum(int v, int* lds) {
    int total = 0;
    block_exclusive_scan(v, lds, total);
    return total;
}

struct Bond {
    int i, j, order;
};

// entry e of the list: a bond of this molecule (0 <= i, j < n, i != j, order 1..3)?  `bad` collects the entries that are not.
__device__ __forceinline__ bool load_bond(const int* list, int e, int n, Bond& bd, int& bad) {
    bd.i = list[e * 3];
    bd.j = list[e * 3 + 1];
    bd.order = list[e * 3 + 2];
    const bool ok = bd.i >= 0 && bd.j >= 0 && bd.i < n && bd.j < n && bd.i != bd.j && bd.order >= 1 && bd.order <= 3;
    bad |= !ok;
    return ok;
}

}  // namespace
