// points.h — coordinates for the kernels that stage a molecule's kept atoms in LDS as fp32 and compute on them in fp64
// (pharmacophore.hip, hydrogens.hip, pose_checks.hip, stereo.hip; relax.hip keeps its state in fp64 and takes the arithmetic).  Every operation rounds once, in the order written: contraction is
// switched off HERE, because a kernel's own `#pragma clang fp contract(off)` stands after its includes and would come too
// late for `dot`.  That is also why none of this is in mol_graph.h, which integer-only kernels include.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// row r of xs ([rows,3]) becomes atom kk of s_x; returns whether a coordinate of it is NaN or infinite
__device__ __forceinline__ int stage_point(const float* xs, int r, float* s_x, int kk) {
    int bad = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float v = xs[size_t(r) * 3 + d];
        s_x[kk * 3 + d] = v;
        bad |= nonfinite(v);
    }
    return bad;
}

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 point(const float* xs, int atom) {
    return {double(xs[atom * 3]), double(xs[atom * 3 + 1]), double(xs[atom * 3 + 2])};
}
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

}  // namespace
