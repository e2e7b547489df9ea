// shape.hip — gridded van der Waals shape overlap of two molecules that share a frame: for every pair of a batch the volume
// of molecule A, of molecule B and of their intersection, counted on a 0.5 A lattice with two layers around every atom.  The
// reference scores this through RDKit (the shape half of calc_SC_RDKit.py:36-38, 1 - ShapeProtrudeDist); RDKit is absent here,
// so the RULE below is this project's own after RDKit's defaults (gridSpacing 0.5, vdwScale 0.8, stepSize 0.25, two bits per
// point, ignoreHs) - NOT RDKit's grid, and not its numbers.  It is stated in full in include/difflinker_hip.h;
// tests/shape_ref.py restates it in numpy float32 and gives the same integers.
//
// THE RULE in short.  Lattice points p = (0.5f*i, 0.5f*j, 0.5f*k), all integers i, j, k.  For a point and an atom of type t at
// (xa, ya, za):  dx = px - xa (dy, dz alike),  d2 = ((dx*dx) + (dy*dy)) + (dz*dz), every operation a separate fp32
// round-to-nearest operation in this order (contraction is OFF for this file), and the atom gives the point
//     (d2 < r2[t][0]) + (d2 < r2[t][1]) + (d2 < r2[t][2])            strict comparisons
// The LEVEL of a point for a molecule is the maximum of that over the molecule's participating atoms.  Outputs are sums over
// the lattice of level_A, level_B, min(level_A, level_B) and the counts of level == 3: integers that depend on no order.
//
// THE MAPPING.  One 256-thread workgroup per pair, ONE launch per batch.
//   look       every participating row of both molecules: finite?  |coordinate| <= 4096?  the lattice extent floor(2*min) ..
//              floor(2*max) per axis.  A flagged pair writes zeros and its status and is done.
//   bricks     the box (extent padded by E + 1 lattice steps, E = ceil(2 * r_max) + 1 over the table's largest radius) is
//              walked in BRICKS of 32 x 32 x 32 points.  A brick holds the thermometer code of both molecules' levels as six
//              BIT PLANES in LDS (level >= 1, >= 2, >= 3, for A and for B): word [z][y] of a plane, bit x.  24 KB.
//   rasterise  per brick and molecule the rows pass in chunks of 256: a thread takes one row, and the rows that take part and
//              reach the brick are compacted into an LDS list (block scan).  The work items are (atom, y, z) COLUMNS of the
//              atom's cube of (2E + 2)^2 columns, y fastest, dealt round-robin to the threads: neighbouring lanes hit
//              neighbouring words, hence different banks.  A column walks its <= 2E + 2 points along x, builds three bit masks
//              in registers and sets them with one LDS atomicOr per plane - an OR is order-free, so the planes are the same
//              bits on every run.  A column is left at once when (dy*dy) or (dz*dz) alone is not below the atom's largest r2:
//              fp32 addition of non-negative terms is monotone, so d2 >= (dy*dy) and d2 >= (dz*dz) hold exactly.
//   count      vol = sum_k popc(plane_k), vol_min = sum_k popc(A_k & B_k), core = popc(plane_3), core_both = popc(A_3 & B_3),
//              in the thread's registers over all bricks; the pass that counts a brick's words clears them for the next.
//   reduce     wave shuffles and one LDS step, as clash.hip sums; thread 0 writes the pair's nine integers.
//
// The bricks partition the lattice, every point of the padded box is in exactly one, and every point outside the box is at
// level 0 for both molecules; so the sums are the rule's, whatever the box.  Every brick index is clipped against the brick
// before LDS is touched: a table outside what the host wrapper admits (r2 not finite or above 400) can give wrong sums, never
// a write outside the planes.  Global memory is written with plain vector stores only, no global atomics; every output
// element is written; nothing is allocated.
#include "workgroup.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_TYPES = 16;
constexpr int BR = 32;                           // points per brick edge: one word of a plane holds a row along x
constexpr int PLANE = BR * BR;                   // words per plane
constexpr int E_MAX = 41;                        // reach of an atom in lattice steps at the largest admitted radius (20 A)
constexpr float COORD_MAX = 4096.0f;
constexpr int EXTENT_MAX = 240;

// the participating rows of one molecule: counts them, ORs the two coordinate flags, widens the lattice extent
__device__ __forceinline__ void look(const float* x, const float* mask, int n_rows, int& count, int& nonfinite, int& far,
                                     int (&lo)[3], int (&hi)[3]) {
    for (int r = threadIdx.x; r < n_rows; r += WG) {
        if (mask[r] == 0.0f) continue;
        ++count;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float c = x[3 * size_t(r) + d];
            if (!isfinite(c)) { nonfinite = 1; continue; }
            if (fabsf(c) > COORD_MAX) { far = 1; continue; }
            const int cell = int(floorf(2.0f * c));                      // exact: |2c| <= 8192
            lo[d] = min(lo[d], cell);
            hi[d] = max(hi[d], cell);
        }
    }
}

__global__ __launch_bounds__(WG) void shape_scores_kernel(dl_shape_args a) {
    __shared__ uint32_t s_plane[6 * PLANE];      // [molecule * 3 + (level - 1)][z][y], bit x
    __shared__ float4 s_atom[WG];                // the chunk's atoms that reach the brick: x, y, z, type
    __shared__ float s_r2[MAX_TYPES * 4];        // r2[t][0..2], and their largest
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int nf = a.nf;
    const float* xa = a.x_a + size_t(b) * a.Na * 3, * xb = a.x_b + size_t(b) * a.Nb * 3;
    const float* ha = a.one_hot_a + size_t(b) * a.Na * nf, * hb = a.one_hot_b + size_t(b) * a.Nb * nf;
    const float* ma = a.mask_a + size_t(b) * a.Na, * mb = a.mask_b + size_t(b) * a.Nb;

    // ---- look: counts, flags, extent
    int n_a = 0, n_b = 0, nonfinite = 0, far = 0;
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-INT32_MAX, -INT32_MAX, -INT32_MAX};
    look(xa, ma, a.Na, n_a, nonfinite, far, lo, hi);
    look(xb, mb, a.Nb, n_b, nonfinite, far, lo, hi);
    for (int k = tid; k < MAX_TYPES * 4; k += WG) {
        const int t = k >> 2, c = k & 3;
        float v = 0.0f;
        if (t < nf) {
            const float* r = a.r2 + 3 * t;
            v = c < 3 ? r[c] : fmaxf(fmaxf(r[0], r[1]), r[2]);
        }
        s_r2[k] = v;
    }
    nonfinite = __syncthreads_or(nonfinite);
    far = __syncthreads_or(far);
    n_a = block_sum(n_a, s_scan);
    n_b = block_sum(n_b, s_scan);
    int status = nonfinite ? DL_SHAPE_NONFINITE : far ? DL_SHAPE_OUT_OF_RANGE : 0;      // decided in this order
    if (!status && n_a + n_b > 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = block_min(lo[d], s_scan);
            hi[d] = -block_min(-hi[d], s_scan);
            if (hi[d] - lo[d] > EXTENT_MAX) status = DL_SHAPE_TOO_LARGE;
        }
    }

    int vol_a = 0, vol_b = 0, vol_min = 0, core_a = 0, core_b = 0, core_both = 0;
    if (!status && n_a + n_b > 0) {                                      // uniform over the workgroup
        float r2_top = 0.0f;
        for (int t = 0; t < nf; ++t) r2_top = fmaxf(r2_top, s_r2[4 * t + 3]);
        // reach of an atom in lattice steps, one step to spare for the roundings of d2 and of the root
        const int E = r2_top < 400.0f ? int(ceilf(2.0f * sqrtf(r2_top))) + 1 : E_MAX;
        const int D = 2 * E + 2;                                         // an atom's cube: cells c - E .. c + 1 + E, c = floor(2x)
        const int o[3] = {lo[0] - E - 1, lo[1] - E - 1, lo[2] - E - 1};  // the box starts here and ends at hi + 2 + E
        int nb[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) nb[d] = (hi[d] + 2 + E - o[d]) / BR + 1;

        for (int k = tid; k < 6 * PLANE; k += WG) s_plane[k] = 0u;
        __syncthreads();

        for (int bz = 0; bz < nb[2]; ++bz)
        for (int by = 0; by < nb[1]; ++by)
        for (int bx = 0; bx < nb[0]; ++bx) {
            const int ox = o[0] + bx * BR, oy = o[1] + by * BR, oz = o[2] + bz * BR;
            int touched = 0;
            for (int m = 0; m < 2; ++m) {
                uint32_t* plane = s_plane + m * 3 * PLANE;
                const float* xm = m ? xb : xa, * hm = m ? hb : ha, * mm = m ? mb : ma;
                const int n_rows = m ? a.Nb : a.Na;
                for (int r0 = 0; r0 < n_rows; r0 += WG) {
                    // ---- this chunk's rows that take part and reach the brick, compacted
                    const int r = r0 + tid;
                    float4 atom = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    int mine = 0;
                    if (r < n_rows && mm[r] != 0.0f) {
                        atom.x = xm[3 * size_t(r)];
                        atom.y = xm[3 * size_t(r) + 1];
                        atom.z = xm[3 * size_t(r) + 2];
                        const int cx = int(floorf(2.0f * atom.x)), cy = int(floorf(2.0f * atom.y)), cz = int(floorf(2.0f * atom.z));
                        mine = cx + 1 + E >= ox && cx - E < ox + BR && cy + 1 + E >= oy && cy - E < oy + BR &&
                               cz + 1 + E >= oz && cz - E < oz + BR;
                        if (mine) atom.w = __int_as_float(first_maximum(hm + size_t(r) * nf, nf));
                    }
                    int n_here = 0;
                    const int slot = block_exclusive_scan(mine, s_scan, n_here);    // its barriers also close the last chunk's reads
                    if (n_here == 0) continue;                                      // uniform
                    if (mine) s_atom[slot] = atom;
                    __syncthreads();
                    touched = 1;

                    // ---- the columns of these atoms' cubes: item = (atom, z, y), y fastest
                    const int items = n_here * D * D;
                    for (int w = tid; w < items; w += WG) {
                        const int at = w / (D * D), rem = w - at * (D * D);
                        const int kk = rem / D, jj = rem - kk * D;
                        const float4 q = s_atom[at];
                        const int j = int(floorf(2.0f * q.y)) - E + jj, k = int(floorf(2.0f * q.z)) - E + kk;
                        if (j < oy || j >= oy + BR || k < oz || k >= oz + BR) continue;
                        const int t = __float_as_int(q.w);
                        const float ra = s_r2[4 * t], rb = s_r2[4 * t + 1], rc = s_r2[4 * t + 2], rtop = s_r2[4 * t + 3];
                        const float dy = 0.5f * float(j) - q.y, dz = 0.5f * float(k) - q.z;
                        const float dy2 = dy * dy, dz2 = dz * dz;
                        if (!(dy2 < rtop) || !(dz2 < rtop)) continue;                // d2 >= dy2 and d2 >= dz2, exactly
                        const int cx = int(floorf(2.0f * q.x));
                        const int i0 = max(cx - E, ox), i1 = min(cx + 1 + E, ox + BR - 1);
                        uint32_t m1 = 0u, m2 = 0u, m3 = 0u;
                        for (int i = i0; i <= i1; ++i) {
                            const float dx = 0.5f * float(i) - q.x;
                            const float d2 = ((dx * dx) + dy2) + dz2;               // contraction is off: one rounding each
                            const int level = (d2 < ra) + (d2 < rb) + (d2 < rc);
                            const uint32_t bit = 1u << (i - ox);
                            if (level >= 1) m1 |= bit;
                            if (level >= 2) m2 |= bit;
                            if (level >= 3) m3 |= bit;
                        }
                        const int word = (k - oz) * BR + (j - oy);
                        if (m1) atomicOr(plane + word, m1);
                        if (m2) atomicOr(plane + PLANE + word, m2);
                        if (m3) atomicOr(plane + 2 * PLANE + word, m3);
                    }
                }
            }
            __syncthreads();                                             // every OR of this brick has landed
            if (!touched) continue;                                      // uniform; the planes are still clear
            // ---- count the brick and clear it for the next
            for (int w = tid; w < PLANE; w += WG) {
                const uint32_t a1 = s_plane[w], a2 = s_plane[PLANE + w], a3 = s_plane[2 * PLANE + w];
                const uint32_t b1 = s_plane[3 * PLANE + w], b2 = s_plane[4 * PLANE + w], b3 = s_plane[5 * PLANE + w];
                vol_a += __popc(a1) + __popc(a2) + __popc(a3);
                vol_b += __popc(b1) + __popc(b2) + __popc(b3);
                vol_min += __popc(a1 & b1) + __popc(a2 & b2) + __popc(a3 & b3);
                core_a += __popc(a3);
                core_b += __popc(b3);
                core_both += __popc(a3 & b3);
#pragma unroll
                for (int p = 0; p < 6; ++p) s_plane[p * PLANE + w] = 0u;
            }
            __syncthreads();
        }
    }

    vol_a = block_sum(vol_a, s_scan);
    vol_b = block_sum(vol_b, s_scan);
    vol_min = block_sum(vol_min, s_scan);
    core_a = block_sum(core_a, s_scan);
    core_b = block_sum(core_b, s_scan);
    core_both = block_sum(core_both, s_scan);
    if (tid == 0) {
        a.vol_a[b] = vol_a;
        a.vol_b[b] = vol_b;
        a.vol_min[b] = vol_min;
        a.core_a[b] = core_a;
        a.core_b[b] = core_b;
        a.core_both[b] = core_both;
        a.n_a[b] = status ? 0 : n_a;
        a.n_b[b] = status ? 0 : n_b;
        a.status[b] = status;
    }
}

}  // namespace

extern "C" {

int32_t dl_shape_scores(const dl_shape_args* a, void* stream) {
    if (!a || a->B < 0 || a->Na < 1 || a->Nb < 1 || a->nf < 1 || a->nf > MAX_TYPES) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x_a || !a->one_hot_a || !a->mask_a || !a->x_b || !a->one_hot_b || !a->mask_b || !a->r2 || !a->vol_a || !a->vol_b ||
        !a->vol_min || !a->core_a || !a->core_b || !a->core_both || !a->n_a || !a->n_b || !a->status)
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(shape_scores_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
