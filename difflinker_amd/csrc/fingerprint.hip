// fingerprint.hip — set-level scores of sampled molecules: circular fingerprints of the bond graphs bonds.hip left on the
// device, and the nearest neighbour and mean Tanimoto similarity of every row of one fingerprint set among rows of another.
// Internal diversity, similarity to the true molecule and similarity to a training set are reductions of these two launches
// (metrics.compute_diversity).  The fingerprint is this project's own, NOT RDKit's Morgan fingerprint: the definitions are
// in include/difflinker_hip.h, tests/fingerprint_ref.py restates them.
//
// FINGERPRINTS.  One 256-thread workgroup per molecule, one launch per batch, the list read with the conventions of
// mol_keys.hip (mol_graph.h holds the shared code).  Everything is indexed by atom number (real rows, at most 1024):
//   stage   real rows numbered in row order; type | KEEP | CENTRE per atom
//   round   r = 0 .. radius: every kept centre ORs bit (colour mod n_bits) into the bit row in LDS; then, unless r is the
//           last round, the list is read once more from global memory: every kept entry adds mix2(colour[j], order) to
//           sum[i] and the mirror image to sum[j] with 64-bit LDS adds, and colour[i] = mix2(colour[i], sum[i])
//   store   the bit row, once, with plain stores
// LDS: 8 + 8 + 4 bytes per atom number (20 KiB) + the bit row.  The adds and the ORs commute: no order of the list and no
// order in which LDS atomics land can change a bit.
//
// TANIMOTO.  One lane per A row, its W words in registers (the kernel is a template on W); a workgroup of 256 lanes owns 256
// consecutive A rows and walks the groups that intersect them.  A group's B segment streams through an LDS tile of
// DL_TANIMOTO_TILE rows: 16-byte coalesced loads, the W / 4 lanes that staged a row sum its popcount with shuffles.  Then
// every lane walks the tile, all lanes reading the SAME address (an LDS broadcast, conflict-free, 128-bit reads): W ANDs and
// W popcounts-with-add per pair, a cross-multiplied compare, and, when sum_q20 is wanted, one unsigned division.  The walk
// takes two rows per turn in two register buffers, so that a row's reads are issued a row of arithmetic ahead of their use.
// Lanes of other groups run along masked.  Nothing is combined across lanes or workgroups: plain stores, no atomics.
#include "mol_graph.h"

namespace {

constexpr int FP_ROWS = 1024;                    // atom numbers a workgroup holds (N <= 1024)
constexpr int FP_MAX_TYPES = 16;
constexpr int FP_MAX_WORDS = 64;                 // 2048 bits
constexpr int FP_KEEP = 1 << 8, FP_CENTRE = 1 << 9;              // s_tk: type | flags

__global__ __launch_bounds__(WG) void fingerprints_kernel(dl_fingerprint_args a) {
    __shared__ u64 s_col[FP_ROWS];
    __shared__ u64 s_sum[FP_ROWS];
    __shared__ int s_tk[FP_ROWS];
    __shared__ unsigned s_bits[FP_MAX_WORDS];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, W = a.n_bits / 32;

    // ---- stage: number the real rows
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* centre = a.centre_mask ? a.centre_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;
    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, a.capacity);
    const int status_in = in.status, nb = in.nb;
    uint32_t* bits = a.bits + size_t(b) * W;

    if (n_kept > DL_FP_MAX_ATOMS) {              // uniform over the workgroup; the list is not looked at
        for (int w = tid; w < W; w += WG) bits[w] = 0;
        if (tid == 0) {
            a.n_on[b] = 0;
            a.n_atoms[b] = n_kept;
            a.n_centres[b] = 0;
            a.status[b] = status_in | DL_FP_TOO_LARGE;
        }
        return;
    }

    int mine_centres = 0;
    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int) {
        const bool is_centre = kept && !(centre && centre[r] == 0.0f);
        s_tk[k] = first_maximum(a.one_hot + (size_t(b) * N + r) * nf, nf) | (kept ? FP_KEEP : 0) | (is_centre ? FP_CENTRE : 0);
        mine_centres += is_centre;
    });
    if (tid < FP_MAX_WORDS) s_bits[tid] = 0;
    const int n_centres = block_sum(mine_centres, s_scan);       // its barriers also publish s_tk and the cleared bit row
    for (int i = tid; i < n; i += WG) {
        s_col[i] = (s_tk[i] & FP_KEEP) ? mix2(SEED_COLOUR, u64((s_tk[i] & 0xFF) + 1)) : 0;
        s_sum[i] = 0;
    }
    __syncthreads();

    const int* list = a.bonds + size_t(b) * a.capacity * 3;      // never dereferenced when nb is 0
    const unsigned bit_mask = unsigned(a.n_bits) - 1;            // n_bits is a power of two
    int bad = 0;
    Bond bd;
    for (int r = 0;; ++r) {
        for (int i = tid; i < n; i += WG)
            if (s_tk[i] & FP_CENTRE) {
                const unsigned bit = unsigned(s_col[i]) & bit_mask;
                atomicOr(&s_bits[bit >> 5], 1u << (bit & 31));
            }
        if (r == a.radius) break;
        for (int e = tid; e < nb; e += WG) {
            if (!load_bond(list, e, n, bd, bad) || !(s_tk[bd.i] & s_tk[bd.j] & FP_KEEP)) continue;
            atomicAdd(&s_sum[bd.i], mix2(s_col[bd.j], u64(bd.order)));
            atomicAdd(&s_sum[bd.j], mix2(s_col[bd.i], u64(bd.order)));
        }
        __syncthreads();
        for (int i = tid; i < n; i += WG) {
            if (s_tk[i] & FP_KEEP) s_col[i] = mix2(s_col[i], s_sum[i]);
            s_sum[i] = 0;
        }
        __syncthreads();
    }
    if (a.radius == 0) {                         // no round has looked at the list: one pass for the status bit alone
        for (int e = tid; e < nb; e += WG) load_bond(list, e, n, bd, bad);
    }
    bad = __syncthreads_or(bad);                 // also orders the ORs of the last round before the reads below

    int on = 0;
    for (int w = tid; w < W; w += WG) {
        const unsigned v = s_bits[w];
        bits[w] = v;
        on += __popc(v);
    }
    const int n_on = block_sum(on, s_scan);
    if (tid == 0) {
        a.n_on[b] = n_on;
        a.n_atoms[b] = n_kept;
        a.n_centres[b] = n_centres;
        a.status[b] = status_in | (bad ? DL_FP_BAD_BOND : 0);
    }
}

constexpr int TT = 256;                          // lanes = A rows per workgroup
constexpr int TILE = DL_TANIMOTO_TILE;

// (clamp_offset and popc_add: workgroup.h, shared with select.hip)

template <int W, bool SUM>
__global__ __launch_bounds__(TT) void tanimoto_kernel(dl_tanimoto_args a) {
    constexpr int Q = W / 4;                     // 16-byte pieces per row
    __shared__ uint4 s_tile[TILE * Q];
    __shared__ int s_pop[TILE];

    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * TT;
    const int rows_end = int(min((long long)a.Ma, row0 + TT));   // one past the workgroup's last row
    const bool real = row0 + tid < a.Ma;
    const int i = real ? int(row0 + tid) : 0;    // (a lane past the last row takes part in the staging only)

    unsigned av[W];
    int pa = 0;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.a_bits) + size_t(real ? i : 0) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const uint4 v = real ? src[q] : make_uint4(0, 0, 0, 0);
            av[4 * q] = v.x; av[4 * q + 1] = v.y; av[4 * q + 2] = v.z; av[4 * q + 3] = v.w;
            pa += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        }
    }

    int best = -1, pairs = 0;
    unsigned best_c = 0, best_u = 0, best_num = 0, best_den = 1;
    u64 sum = 0;

    // the first group that ends after the workgroup's first row (offsets do not decrease: bisection)
    int lo = 0, hi = a.G;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (clamp_offset(a.a_offsets[mid + 1], a.Ma) > row0) hi = mid; else lo = mid + 1;
    }
    const uint4* b4 = reinterpret_cast<const uint4*>(a.b_bits);
    for (int g = lo; g < a.G; ++g) {
        const int a_lo = clamp_offset(a.a_offsets[g], a.Ma), a_hi = clamp_offset(a.a_offsets[g + 1], a.Ma);
        if (a_lo >= rows_end) break;
        if (max(a_lo, int(row0)) >= min(a_hi, rows_end)) continue;                   // none of this workgroup's rows
        const int b_lo = clamp_offset(a.b_offsets[g], a.Mb), b_hi = clamp_offset(a.b_offsets[g + 1], a.Mb);
        const bool member = real && i >= a_lo && i < a_hi;
        for (int t = b_lo; t < b_hi; t += TILE) {
            const int rows = min(TILE, b_hi - t);
            __syncthreads();                     // the tile before this one has been walked
            for (int q = tid; q < rows * Q; q += TT) {                              // the Q lanes of a row enter together
                const uint4 v = b4[size_t(t) * Q + q];
                s_tile[q] = v;
                int p = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
#pragma unroll
                for (int off = 1; off < Q; off <<= 1) p += __shfl_xor(p, off, 64);
                if (q % Q == 0) s_pop[q / Q] = p;
            }
            __syncthreads();
            // Two rows per turn, in two register buffers: the reads of a row are issued a whole row of arithmetic before
            // their use, so that one wave per SIMD does not wait for the LDS.  Reads past the segment's last row stay inside
            // the tile (the index is clamped) and their row is masked.
            const auto fetch = [&](uint4 (&dst)[Q], int r) {
                const uint4* row = s_tile + min(r, TILE - 1) * Q;
#pragma unroll
                for (int q = 0; q < Q; ++q) dst[q] = row[q];
            };
            const auto score = [&](const uint4 (&v)[Q], int r) {
                unsigned c = 0, c1 = 0;          // two chains: a popcount never waits for the one before it
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    c = popc_add(av[4 * q] & v[q].x, c);
                    c1 = popc_add(av[4 * q + 1] & v[q].y, c1);
                    c = popc_add(av[4 * q + 2] & v[q].z, c);
                    c1 = popc_add(av[4 * q + 3] & v[q].w, c1);
                }
                c += c1;
                const unsigned u = unsigned(pa + s_pop[min(r, TILE - 1)]) - c;
                const int j = t + r;
                const bool candidate = member && r < rows && !(a.exclude_diagonal && j == i);
                const unsigned num = u ? c : 1u, den = u ? u : 1u;                  // two empty fingerprints are equal
                if (candidate) {
                    ++pairs;
                    if (best < 0 || num * best_den > best_num * den) {              // < 2^24: exact in 32 bits
                        best = j; best_c = c; best_u = u; best_num = num; best_den = den;
                    }
                    if (SUM) sum += u ? (c << 20) / u : (1u << 20);                 // c << 20 reaches 2^31: unsigned
                }
            };
            uint4 even[Q], odd[Q];
            fetch(even, 0);
            for (int r = 0; r < rows; r += 2) {
                fetch(odd, r + 1);
                score(even, r);
                fetch(even, r + 2);
                score(odd, r + 1);
            }
        }
    }
    if (real) {
        a.nn_index[i] = best;
        a.nn_common[i] = int(best_c);
        a.nn_union[i] = int(best_u);
        a.n_pairs[i] = pairs;
        if (SUM) a.sum_q20[i] = sum;
    }
}

template <int W>
void launch_tanimoto(const dl_tanimoto_args& a, hipStream_t stream) {
    const dim3 grid(unsigned((a.Ma + TT - 1) / TT)), block(TT);
    if (a.sum_q20) hipLaunchKernelGGL((tanimoto_kernel<W, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((tanimoto_kernel<W, false>), grid, block, 0, stream, a);
}

}  // namespace

extern "C" {

int32_t dl_fingerprints(const dl_fingerprint_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > FP_ROWS || a->nf < 1 || a->nf > FP_MAX_TYPES || a->capacity < 0) return DL_ERR_BAD_ARG;
    if (a->radius < 0 || a->radius > DL_FP_MAX_RADIUS || (a->n_bits != 512 && a->n_bits != 1024 && a->n_bits != 2048))
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->node_mask || !a->n_bonds_in || !a->status_in || !a->bits || !a->n_on || !a->n_atoms || !a->n_centres ||
        !a->status || (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(fingerprints_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_tanimoto_nearest(const dl_tanimoto_args* a) {
    if (!a || a->Ma < 0 || a->Mb < 0 || a->G < 0 || (a->W != 16 && a->W != 32 && a->W != 64)) return DL_ERR_BAD_ARG;
    if ((a->Ma > 0 && !a->a_bits) || (a->Mb > 0 && !a->b_bits) || (a->G > 0 && (!a->a_offsets || !a->b_offsets))) return DL_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(a->a_bits) | reinterpret_cast<uintptr_t>(a->b_bits)) & 15) return DL_ERR_BAD_ARG;
    if (a->Ma == 0) return DL_OK;
    if (!a->nn_index || !a->nn_common || !a->nn_union || !a->n_pairs) return DL_ERR_BAD_ARG;
    const hipStream_t stream = static_cast<hipStream_t>(a->stream);
    if (a->W == 16) launch_tanimoto<16>(*a, stream);
    else if (a->W == 32) launch_tanimoto<32>(*a, stream);
    else launch_tanimoto<64>(*a, stream);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
