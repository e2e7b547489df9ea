// bonds.hip — bond perception and a connectivity check for a whole sampled batch (reference build_xae_molecule /
// get_bond_order, src/molecule_builder.py:44-102, and the fragment count behind metrics.is_connected).
//
// One 256-thread workgroup per molecule, one launch per batch.  The rule, for every pair j < i of real atoms:
//   d = 100 |x_i - x_j| (pm, fp32);  order = 0;  if d < T[ti][tj][0] { order = 1; if d < T[..][1] { order = 2; if d < T[..][2]
//   order = 3 } }  with T the caller's table of upper bounds [nf][nf][3] (a negative entry = "no such order": it is never
//   undercut, so a missing single-bond length gives no bond and a missing double ends the nesting at the single).
// NaN / inf distances fail every `<`, so a non-finite coordinate bonds to nothing (status bit DL_BONDS_NONFINITE).
//
// LDS holds seven words per atom (N <= 1024: 28 KiB) and the table; nothing of size N * N exists anywhere, pair orders are
// recomputed where they are needed (three coordinates and one table row per pair, all from LDS).
//
//   stage   real atoms (node_mask != 0) are compacted in row order: atom k of the outputs is the k-th real row, as the
//           reference masks a molecule before it builds it.  type = first maximum of the one-hot row.
//   count   wave w takes rows i = w, w + 4, ...; lanes take j = lane, lane + 64, ... < i.  A 64-bit ballot gives the row's
//           bond count; the valence of i is a wave sum, the valence of j an integer LDS add (integer: order-independent).
//   scan    exclusive prefix sum of the row counts over the workgroup -> the row's first slot and n_bonds.
//   fill    the same walk again; a bond's slot is row offset + bonds before it in the row (ballot + popcount of the lower
//           lanes), so the list is in row-major (i, j) order, the order torch.nonzero(A) walks the reference's matrix.
//           Slots >= capacity are not written (status bit DL_BONDS_OVERFLOW; n_bonds is still the true count).
//   label   label[i] = i, then rounds of (a) every bonded pair lowers both labels to their minimum (integer LDS min) and
//           (b) label[i] = label[label[i]] (pointer jumping), until a workgroup-wide vote sees no change.  Labels only
//           fall and label[i] stays a member of i's component, so the fixed point is the smallest atom index of the
//           component whatever the order of the updates: the outputs have the same bits on every run.
//
// Global memory is written with plain vector stores only; no global atomics of any kind.
#include "workgroup.h"

namespace {

constexpr int MAX_ATOMS = 1024;
constexpr int MAX_TYPES = 16;                    // widest one-hot row / table edge

struct Mol {
    const float *x, *y, *z;
    const int* type;
    const float* table;
    int nf;
};

__device__ __forceinline__ int pair_order(const Mol& m, int i, int j) {
    const float d = bond_distance_pm(m.x[i] - m.x[j], m.y[i] - m.y[j], m.z[i] - m.z[j]);
    const float* t = m.table + (m.type[i] * m.nf + m.type[j]) * 3;
    int order = 0;
    if (d < t[0]) {
        order = 1;
        if (d < t[1]) {
            order = 2;
            if (d < t[2]) order = 3;
        }
    }
    return order;
}

__global__ __launch_bounds__(WG) void perceive_bonds_kernel(dl_bonds_args a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ float s_table[MAX_TYPES * MAX_TYPES * 3];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int N = a.N, nf = a.nf;
    float* s_x = reinterpret_cast<float*>(lds_raw);
    float* s_y = s_x + N;
    float* s_z = s_y + N;
    int* s_type = reinterpret_cast<int*>(s_z + N);
    int* s_first = s_type + N;                   // row counts, then the rows' first slots
    int* s_val = s_first + N;
    int* s_label = s_val + N;

    for (int k = tid; k < nf * nf * 3; k += WG) s_table[k] = a.table[k];

    // ---- stage: compact the real rows
    const Rows own = own_rows(N);
    const int per = own.per, r0 = own.r0;        // the scan below deals the atoms out the same way
    const float* mask = a.node_mask + size_t(b) * N;
    int n = 0;
    int k = block_exclusive_scan(count_rows(own, mask), s_scan, n);
    int bad = 0;
    for (int r = own.r0; r < own.r1; ++r) {
        if (mask[r] == 0.0f) continue;
        const float* xr = a.x + (size_t(b) * N + r) * 3;
        const float px = xr[0], py = xr[1], pz = xr[2];
        bad |= !(isfinite(px) && isfinite(py) && isfinite(pz));
        s_x[k] = px; s_y[k] = py; s_z[k] = pz;
        s_type[k] = first_maximum(a.one_hot + (size_t(b) * N + r) * nf, nf);
        ++k;
    }
    for (int i = tid; i < N; i += WG) { s_first[i] = 0; s_val[i] = 0; s_label[i] = i; }
    bad = __syncthreads_or(bad);

    const Mol m{s_x, s_y, s_z, s_type, s_table, nf};

    // ---- count: bonds of row i (j < i) and valences
    for (int i = w; i < n; i += WG_WAVES) {
        int cnt = 0, vi = 0;
        for (int j0 = 0; j0 < i; j0 += 64) {
            const int j = j0 + lane;
            const int order = j < i ? pair_order(m, i, j) : 0;
            cnt += __popcll(__ballot(order > 0));
            vi += order;
            if (order > 0) atomicAdd(&s_val[j], order);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) vi += __shfl_xor(vi, off, 64);
        if (lane == 0) {
            s_first[i] = cnt;
            if (vi) atomicAdd(&s_val[i], vi);
        }
    }
    __syncthreads();

    // ---- scan: first slot of every row
    int rows[(MAX_ATOMS + WG - 1) / WG];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < (MAX_ATOMS + WG - 1) / WG; ++q) {
        const int r = r0 + q;
        rows[q] = (q < per && r < n) ? s_first[r] : 0;
        sum += rows[q];
    }
    int n_bonds = 0;
    int slot = block_exclusive_scan(sum, s_scan, n_bonds);
#pragma unroll
    for (int q = 0; q < (MAX_ATOMS + WG - 1) / WG; ++q) {
        const int r = r0 + q;
        if (q < per && r < n) { s_first[r] = slot; slot += rows[q]; }
    }
    __syncthreads();

    // ---- fill: (i, j, order) in row-major order
    int* out = a.bonds + size_t(b) * a.capacity * 3;
    for (int i = w; i < n; i += WG_WAVES) {
        int at = s_first[i];
        for (int j0 = 0; j0 < i; j0 += 64) {
            const int j = j0 + lane;
            const int order = j < i ? pair_order(m, i, j) : 0;
            const unsigned long long hit = __ballot(order > 0);
            const int p = at + __popcll(hit & ((1ull << lane) - 1ull));
            if (order > 0 && p < a.capacity) { out[p * 3] = i; out[p * 3 + 1] = j; out[p * 3 + 2] = order; }
            at += __popcll(hit);
        }
    }

    // ---- label: smallest atom index of every component
    for (;;) {
        int changed = 0;
        for (int i = w; i < n; i += WG_WAVES) {
            for (int j0 = 0; j0 < i; j0 += 64) {
                const int j = j0 + lane;
                if (j < i && pair_order(m, i, j) > 0) {
                    const int li = s_label[i], lj = s_label[j];
                    if (li != lj) {
                        changed = 1;
                        atomicMin(li < lj ? &s_label[j] : &s_label[i], min(li, lj));
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += WG) {
            const int l = s_label[i], ll = s_label[l];
            if (ll != l) { s_label[i] = ll; changed = 1; }      // ll <= l: concurrent jumps only lower labels further
        }
        if (!__syncthreads_or(changed)) break;
    }

    int roots = 0;
    for (int i = tid; i < N; i += WG) {
        const bool real = i < n;
        a.valence[size_t(b) * N + i] = real ? s_val[i] : 0;
        a.component[size_t(b) * N + i] = real ? s_label[i] : -1;
        roots += real && s_label[i] == i;
    }
    const int n_comp = block_sum(roots, s_scan);
    if (tid == 0) {
        a.n_bonds[b] = n_bonds;
        a.n_components[b] = n_comp;
        a.status[b] = (n_bonds > a.capacity ? DL_BONDS_OVERFLOW : 0) | (bad ? DL_BONDS_NONFINITE : 0);
    }
}

size_t lds_bytes(int N) { return size_t(7) * N * sizeof(float); }

}  // namespace

extern "C" {

size_t dl_bonds_workspace_bytes(int32_t B, int32_t N) {
    (void)B; (void)N;
    return 0;                                    // every intermediate lives in LDS
}

int32_t dl_perceive_bonds(const dl_bonds_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ATOMS || a->nf < 1 || a->nf > MAX_TYPES || a->capacity < 0) return DL_ERR_BAD_ARG;
    if (a->table_len != a->nf * a->nf * 3) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->one_hot || !a->x || !a->node_mask || !a->table || !a->n_bonds || !a->valence || !a->n_components || !a->component ||
        !a->status || (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    if (a->workspace_bytes < dl_bonds_workspace_bytes(a->B, a->N)) return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(perceive_bonds_kernel, dim3(a->B), dim3(WG), lds_bytes(a->N), static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
