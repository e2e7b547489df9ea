// pocket.hip — the pocket of a ligand in its protein: every protein atom whose GROUP (its residue, as the host numbers it)
// holds an atom within `cutoff` of some ligand atom.  What the reference asks of Bio.PDB and numpy once per ligand in
// data/pocket/prepare_dataset.py::get_pocket, asked of a whole batch of (ligand, protein) pairs in one launch.
//
// THE RULE.  Proteins are concatenated: protein p owns the atoms protein_offset[p] .. protein_offset[p + 1] of protein_x (fp32,
// as Bio.PDB keeps them) and protein_group (dense ids 0 .. G_p - 1 within its protein, given by the host: the residue number
// alone for the reference's rule, or chain + number + insertion code).  Pair b is the protein pair_protein[b] and the ligand
// rows i with ligand_mask[b, i] != 0 (fp64, as the SDF's decimals are kept); rows with mask 0 are never read.  For protein
// atom j and ligand atom i
//     dx = (double)xp - xl (dy, dz alike),   d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
// every operation a separate fp64 round-to-nearest operation in exactly this order: contraction is OFF for this file.  Atom j is
// a CONTACT atom when d2 <= cutoff * cutoff for some i (one fp64 multiply, the comparison NOT strict), a group is SELECTED when
// it holds a contact atom, and atom j is a POCKET atom when its group is selected.  Every output is a flag, a count or a
// position: the same bits on every run and under every mapping.  get_pocket compares sqrt(d2) <= cutoff; the two forms can
// differ only for a pair within one rounding of the cutoff.
//
// THE MAPPING.  One 256-thread workgroup per pair, ONE launch per batch; the protein is streamed twice, so its size has no limit.
//   stage    the real ligand rows are counted (thread t owns a contiguous run of rows; a block scan gives its first slot) and go
//            to LDS as fp64, at most DL_POCKET_MAX_LIGAND = 256 of them (6 KiB); the selected-group set is a bitset of
//            DL_POCKET_MAX_GROUPS = 32768 bits in LDS (4 KiB), cleared here
//   pass 1   tiles of 256 atoms, one per thread: the thread walks the ligand in LDS (every lane reads the same entry: a
//            broadcast) and leaves at the first contact; a contact atom ORs its group's bit into the set (an LDS integer OR: the
//            order does not matter) and its contact flag goes to `member`
//   pass 2   the same tiles, the same thread per atom: the flag it wrote comes back, the group's bit makes bit 1, `member` is
//            written and the pocket atoms of the tile are numbered in file order by a block prefix scan for `index`
// A pair that cannot be answered (DL_POCKET_TOO_LARGE, _BAD_PROTEIN, _TOO_MANY_GROUPS, _NONFINITE) gets dead outputs: counts 0
// (n_ligand stays), member 0, index -1.  _BAD_PROTEIN is what keeps every access inside the arrays: a protein number outside
// [0, P), offsets that do not ascend inside [0, M_total], or a protein larger than the row of `member`.
//
// LDS: 6 KiB ligand + 4 KiB bitset, static.  Global memory is written with plain vector stores only; no global atomics; every
// output element is written on every launch.
#include "workgroup.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_LIGAND = DL_POCKET_MAX_LIGAND;
constexpr int MAX_GROUPS = DL_POCKET_MAX_GROUPS;
constexpr int SET_WORDS = MAX_GROUPS / 32;
static_assert(MAX_LIGAND == WG && SET_WORDS % WG == 0, "one staged ligand atom per thread, whole words of the set per thread");

__global__ __launch_bounds__(WG) void pocket_select_kernel(dl_pocket_args a) {
    __shared__ double s_lig[MAX_LIGAND * 3];
    __shared__ unsigned int s_set[SET_WORDS];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = a.L, Mmax = a.Mmax, R = a.capacity;
    unsigned char* member = a.member + size_t(b) * Mmax;        // never written when Mmax == 0
    int* index = a.index + size_t(b) * R;                       // never written when R == 0

    // ---- stage: count the real ligand rows (thread t owns the rows [r0, r1))
    const Rows rows = own_rows(L);
    const int r0 = rows.r0, r1 = rows.r1;
    const float* mask = a.ligand_mask + size_t(b) * L;          // never read when L == 0
    int n_ligand = 0;
    int k = block_exclusive_scan(count_rows(rows, mask), s_scan, n_ligand);

    // which atoms are this pair's: every access below stays inside [0, M_total) and inside the row of `member`
    const int p = a.pair_protein[b];
    int first = 0, M = 0;
    int status = n_ligand > MAX_LIGAND ? DL_POCKET_TOO_LARGE : 0;                // uniform over the workgroup, like all of it
    if (!status) {
        if (p < 0 || p >= a.P) {
            status = DL_POCKET_BAD_PROTEIN;
        } else {
            first = a.protein_offset[p];
            const int end = a.protein_offset[p + 1];
            M = end - first;
            if (first < 0 || end < first || end > a.M_total || M > Mmax) status = DL_POCKET_BAD_PROTEIN;
        }
    }

    int n_contact = 0, n_groups = 0, n_pocket = 0;
    if (!status) {
        int bad = 0, bad_group = 0;
        const double* lig = a.ligand_x + size_t(b) * L * 3;
        for (int r = r0; r < r1; ++r) {
            if (mask[r] == 0.0f) continue;
            const double x = lig[3 * r], y = lig[3 * r + 1], z = lig[3 * r + 2];
            bad |= !(isfinite(x) && isfinite(y) && isfinite(z));
            s_lig[3 * k] = x;
            s_lig[3 * k + 1] = y;
            s_lig[3 * k + 2] = z;
            ++k;
        }
#pragma unroll
        for (int w = 0; w < SET_WORDS / WG; ++w) s_set[w * WG + tid] = 0u;
        __syncthreads();

        // ---- pass 1: contact atoms and the groups they select
        const double c2 = a.cutoff * a.cutoff;
        const float* px = a.protein_x + size_t(first) * 3;
        const int* group = a.protein_group + first;
        for (int j = tid; j < M; j += WG) {
            const float fx = px[3 * size_t(j)], fy = px[3 * size_t(j) + 1], fz = px[3 * size_t(j) + 2];
            const int g = group[j];
            const bool finite = isfinite(fx) && isfinite(fy) && isfinite(fz), known = g >= 0 && g < MAX_GROUPS;
            bad |= !finite;
            bad_group |= !known;
            bool contact = false;
            if (finite && known) {
                const double x = double(fx), y = double(fy), z = double(fz);
                for (int i = 0; i < n_ligand; ++i) {
                    const double dx = x - s_lig[3 * i], dy = y - s_lig[3 * i + 1], dz = z - s_lig[3 * i + 2];
                    const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);       // contraction is off: five roundings, in this order
                    if (d2 <= c2) { contact = true; break; }
                }
                if (contact) atomicOr(&s_set[g >> 5], 1u << (g & 31));
            }
            member[j] = contact ? 1 : 0;
            n_contact += contact;
        }
        if (__syncthreads_or(bad)) status |= DL_POCKET_NONFINITE;                // also the barrier between the passes
        if (__syncthreads_or(bad_group)) status |= DL_POCKET_TOO_MANY_GROUPS;
    }

    if (status) {                                // ---- dead outputs
        for (int j = tid; j < Mmax; j += WG) member[j] = 0;
        for (int q = tid; q < R; q += WG) index[q] = -1;
        n_contact = 0;
    } else {
        n_contact = block_sum(n_contact, s_scan);
#pragma unroll
        for (int w = 0; w < SET_WORDS / WG; ++w) n_groups += __popc(s_set[w * WG + tid]);
        n_groups = block_sum(n_groups, s_scan);

        // ---- pass 2: pocket atoms, numbered in file order (uniform trip count: the scan has barriers)
        const int* group = a.protein_group + first;
        for (int j0 = 0; j0 < M; j0 += WG) {
            const int j = j0 + tid;
            int pocket = 0;
            if (j < M) {
                const int g = group[j];                                          // 0 <= g < MAX_GROUPS: the pair is not dead
                pocket = (s_set[g >> 5] >> (g & 31)) & 1u;
                member[j] = (unsigned char)(member[j] | (pocket << 1));          // this thread's own store of pass 1 comes back
            }
            int tile = 0;
            const int slot = n_pocket + block_exclusive_scan(pocket, s_scan, tile);
            if (pocket && slot < R) index[slot] = j;
            n_pocket += tile;
        }
        for (int j = M + tid; j < Mmax; j += WG) member[j] = 0;
        for (int q = min(n_pocket, R) + tid; q < R; q += WG) index[q] = -1;
        if (n_pocket > R) status |= DL_POCKET_TRUNCATED;
    }
    if (tid == 0) {
        a.n_ligand[b] = n_ligand;
        a.n_contact_atoms[b] = n_contact;
        a.n_groups_selected[b] = n_groups;
        a.n_pocket[b] = n_pocket;
        a.status[b] = status;
    }
}

}  // namespace

extern "C" {

int32_t dl_pocket_select(const dl_pocket_args* a, void* stream) {
    if (!a || a->B < 0 || a->L < 0 || a->P < 0 || a->M_total < 0 || a->Mmax < 0 || a->capacity < 0 || !(a->cutoff >= 0.0))
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->protein_offset || !a->pair_protein || !a->n_ligand || !a->n_contact_atoms || !a->n_groups_selected || !a->n_pocket ||
        !a->status || (a->M_total > 0 && (!a->protein_x || !a->protein_group)) || (a->L > 0 && (!a->ligand_x || !a->ligand_mask)) ||
        (a->Mmax > 0 && !a->member) || (a->capacity > 0 && !a->index))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(pocket_select_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
