// pharmacophore.hip — pharmacophore features of the bond graphs bonds.hip and aromatic.hip left on the device, and the
// Best-mode feature-map match of two feature lists: the feature half of SC-RDKit.  The rule is this project's own, after
// RDKit's BaseFeatures.fdef and the FeatMapParams defaults; it is stated in full in include/difflinker_hip.h and restated in
// tests/pharmacophore_ref.py, and it is NOT RDKit's feature factory and NOT RDKit's numbers.
//
// dl_pharmacophore_features: one 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h.
//
//   stage    rows ranked by number_rows; class, default valence, mark, atom number and coordinates of the kept atoms go to
//            LDS by kept index
//   build    four 256 x 256 bit matrices over the kept atoms: the pairs, the pairs of order 2, of order 3, and the aromatic
//            pairs (the two passes of mol_graph.h): the first entry of a pair alone gives it its order and its aromatic flag
//   atoms    thread u owns kept atom u: one pass over its four rows gives deg, val, h, arom and multi; a ballot per wave
//            writes the 256-bit sets (classes, arom, multi, terminal oxygens) that the neighbour tests AND a row with
//   rings    thread s walks the aromatic pairs from atom s over larger atoms with two or three aromatic pairs, at most six
//            deep and at most 3 * 2^4 leaves, and closes chordless cycles of 5 and 6 atoms in canonical order (an LDS counter
//            hands out slots); at most 64 rings are then ranked by their atom sequence, 64 x 64 comparisons
//   list     a block scan over the atoms' feature counts, then one over the ranked rings', gives every feature its place
//
// dl_feature_match: one workgroup per pair.  The A list goes through LDS 256 features at a time, one lane per B feature, no
// cross-lane traffic in the loop; d2 is clash.hip's, fp32 with contraction off.
//
// LDS: 4 x 8 KiB matrices + 4 KiB map + 3 KiB coordinates + per-atom and per-ring arrays: 42.5 KiB, static; 80 bytes of
// scratch per lane for the walk's arrays.
// Global memory is written with plain vector stores only; no global atomics of any kind; every output element is written.
#include "mol_graph.h"
#include "points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_PHARM_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;
constexpr int MAX_RINGS = DL_PHARM_MAX_RINGS;
constexpr int FAMILIES = DL_PHARM_FAMILIES;
constexpr int ATOM_FAMILIES = 5;                 // 0 .. 4 sit on an atom, 5 and 6 on a ring
enum : int { CLS_C = 1, CLS_N, CLS_O, CLS_S, CLS_P, CLS_F, CLS_HALOGEN };
enum : int { SET_C = 0, SET_N, SET_O, SET_S, SET_AROM, SET_MULTI, SET_O1, SET_ELIG, SETS };
static_assert(DL_PHARM_MAX_ATOMS == MATRIX_ATOMS && MAX_RINGS <= WG, "the matrix holds a molecule; one thread per ring");

struct Row {
    u64 w[WORDS];
};

__device__ __forceinline__ Row load_row(const u64* m, int u) {
    Row r;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) r.w[w] = m[u * WORDS + w];
    return r;
}
__device__ __forceinline__ int count(const Row& r) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) c += __popcll(r.w[w]);
    return c;
}
__device__ __forceinline__ int count_in(const Row& r, const u64* set) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) c += __popcll(r.w[w] & set[w]);
    return c;
}
__device__ __forceinline__ int count_outside(const Row& r, const u64* set) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) c += __popcll(r.w[w] & ~set[w]);
    return c;
}

// the first `limit` atoms above `floor` that are in row u of m and in `set`, ascending; returns how many were written
__device__ __forceinline__ int members_above(const u64* m, int u, const u64* set, int floor, int* out, int limit) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        u64 f = m[u * WORDS + w] & set[w];
        while (f && c < limit) {
            const int t = w * 64 + __builtin_ctzll(f);
            f &= f - 1;
            if (t > floor) out[c++] = t;
        }
    }
    return c;
}

__global__ __launch_bounds__(WG) void pharmacophore_kernel(dl_pharm_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_o2[MAX_KEPT * WORDS];          // of order 2
    __shared__ __align__(16) u64 s_o3[MAX_KEPT * WORDS];          // of order 3
    __shared__ __align__(16) u64 s_ar[MAX_KEPT * WORDS];          // aromatic
    __shared__ u64 s_set[SETS * WORDS];
    __shared__ u64 s_key[MAX_RINGS];
    __shared__ int s_map[MAX_ROWS];
    __shared__ float s_x[MAX_KEPT * 3];
    __shared__ int s_dv[MAX_KEPT];
    __shared__ short s_atom[MAX_KEPT];                            // atom number of a kept atom
    __shared__ unsigned char s_cls[MAX_KEPT], s_mark[MAX_KEPT];
    __shared__ unsigned char s_ring[MAX_RINGS * 6], s_ring_len[MAX_RINGS], s_sorted[MAX_RINGS];
    __shared__ int s_count[2];                                    // rings found, rings of carbons alone
    __shared__ int s_fc[ATOM_FAMILIES];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity, Fcap = a.Fcap;

    // ---- stage: rank the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;

    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb;
    int* family = a.family + size_t(b) * Fcap;
    int* anchor = a.anchor + size_t(b) * Fcap;
    float* position = a.position + size_t(b) * Fcap * 3;
    int* marked_out = a.marked + size_t(b) * Fcap;
    int* family_count = a.family_count + size_t(b) * FAMILIES;

    auto blank = [&](int first) {                                // the list from `first` on
        for (int f = first + tid; f < Fcap; f += WG) {
            family[f] = -1;
            anchor[f] = -1;
            position[f * 3] = position[f * 3 + 1] = position[f * 3 + 2] = 0.0f;
            marked_out[f] = 0;
        }
    };

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrices do not hold this molecule
        blank(0);
        if (tid < FAMILIES) family_count[tid] = 0;
        if (tid == 0) {
            a.n_features[b] = 0;
            a.status[b] = in.status | DL_PHARM_TOO_LARGE;
        }
        return;
    }

    const float* xs = a.x + size_t(b) * N * 3;
    const float* hot = a.one_hot + size_t(b) * N * nf;
    int bad_x = 0;
    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? kk : -1;
        if (!kept) return;
        const int type = first_maximum(hot + size_t(r) * nf, nf);
        const int cls = a.feature_class[type];
        s_cls[kk] = cls >= CLS_C && cls <= CLS_HALOGEN ? cls : 0;
        s_dv[kk] = a.default_valence[type];
        s_mark[kk] = mark && mark[r] != 0.0f;
        s_atom[kk] = short(k);
        bad_x |= stage_point(xs, r, s_x, kk);
    });
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = s_o2[tid * WORDS + w] = s_o3[tid * WORDS + w] = s_ar[tid * WORDS + w] = 0;
    if (tid < 2) s_count[tid] = 0;
    if (tid < ATOM_FAMILIES) s_fc[tid] = 0;
    __syncthreads();

    // ---- build: the pairs first, then what the first entry of every pair says about it
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    const int* arom_in = a.bond_aromatic + size_t(b) * capacity;
    const PairBuild pairs = build_pairs(list, nb, n, s_map, s_adj);
    for_each_first_entry(list, nb, n, s_map, pairs.repeated, [&](int e, const Bond& bd, int u, int v) {
        if (bd.order == 2) set_pair(s_o2, u, v);
        if (bd.order == 3) set_pair(s_o3, u, v);
        if (arom_in[e] != 0) set_pair(s_ar, u, v);
    });
    __syncthreads();

    // ---- atoms: the numbers of every atom, and the sets the neighbour tests need (bit t of word w is thread 64 w + t)
    const bool atom = tid < n_kept;
    const Row adj = load_row(s_adj, tid), o2 = load_row(s_o2, tid), o3 = load_row(s_o3, tid), ar = load_row(s_ar, tid);
    const int cls = atom ? s_cls[tid] : 0;
    const int deg = count(adj), n2 = count(o2), n3 = count(o3), n_ar = count(ar);
    const int val = deg + n2 + 2 * n3;
    const int h = atom ? max(0, s_dv[tid] - val) : 0;
    const bool arom = n_ar > 0, multi = n2 + n3 > 0;
    {
        const int w = tid >> 6;
        const u64 in_c = __ballot(cls == CLS_C), in_n = __ballot(cls == CLS_N), in_o = __ballot(cls == CLS_O),
                  in_s = __ballot(cls == CLS_S), in_arom = __ballot(arom), in_multi = __ballot(multi),
                  in_o1 = __ballot(cls == CLS_O && deg == 1), in_elig = __ballot(n_ar == 2 || n_ar == 3);
        if ((tid & 63) == 0) {
            s_set[SET_C * WORDS + w] = in_c;
            s_set[SET_N * WORDS + w] = in_n;
            s_set[SET_O * WORDS + w] = in_o;
            s_set[SET_S * WORDS + w] = in_s;
            s_set[SET_AROM * WORDS + w] = in_arom;
            s_set[SET_MULTI * WORDS + w] = in_multi;
            s_set[SET_O1 * WORDS + w] = in_o1;
            s_set[SET_ELIG * WORDS + w] = in_elig;
        }
    }
    __syncthreads();
    const u64* C = s_set + SET_C * WORDS;
    const u64* Nn = s_set + SET_N * WORDS;
    const u64* O = s_set + SET_O * WORDS;
    const u64* S = s_set + SET_S * WORDS;
    const u64* O1 = s_set + SET_O1 * WORDS;
    const u64* elig = s_set + SET_ELIG * WORDS;

    int fam = 0;                                                 // bit f: this atom has family f
    if (atom) {
        const bool quiet = count_in(adj, s_set + SET_AROM * WORDS) == 0 && count_in(adj, s_set + SET_MULTI * WORDS) == 0;
        const bool all_c = count_outside(adj, C) == 0;
        const bool donor = (cls == CLS_N || cls == CLS_O) && h >= 1;
        const bool acceptor = (cls == CLS_O && !arom && val <= 2) ||
                              (cls == CLS_N && h == 0 && val <= 3 && (multi || (deg == 3 && !arom && quiet)));
        bool positive = cls == CLS_N && !arom && !multi && val <= 3 && deg >= 1 && all_c && quiet;
        if (cls == CLS_C && !arom && n2 == 1 && n3 == 0 && count_in(o2, Nn) == 1 && count_in(adj, O) == 0 && count_in(adj, S) == 0) {
            Row single;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) single.w[w] = adj.w[w] & ~o2.w[w];
            positive = count_in(single, Nn) >= 1;
        }
        const int terminal = count_in(adj, O1);
        const bool negative = count_in(o2, O1) >= 1 &&
                              ((cls == CLS_C && terminal >= 2) || (cls == CLS_P && terminal >= 2) || (cls == CLS_S && terminal >= 3));
        const bool hydrophobe = (cls == CLS_C && deg >= 1 && all_c) || (cls == CLS_HALOGEN && deg == 1) ||
                                (cls == CLS_S && deg == 2 && !multi && !arom && all_c);
        fam = int(donor) | int(acceptor) << 1 | int(positive) << 2 | int(negative) << 3 | int(hydrophobe) << 4;
#pragma unroll
        for (int f = 0; f < ATOM_FAMILIES; ++f)
            if (fam >> f & 1) atomicAdd(&s_fc[f], 1);
    }
    int n_atom_features;
    int place = block_exclusive_scan(__popc(fam), s_scan, n_atom_features);
    for (int f = 0; f < ATOM_FAMILIES; ++f) {
        if (!(fam >> f & 1)) continue;
        if (place < Fcap) {
            family[place] = f;
            anchor[place] = s_atom[tid];
            position[place * 3] = s_x[tid * 3];
            position[place * 3 + 1] = s_x[tid * 3 + 1];
            position[place * 3 + 2] = s_x[tid * 3 + 2];
            marked_out[place] = s_mark[tid];
        }
        ++place;
    }

    // ---- rings: chordless 5- and 6-cycles of aromatic pairs, from their smallest atom
    if (atom && has(elig, tid)) {
        int path[6], cand[6][3], cnt[6], idx[6];
        int depth = 0;
        path[0] = tid;
        cnt[0] = members_above(s_ar, tid, elig, tid, cand[0], 3);
        idx[0] = 0;
        while (depth >= 0) {
            if (idx[depth] == cnt[depth]) { --depth; continue; }
            const int t = cand[depth][idx[depth]++];
            bool on_path = false;
            for (int l = 1; l <= depth; ++l) on_path |= path[l] == t;
            if (on_path) continue;
            path[++depth] = t;
            const int len = depth + 1;
            if (len >= 5 && bit(s_ar, t, tid) && path[1] < t) {
                bool chord = false;
                for (int p = 0; p < len; ++p)
                    for (int l = p + 2; l < len; ++l)
                        if (!(p == 0 && l == len - 1)) chord |= bit(s_adj, path[p], path[l]);
                if (!chord) {
                    const int slot = atomicAdd(&s_count[0], 1);
                    if (slot < MAX_RINGS) {
                        for (int l = 0; l < len; ++l) s_ring[slot * 6 + l] = path[l];
                        s_ring_len[slot] = len;
                    }
                }
            }
            if (len < 6) {
                cnt[depth] = members_above(s_ar, t, elig, tid, cand[depth], 3);
                idx[depth] = 0;
            } else {
                --depth;
            }
        }
    }
    __syncthreads();
    const int n_found = s_count[0];
    const bool many = n_found > MAX_RINGS;       // uniform: no ring feature is listed
    const int n_rings = many ? 0 : n_found;

    // rank the rings by their atom sequence: one byte per atom, a five-ring padded with 0, which no later atom of a ring is
    if (tid < n_rings) {
        u64 key = 0;
        for (int l = 0; l < 6; ++l) key = key << 8 | (l < s_ring_len[tid] ? s_ring[tid * 6 + l] : 0);
        s_key[tid] = key;
    }
    __syncthreads();
    if (tid < n_rings) {
        int rank = 0;
        for (int q = 0; q < n_rings; ++q) rank += s_key[q] < s_key[tid];
        s_sorted[rank] = tid;
    }
    __syncthreads();

    int len = 0, ring = 0, lumped = 0, all_marked = 0;
    if (tid < n_rings) {
        ring = s_sorted[tid];
        len = s_ring_len[ring];
        lumped = all_marked = 1;
        for (int l = 0; l < len; ++l) {
            const int v = s_ring[ring * 6 + l];
            lumped &= s_cls[v] == CLS_C;
            all_marked &= s_mark[v] != 0;
        }
        if (lumped) atomicAdd(&s_count[1], 1);
    }
    int n_ring_features;
    place = n_atom_features + block_exclusive_scan(len ? 1 + lumped : 0, s_scan, n_ring_features);
    if (len) {
        float c[3];
        for (int d = 0; d < 3; ++d) {
            double s = double(s_x[s_ring[ring * 6] * 3 + d]);
            for (int l = 1; l < len; ++l) s = s + double(s_x[s_ring[ring * 6 + l] * 3 + d]);
            c[d] = float(s / double(len));
        }
        for (int f = DL_PHARM_AROMATIC; f <= DL_PHARM_AROMATIC + lumped; ++f, ++place) {
            if (place >= Fcap) continue;
            family[place] = f;
            anchor[place] = s_atom[s_ring[ring * 6]];
            position[place * 3] = c[0];
            position[place * 3 + 1] = c[1];
            position[place * 3 + 2] = c[2];
            marked_out[place] = all_marked;
        }
    }
    const int n_features = n_atom_features + n_ring_features;
    blank(min(n_features, Fcap));
    bad_x = __syncthreads_or(bad_x);             // also orders s_count[1] before its read
    if (tid < ATOM_FAMILIES) family_count[tid] = s_fc[tid];
    if (tid == 0) {
        family_count[DL_PHARM_AROMATIC] = n_rings;
        family_count[DL_PHARM_AROMATIC + 1] = s_count[1];
        a.n_features[b] = n_features;
        a.status[b] = in.status | (pairs.bad ? DL_PHARM_BAD_BOND : 0) | (many ? DL_PHARM_MANY_RINGS : 0) |
                      (n_features > Fcap ? DL_PHARM_OVERFLOW : 0) | (bad_x ? DL_PHARM_NONFINITE : 0);
    }
}

__global__ __launch_bounds__(WG) void feature_match_kernel(dl_feature_match_args a) {
    __shared__ float s_ax[WG], s_ay[WG], s_az[WG];
    __shared__ int s_af[WG];                                      // family, or -1 for a feature that takes no part
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int Fa = a.Fa, Fb = a.Fb;
    const int na = min(max(a.n_features_a[b], 0), Fa), nbf = min(max(a.n_features_b[b], 0), Fb);
    const int* fam_a = a.family_a + size_t(b) * Fa;
    const int* fam_b = a.family_b + size_t(b) * Fb;
    const float* pos_a = a.position_a + size_t(b) * Fa * 3;
    const float* pos_b = a.position_b + size_t(b) * Fb * 3;
    const int* mk_a = a.marked_a + size_t(b) * Fa;
    const int* mk_b = a.marked_b + size_t(b) * Fb;
    int* best_index = a.best_index + size_t(b) * Fb;
    float* best_d2 = a.best_d2 + size_t(b) * Fb;
    const float radius2 = a.radius2;
    const bool marked_only = a.marked_only != 0;
    auto takes_part = [&](const int* fam, const int* mk, int f) {
        return fam[f] >= 0 && fam[f] < DL_PHARM_FAMILIES && !(marked_only && mk[f] == 0);
    };

    int mine_a = 0, mine_b = 0, mine_matched = 0;
    for (int i = tid; i < na; i += WG) mine_a += takes_part(fam_a, mk_a, i);
    for (int j0 = 0; j0 < Fb; j0 += WG) {        // uniform: every thread walks every block of B and every tile of A
        const int j = j0 + tid;
        const bool live = j < nbf && takes_part(fam_b, mk_b, j);
        const int fb = live ? fam_b[j] : -2;
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        if (live) { bx = pos_b[j * 3]; by = pos_b[j * 3 + 1]; bz = pos_b[j * 3 + 2]; }
        float best = __builtin_inff();
        int best_i = -1;
        for (int i0 = 0; i0 < (j0 < nbf ? na : 0); i0 += WG) {   // beyond B's count there is nothing to look for
            const int i = i0 + tid;
            const bool in = i < na && takes_part(fam_a, mk_a, i);
            s_af[tid] = in ? fam_a[i] : -1;
            if (i < na) { s_ax[tid] = pos_a[i * 3]; s_ay[tid] = pos_a[i * 3 + 1]; s_az[tid] = pos_a[i * 3 + 2]; }
            __syncthreads();
            const int tile = min(WG, na - i0);
            for (int q = 0; q < tile; ++q) {
                if (s_af[q] != fb) continue;
                const float dx = s_ax[q] - bx, dy = s_ay[q] - by, dz = s_az[q] - bz;
                const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);     // contraction is off: five roundings, in this order
                if (d2 < radius2 && d2 < best) { best = d2; best_i = i0 + q; }
            }
            __syncthreads();
        }
        if (j < Fb) {
            best_index[j] = best_i;
            best_d2[j] = best;
        }
        mine_b += live;
        mine_matched += best_i >= 0;
    }
    const int n_a = block_sum(mine_a, s_scan), n_b = block_sum(mine_b, s_scan), n_matched = block_sum(mine_matched, s_scan);
    if (tid == 0) {
        a.n_a[b] = n_a;
        a.n_b[b] = n_b;
        a.n_matched[b] = n_matched;
    }
}

}  // namespace

extern "C" {

int32_t dl_pharmacophore_features(const dl_pharm_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->capacity < 0 || a->Fcap < 0) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->feature_class || !a->default_valence || !a->n_bonds_in || !a->status_in ||
        !a->n_features || !a->family_count || !a->status || (a->capacity > 0 && (!a->bonds || !a->bond_aromatic)) ||
        (a->Fcap > 0 && (!a->family || !a->anchor || !a->position || !a->marked)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(pharmacophore_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

int32_t dl_feature_match(const dl_feature_match_args* a) {
    if (!a || a->B < 0 || a->Fa < 0 || a->Fb < 0 || !(a->radius2 >= 0.0f)) return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->n_features_a || !a->n_features_b || !a->n_a || !a->n_b || !a->n_matched ||
        (a->Fa > 0 && (!a->family_a || !a->position_a || !a->marked_a)) ||
        (a->Fb > 0 && (!a->family_b || !a->position_b || !a->marked_b || !a->best_index || !a->best_d2)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(feature_match_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
