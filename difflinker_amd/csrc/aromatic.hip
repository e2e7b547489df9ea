// aromatic.hip — aromatic rings of the bond graphs bonds.hip left on the device, perceived from the 3D geometry: planar five-
// and six-rings, a Kekule assignment of single and double bonds to them, and the rings whose electron count is six.  The rule
// is this project's own, stated in full in include/difflinker_hip.h and restated in tests/aromatic_ref.py; it is NOT RDKit's
// aromaticity model and NOT OpenBabel's bond typing, which the reference reaches through `obabel`.
//
// One 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h: atom k is the k-th row with
// node_mask != 0; drop_mask removes atoms after that numbering together with their bonds; an entry (i, j, order) is a bond
// when 0 <= i, j < atoms, i != j and 1 <= order <= 3; anything else is skipped and sets DL_AROM_BAD_BOND.
//
//   stage    rows ranked by number_rows of mol_graph.h; the kept atoms' coordinates, classes and marks go to LDS by kept index
//   build    the 256 x 256 bit matrix of the kept pairs (LDS atomicOr; the old value tells a repeated pair)
//   cycles   thread s owns kept atom s: a depth-first walk over eligible atoms larger than s, at most six deep and at most
//            3 * 2^4 leaves, that closes chordless cycles of 5 and 6 atoms in canonical order.  The thread that closes a
//            cycle tests its planarity on the spot, in fp64 with contraction off and the operations in the header's order,
//            and appends a planar one to the ring list (an LDS counter; the order of the list plays no part below: every
//            later step is an OR, a count or a per-ring answer)
//   systems  ring bonds into a second bit matrix; label propagation with pointer jumping over it, as rings.hip labels pieces
//   roles    one thread per list entry flags the ends of bonds of order 2 or 3 outside the rings; one thread per atom
//   kekule   the thread of a system's smallest atom solves the system alone (kekule.h: at most 32 atoms, bit masks), its
//            arrays in one of SLOTS workspaces in LDS; a molecule with more systems than that takes them in rounds
//   rings    one thread per planar ring: covered P atoms and the electron count; aromatic bonds into a third bit matrix
//   write    one thread per list entry, then one per row
//
// "The first entry of a repeated pair" needs list order, which the matrix does not keep: only when the build saw a repeated
// pair (never in a list of dl_perceive_bonds) an entry looks through the entries before it.
// LDS: 3 x 8 KiB matrices + 4 KiB map + 3 KiB coordinates + 6 KiB solver workspaces + per-atom and per-ring arrays: about
// 45 KiB, static.
// Global memory is written with plain vector stores only; no global atomics of any kind; every output element is written.
#include "mol_graph.h"
#include "kekule.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_AROM_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;
constexpr int MAX_RINGS = DL_AROM_MAX_RINGS;
constexpr int MAX_SYSTEM = DL_AROM_MAX_SYSTEM;
constexpr int SLOTS = 8;                         // systems solved at a time
constexpr int MARK = 1 << 16;                    // s_map: kept index | MARK
enum : int { ROLE_NONE = 0, ROLE_D, ROLE_X, ROLE_P, ROLE_F };
static_assert(MAX_RINGS <= WG && MAX_SYSTEM == kekule::MAXV, "one thread per ring; kekule.h holds a system");

// the first `limit` neighbours of atom a in ascending order; returns how many were written
__device__ __forceinline__ int neighbours(const u64* m, int a, int* out, int limit) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        u64 f = m[a * WORDS + w];
        while (f && c < limit) {
            out[c++] = w * 64 + __builtin_ctzll(f);
            f &= f - 1;
        }
    }
    return c;
}

// the planarity test of the header for the cycle path[0..len) in canonical order
__device__ bool ring_is_planar(const u64* adj, const float* xs, const int* path, int len, double tol2_ring, double tol2_sub) {
    double p[6][3], q[6][3], c[3], m[3];
    for (int k = 0; k < len; ++k)
        for (int d = 0; d < 3; ++d) p[k][d] = double(xs[path[k] * 3 + d]);
    for (int d = 0; d < 3; ++d) {
        double s = p[0][d];
        for (int k = 1; k < len; ++k) s = s + p[k][d];
        c[d] = s / double(len);
    }
    for (int k = 0; k < len; ++k)
        for (int d = 0; d < 3; ++d) q[k][d] = p[k][d] - c[d];
    for (int k = 0; k < len; ++k) {
        const double* a = q[k];
        const double* b = q[k + 1 == len ? 0 : k + 1];
        const double tx = a[1] * b[2] - a[2] * b[1];
        const double ty = a[2] * b[0] - a[0] * b[2];
        const double tz = a[0] * b[1] - a[1] * b[0];
        if (k == 0) { m[0] = tx; m[1] = ty; m[2] = tz; }
        else { m[0] = m[0] + tx; m[1] = m[1] + ty; m[2] = m[2] + tz; }
    }
    const double mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (!(mm > 0.0)) return false;
    const double limit_ring = tol2_ring * mm, limit_sub = tol2_sub * mm;
    for (int k = 0; k < len; ++k) {
        const double d = (q[k][0] * m[0] + q[k][1] * m[1]) + q[k][2] * m[2];
        if (!(d * d <= limit_ring)) return false;
    }
    for (int k = 0; k < len; ++k) {
        int nb[3];
        const int cnt = neighbours(adj, path[k], nb, 3);          // ring atoms are eligible: at most three neighbours
        for (int t = 0; t < cnt; ++t) {
            const int s = nb[t];
            bool inside = false;
            for (int l = 0; l < len; ++l) inside |= path[l] == s;
            if (inside) continue;
            const double sx = double(xs[s * 3]) - c[0], sy = double(xs[s * 3 + 1]) - c[1], sz = double(xs[s * 3 + 2]) - c[2];
            const double d = (sx * m[0] + sy * m[1]) + sz * m[2];
            if (!(d * d <= limit_sub)) return false;
        }
    }
    return true;
}

__global__ __launch_bounds__(WG) void aromatic_rings_kernel(dl_aromatic_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_rb[MAX_KEPT * WORDS];          // ring bonds
    __shared__ __align__(16) u64 s_ab[MAX_KEPT * WORDS];          // aromatic bonds
    __shared__ int s_map[MAX_ROWS];
    __shared__ float s_x[MAX_KEPT * 3];
    __shared__ int s_label[MAX_KEPT];
    __shared__ int s_size[MAX_KEPT];                              // atoms of the system, at its label
    __shared__ int s_val[MAX_KEPT];
    __shared__ int s_exo[MAX_KEPT];                               // has a bond of order >= 2 that is no ring bond
    __shared__ int s_arom[MAX_KEPT];
    __shared__ short s_mate[MAX_KEPT];
    __shared__ unsigned char s_cls[MAX_KEPT], s_mark[MAX_KEPT], s_deg[MAX_KEPT], s_elig[MAX_KEPT], s_role[MAX_KEPT],
        s_local[MAX_KEPT];
    __shared__ unsigned char s_ring[MAX_RINGS * 6], s_ring_len[MAX_RINGS];
    __shared__ int s_count[4];                                    // planar rings, aromatic rings, aromatic marked rings, systems
    __shared__ int s_work[SLOTS * kekule::WORDS];
    __shared__ int s_scan[WG_WAVES];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, nf = a.nf, capacity = a.capacity;

    // ---- stage: rank the real rows, and the kept rows among themselves
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept;

    const int given = a.n_bonds_in[b];
    const int nb = min(max(given, 0), capacity);
    const int status_in = a.status_in[b] | (given > capacity ? DL_BONDS_OVERFLOW : 0);
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    int* order_out = a.order_out + size_t(b) * capacity;
    int* bond_aromatic = a.bond_aromatic + size_t(b) * capacity;
    int* atom_aromatic = a.atom_aromatic + size_t(b) * N;
    int* valence_out = a.valence_out + size_t(b) * N;

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrices do not hold this molecule
        int bad = 0;
        for (int e = tid; e < capacity; e += WG) {
            int i, j, order = 0;
            if (e < nb && !load_bond<3>(list, e, n, i, j, order)) { bad = 1; order = 0; }
            order_out[e] = e < nb ? order : 0;
            bond_aromatic[e] = 0;
        }
        for (int i = tid; i < N; i += WG) { atom_aromatic[i] = 0; valence_out[i] = 0; }
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            a.n_planar_rings[b] = 0;
            a.n_aromatic_rings[b] = 0;
            a.n_aromatic_marked[b] = 0;
            a.status[b] = status_in | DL_AROM_TOO_LARGE | (bad ? DL_AROM_BAD_BOND : 0);
        }
        return;
    }

    const float* xs = a.x + size_t(b) * N * 3;
    const float* hot = a.one_hot + size_t(b) * N * nf;
    // the numbering loop and, below, the list's length and the pair build stand here in their own text and not as
    // for_each_real_row, bonds_in and add_pair of mol_graph.h: with those refine_bond_orders measured 0.3 % slower than before
    // the helpers were shared, and this kernel is the one the time goes to (profiles/mol_graph/README.md)
    int k = rn.k, kk = rn.kk;
    for (int r = rows.r0; r < rows.r1; ++r) {
        if (mask[r] == 0.0f) continue;
        const bool kept = !(drop && drop[r] != 0.0f);
        const bool marked = mark && mark[r] != 0.0f;
        s_map[k++] = kept ? (kk | (marked ? MARK : 0)) : -1;
        if (!kept) continue;
        const int cls = a.ring_class[first_maximum(hot + size_t(r) * nf, nf)];
        s_cls[kk] = cls >= 1 && cls <= 3 ? cls : 0;
        s_mark[kk] = marked;
        s_x[kk * 3] = xs[r * 3];
        s_x[kk * 3 + 1] = xs[r * 3 + 1];
        s_x[kk * 3 + 2] = xs[r * 3 + 2];
        ++kk;
    }
#pragma unroll
    for (int w = 0; w < WORDS; ++w) s_adj[tid * WORDS + w] = s_rb[tid * WORDS + w] = s_ab[tid * WORDS + w] = 0;
    s_label[tid] = tid;
    s_size[tid] = 0;
    s_val[tid] = 0;
    s_exo[tid] = 0;
    s_arom[tid] = 0;
    s_mate[tid] = -1;
    if (tid < 4) s_count[tid] = 0;
    __syncthreads();

    // ---- build: the bit matrix over the kept atoms
    int bad = 0, repeated = 0;
    for (int e = tid; e < nb; e += WG) {
        int i, j, order;
        if (!load_bond<3>(list, e, n, i, j, order)) { bad = 1; continue; }
        const int mi = s_map[i], mj = s_map[j];
        if ((mi | mj) < 0) continue;                             // an end is dropped: no bond of this graph, and no error
        const int u = mi & 0xFFFF, v = mj & 0xFFFF;
        const int lo = min(u, v), hi = max(u, v);
        const u64 one = 1ull << (hi & 63);
        const u64 old = atomicOr(&s_adj[lo * WORDS + (hi >> 6)], one);
        atomicOr(&s_adj[hi * WORDS + (lo >> 6)], 1ull << (lo & 63));
        if (old & one) repeated = 1;                             // the pair a second time
    }
    repeated = __syncthreads_or(repeated);
    bad = __syncthreads_or(bad) | repeated;

    // ---- eligible atoms
    const bool atom = tid < n_kept;
    {
        int deg = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) deg += __popcll(s_adj[tid * WORDS + w]);
        const int cls = atom ? s_cls[tid] : 0;
        s_deg[tid] = min(deg, 255);
        s_elig[tid] = atom && (((cls == 1 || cls == 2) && (deg == 2 || deg == 3)) || (cls == 3 && deg == 2));
    }
    __syncthreads();

    // ---- cycles: chordless 5- and 6-cycles from their smallest atom, planar ones into the list
    if (s_elig[tid]) {
        int path[6], cand[6][3], cnt[6], idx[6];
        int depth = 0;
        path[0] = tid;
        cnt[0] = neighbours(s_adj, tid, cand[0], 3);
        idx[0] = 0;
        while (depth >= 0) {
            if (idx[depth] == cnt[depth]) { --depth; continue; }
            const int t = cand[depth][idx[depth]++];
            if (t <= tid || !s_elig[t]) continue;
            bool on_path = false;
            for (int l = 1; l <= depth; ++l) on_path |= path[l] == t;
            if (on_path) continue;
            path[++depth] = t;
            const int len = depth + 1;
            if (len >= 5 && bit(s_adj, t, tid) && path[1] < t) {
                bool chord = false;
                for (int p = 0; p < len; ++p)
                    for (int l = p + 2; l < len; ++l)
                        if (!(p == 0 && l == len - 1)) chord |= bit(s_adj, path[p], path[l]);
                if (!chord && ring_is_planar(s_adj, s_x, path, len, a.tol2_ring, a.tol2_sub)) {
                    const int slot = atomicAdd(&s_count[0], 1);
                    if (slot < MAX_RINGS) {
                        for (int l = 0; l < len; ++l) s_ring[slot * 6 + l] = path[l];
                        s_ring_len[slot] = len;
                    }
                }
            }
            if (len < 6) {
                cnt[depth] = neighbours(s_adj, t, cand[depth], 3);
                idx[depth] = 0;
            } else {
                --depth;
            }
        }
    }
    __syncthreads();
    const int n_planar = s_count[0];
    const bool many = n_planar > MAX_RINGS;      // uniform: no ring is used, every order passes through
    const int n_rings = many ? 0 : n_planar;

    // ---- systems: ring bonds, then the pieces of their graph
    if (tid < n_rings) {
        const int len = s_ring_len[tid];
        for (int l = 0; l < len; ++l) set_pair(s_rb, s_ring[tid * 6 + l], s_ring[tid * 6 + (l + 1 == len ? 0 : l + 1)]);
    }
    __syncthreads();
    for (;;) {
        int changed = 0, best = tid;
        if (atom) {
            best = s_label[tid];
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = s_rb[tid * WORDS + w];
                while (f) {
                    best = min(best, s_label[w * 64 + __builtin_ctzll(f)]);
                    f &= f - 1;
                }
            }
        }
        __syncthreads();
        if (atom && best < s_label[tid]) { s_label[tid] = best; changed = 1; }
        __syncthreads();
        const int jump = s_label[s_label[tid]];
        __syncthreads();
        if (jump != s_label[tid]) { s_label[tid] = jump; changed = 1; }
        if (!__syncthreads_or(changed)) break;
    }
    const bool in_system = (s_rb[tid * WORDS] | s_rb[tid * WORDS + 1] | s_rb[tid * WORDS + 2] | s_rb[tid * WORDS + 3]) != 0;
    if (in_system) atomicAdd(&s_size[s_label[tid]], 1);

    // ---- roles
    for (int e = tid; e < nb; e += WG) {
        int i, j, order;
        if (!load_bond<3>(list, e, n, i, j, order) || order < 2) continue;
        const int mi = s_map[i], mj = s_map[j];
        if ((mi | mj) < 0) continue;
        const int u = mi & 0xFFFF, v = mj & 0xFFFF;
        if (bit(s_rb, u, v) || (repeated && seen_before<3>(list, e, n, i, j))) continue;
        atomicOr(&s_exo[u], 1);
        atomicOr(&s_exo[v], 1);
    }
    __syncthreads();
    {
        int role = ROLE_NONE;
        if (in_system) {
            const int cls = s_cls[tid];
            role = (cls == 3 || (cls == 2 && s_deg[tid] == 3)) ? ROLE_D : s_exo[tid] ? ROLE_X : cls == 1 ? ROLE_P : ROLE_F;
        }
        s_role[tid] = role;
    }
    __syncthreads();

    // ---- kekule: the thread of a system's smallest atom assigns the system, SLOTS systems at a time
    const bool root = in_system && s_label[tid] == tid;
    const int big = __syncthreads_or(root && s_size[tid] > MAX_SYSTEM);
    const bool solves = root && s_size[tid] <= MAX_SYSTEM;
    const int turn = solves ? atomicAdd(&s_count[3], 1) : 0;     // any order: a system's answer depends on the system alone
    __syncthreads();
    const int n_systems = s_count[3];
    for (int round = 0; round * SLOTS < n_systems; ++round) {
        if (solves && turn / SLOTS == round) {
            int* work = s_work + (turn % SLOTS) * kekule::WORDS;
            int members[MAX_SYSTEM], mate[MAX_SYSTEM];
            kekule::mask_t can = 0, heavy = 0;
            int count = 0;
            for (int v = tid; v < n_kept && count < MAX_SYSTEM; ++v) {
                const bool member = s_label[v] == tid &&
                                    (s_rb[v * WORDS] | s_rb[v * WORDS + 1] | s_rb[v * WORDS + 2] | s_rb[v * WORDS + 3]) != 0;
                if (!member) continue;
                s_local[v] = count;              // read by this thread alone
                members[count] = v;
                const int role = s_role[v];
                if (role == ROLE_P || role == ROLE_F) can |= 1u << count;
                if (role == ROLE_P) heavy |= 1u << count;
                ++count;
            }
            for (int l = 0; l < count; ++l) {
                kekule::mask_t row = 0;
                if (can >> l & 1) {
                    int nbr[3];
                    const int c = neighbours(s_rb, members[l], nbr, 3);
                    for (int t = 0; t < c; ++t) {
                        const int other = s_local[nbr[t]];
                        if (can >> other & 1) row |= 1u << other;
                    }
                }
                work[l] = int(row);
            }
            kekule::assign(work, count, can, heavy, mate);
            for (int l = 0; l < count; ++l)
                if (mate[l] >= 0) s_mate[members[l]] = short(members[mate[l]]);
        }
        __syncthreads();
    }

    // ---- rings: which planar rings are aromatic
    if (tid < n_rings && s_size[s_label[s_ring[tid * 6]]] <= MAX_SYSTEM) {
        const int len = s_ring_len[tid];
        int electrons = 0;
        bool open = false, all_marked = true;
        for (int l = 0; l < len; ++l) {
            const int v = s_ring[tid * 6 + l];
            const int role = s_role[v];
            const bool covered = s_mate[v] >= 0;
            open |= role == ROLE_P && !covered;
            electrons += role == ROLE_D ? 2 : role == ROLE_X ? 0 : covered ? 1 : 2;
            all_marked &= s_mark[v] != 0;
        }
        if (!open && electrons == 6) {
            atomicAdd(&s_count[1], 1);
            if (mark && all_marked) atomicAdd(&s_count[2], 1);
            for (int l = 0; l < len; ++l) {
                const int v = s_ring[tid * 6 + l];
                atomicOr(&s_arom[v], 1);
                set_pair(s_ab, v, s_ring[tid * 6 + (l + 1 == len ? 0 : l + 1)]);
            }
        }
    }
    __syncthreads();

    // ---- write
    for (int e = tid; e < capacity; e += WG) {
        int order = 0, aromatic = 0, i, j;
        if (e < nb && load_bond<3>(list, e, n, i, j, order)) {
            const int mi = s_map[i], mj = s_map[j];
            if ((mi | mj) >= 0) {
                const int u = mi & 0xFFFF, v = mj & 0xFFFF;
                if (bit(s_rb, u, v) && s_size[s_label[u]] <= MAX_SYSTEM) {
                    order = s_mate[u] == v ? 2 : 1;
                    aromatic = bit(s_ab, u, v);
                }
                if (!(repeated && seen_before<3>(list, e, n, i, j))) {
                    atomicAdd(&s_val[u], order);
                    atomicAdd(&s_val[v], order);
                }
            }
        } else {
            order = 0;
        }
        order_out[e] = order;
        bond_aromatic[e] = aromatic;
    }
    __syncthreads();
    for (int i = tid; i < N; i += WG) {
        int valence = 0, aromatic = 0;
        if (i < n && s_map[i] >= 0) {
            valence = s_val[s_map[i] & 0xFFFF];
            aromatic = s_arom[s_map[i] & 0xFFFF];
        }
        valence_out[i] = valence;
        atom_aromatic[i] = aromatic;
    }
    if (tid == 0) {
        a.n_planar_rings[b] = n_rings;
        a.n_aromatic_rings[b] = s_count[1];
        a.n_aromatic_marked[b] = s_count[2];
        a.status[b] = status_in | (bad ? DL_AROM_BAD_BOND : 0) | (many ? DL_AROM_MANY_RINGS : 0) | (big ? DL_AROM_BIG_SYSTEM : 0);
    }
}

}  // namespace

extern "C" {

int32_t dl_aromatic_rings(const dl_aromatic_args* a, void* stream) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->capacity < 0 || !(a->tol2_ring >= 0.0) ||
        !(a->tol2_sub >= 0.0))
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->ring_class || !a->n_bonds_in || !a->status_in || !a->atom_aromatic ||
        !a->valence_out || !a->n_planar_rings || !a->n_aromatic_rings || !a->n_aromatic_marked || !a->status ||
        (a->capacity > 0 && (!a->bonds || !a->order_out || !a->bond_aromatic)))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(aromatic_rings_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
