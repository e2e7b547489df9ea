// relax.hip — a restrained clean-up of the marked (linker) atoms of every molecule: FIRE minimisation (Bitzek et al., PRL 97,
// 170201) of bond, angle, repulsion, wall and position-restraint terms in fp64, the topology frozen at the bond list
// bonds.hip and aromatic.hip left on the device.  The rule is this project's own; it is stated in full in
// include/difflinker_hip.h and restated in tests/relax_ref.py, and it is NOT UFF, MMFF, RDKit's or OpenBabel's optimiser.
//
// dl_relax_molecules: one 256-thread workgroup per molecule, one launch per batch, with the conventions of mol_graph.h.
//
//   stage    rows ranked by number_rows; type, planar flag, mark, row and the fp64 position of the kept atoms go to LDS by kept
//            index; the dropped real rows - the wall - leave their row and type by wall rank (atom number minus kept index)
//   build    four 256 x 256 bit matrices: the pairs (build_pairs), those of order 2, of order 3, and those flagged aromatic
//   atoms    thread u owns kept atom u: the class of its angles and which of its (at most six) pairs carry a term; its far
//            pairs as a row of a fifth matrix; a scan numbers the movable atoms
//   step     thread u sums the bond and angle terms of its atom in the stated order, while wave w walks the far pairs and
//            the wall of the movable atoms w, w + 4 ... : lane l takes the partners l, l + 64 ... - the 64 partials of the rule
//            - and the xor-butterfly is the rule's tree.  One barrier; one fused reduction of F.v, F.F, v.v and max |F|;
//            the update; one barrier
//   energy   twice, the same terms by their owners, five tree sums
//
// LDS: 5 x 8 KiB matrices + 4 KiB map + 6 KiB positions + 6 KiB pair forces + 3 KiB wall rows and types + per-atom arrays:
// about 62 KiB, static.  The wall's coordinates are read in place (L2).  Global memory is written with plain vector stores
// only; no atomics on global memory; no workspace.
#include "mol_graph.h"
#include "points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_ROWS = 1024;                   // N, as for dl_perceive_bonds
constexpr int MAX_KEPT = MATRIX_ATOMS;           // DL_RELAX_MAX_ATOMS
constexpr int WORDS = MATRIX_WORDS;
static_assert(DL_RELAX_MAX_ATOMS == MATRIX_ATOMS, "the matrix holds a molecule");
static_assert(DL_RELAX_TERMS == 5, "five terms per row of energy");

enum : int { LINEAR = 0, TRIGONAL = 1, TETRAHEDRAL = 2 };

__device__ __forceinline__ bool nonfinite(double v) { return (__double2hiint(v) & 0x7ff00000) == 0x7ff00000; }
__device__ __forceinline__ V3 dpoint(const double* xs, int atom) { return {xs[atom * 3], xs[atom * 3 + 1], xs[atom * 3 + 2]}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 times(double g, V3 a) { return {g * a.x, g * a.y, g * a.z}; }
__device__ __forceinline__ V3 wave_tree_sum(V3 a) { return {wave_tree_sum(a.x), wave_tree_sum(a.y), wave_tree_sum(a.z)}; }

// the cosine of the angle j-a-k and what its gradient needs; false: an arm of length zero, no term
struct Angle {
    V3 p, q;
    double pp, qq, den, c;
};
__device__ __forceinline__ bool angle_at(V3 xa, V3 xj, V3 xk, Angle& g) {
    g.p = sub(xj, xa);
    g.q = sub(xk, xa);
    g.pp = dot(g.p, g.p);
    g.qq = dot(g.q, g.q);
    if (g.pp == 0.0 || g.qq == 0.0) return false;
    g.den = sqrt(g.pp * g.qq);
    g.c = dot(g.p, g.q) / g.den;
    return true;
}

// the force of the angle term on its centre (role 0), on j (1) or on k (2)
__device__ __forceinline__ bool angle_force(V3 xa, V3 xj, V3 xk, double c0, double two_k, int role, V3& f) {
    Angle g;
    if (!angle_at(xa, xj, xk, g)) return false;
    const double mg = two_k * (c0 - g.c), inv = 1.0 / g.den, pa = g.c / g.pp, pb = g.c / g.qq;
    const V3 fj = {mg * (g.q.x * inv - g.p.x * pa), mg * (g.q.y * inv - g.p.y * pa), mg * (g.q.z * inv - g.p.z * pa)};
    const V3 fk = {mg * (g.p.x * inv - g.q.x * pb), mg * (g.p.y * inv - g.q.y * pb), mg * (g.p.z * inv - g.q.z * pb)};
    f = role == 1 ? fj : role == 2 ? fk : V3{-(fj.x + fk.x), -(fj.y + fk.y), -(fj.z + fk.z)};
    return true;
}

__device__ __forceinline__ int pair_bit(int lo, int hi) { return hi * (hi - 1) / 2 + lo; }     // pair order: hi, then lo

__global__ __launch_bounds__(WG) void relax_kernel(dl_relax_args a) {
    __shared__ __align__(16) u64 s_adj[MAX_KEPT * WORDS];         // kept pairs
    __shared__ __align__(16) u64 s_o2[MAX_KEPT * WORDS];          // of order 2
    __shared__ __align__(16) u64 s_o3[MAX_KEPT * WORDS];          // of order 3
    __shared__ __align__(16) u64 s_ar[MAX_KEPT * WORDS];          // flagged aromatic
    __shared__ __align__(16) u64 s_far[MAX_KEPT * WORDS];         // far pairs
    __shared__ int s_map[MAX_ROWS];                               // atom number -> kept index, or -1
    __shared__ double s_x[MAX_KEPT * 3];                          // the state
    __shared__ double s_nb[MAX_KEPT * 3];                         // far + wall force of the movable atoms (energy: the two terms)
    __shared__ unsigned short s_wall[MAX_ROWS], s_row[MAX_KEPT], s_movable[MAX_KEPT];       // rows by wall rank / kept index; kept index by movable rank
    __shared__ unsigned char s_wtype[MAX_ROWS], s_type[MAX_KEPT], s_planar[MAX_KEPT], s_mov[MAX_KEPT], s_terms[MAX_KEPT], s_cls[MAX_KEPT];
    __shared__ int s_scan[WG_WAVES];
    __shared__ double s_sum[WG_WAVES], s_red[WG_WAVES * 4];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, nf = a.nf, capacity = a.capacity;

    // ---- stage
    const Rows rows = own_rows(N);
    const float* mask = a.node_mask + size_t(b) * N;
    const float* drop = a.drop_mask ? a.drop_mask + size_t(b) * N : nullptr;
    const float* mark = a.mark_mask ? a.mark_mask + size_t(b) * N : nullptr;
    const int* planar = a.atom_planar ? a.atom_planar + size_t(b) * N : nullptr;
    const RowNumbers rn = number_rows(rows, mask, drop, s_scan);
    const int n = rn.n, n_kept = rn.n_kept, n_wall = a.use_wall ? n - n_kept : 0;

    const BondsIn in = bonds_in(a.n_bonds_in, a.status_in, b, capacity);
    const int nb = in.nb;
    const float* xs = a.x + size_t(b) * N * 3;
    const float* hot = a.one_hot + size_t(b) * N * nf;
    const unsigned* x_bits = reinterpret_cast<const unsigned*>(xs);
    unsigned* out_bits = reinterpret_cast<unsigned*>(a.x_out + size_t(b) * N * 3);
    double* energy = a.energy + size_t(b) * 2 * DL_RELAX_TERMS;

    // a molecule that does not run: x_out = x, `done` steps and the energy written so far stand, the rest is 0
    auto leave = [&](int status, int done, bool keep_before) {
        for (int k = tid; k < N * 3; k += WG) out_bits[k] = x_bits[k];
        if (tid < 2 * DL_RELAX_TERMS && !(keep_before && tid < DL_RELAX_TERMS)) energy[tid] = 0.0;
        if (tid == 0) {
            a.steps_done[b] = done;
            a.f_max[b] = 0.0;
            a.moved2[b] = 0.0;
            a.status[b] = status;
        }
    };

    if (n_kept > MAX_KEPT) {                     // uniform over the workgroup: the matrices do not hold this molecule
        leave(in.status | DL_POSE_TOO_LARGE, 0, false);
        return;
    }

    int bad_x = 0;
    for_each_real_row(rows, mask, drop, rn, [&](int r, int k, bool kept, int kk) {
        s_map[k] = kept ? kk : -1;
        if (!kept) {
            if (n_wall) {
                s_wall[k - kk] = (unsigned short)r;
                s_wtype[k - kk] = (unsigned char)first_maximum(hot + size_t(r) * nf, nf);
            }
            return;
        }
        s_row[kk] = (unsigned short)r;
        s_type[kk] = (unsigned char)first_maximum(hot + size_t(r) * nf, nf);
        s_planar[kk] = planar && planar[k] != 0;
        s_mov[kk] = !mark || mark[r] != 0.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = xs[size_t(r) * 3 + d];
            s_x[kk * 3 + d] = double(v);
            bad_x |= nonfinite(v);
        }
    });
#pragma unroll
    for (int w = 0; w < WORDS; ++w)
        s_adj[tid * WORDS + w] = s_o2[tid * WORDS + w] = s_o3[tid * WORDS + w] = s_ar[tid * WORDS + w] = s_far[tid * WORDS + w] = 0;
    s_terms[tid] = 0;
    bad_x = __syncthreads_or(bad_x);

    // ---- build
    const int* list = a.bonds + size_t(b) * capacity * 3;        // never read when nb == 0
    const int* flagged = a.bond_aromatic ? a.bond_aromatic + size_t(b) * capacity : nullptr;
    const PairBuild pairs = build_pairs(list, nb, n, s_map, s_adj);
    const int status0 = in.status | (pairs.bad ? DL_POSE_BAD_BOND : 0);
    if (bad_x) {
        leave(status0 | DL_POSE_NONFINITE, 0, false);
        return;
    }
    for_each_first_entry(list, nb, n, s_map, pairs.repeated, [&](int e, const Bond& bd, int u, int v) {
        if (bd.order == 2) set_pair(s_o2, u, v);
        if (bd.order == 3) set_pair(s_o3, u, v);
        if (flagged && flagged[e] != 0) set_pair(s_ar, u, v);
    });
    __syncthreads();                             // the matrices are complete

    // ---- atoms: angle terms and far pairs of u; the movable atoms numbered
    const bool mine = tid < n_kept;
    const int u = tid;
    const bool mov_u = mine && s_mov[u];
    if (mine) {
        const int d = count_row(s_adj, u);
        if (d >= 2 && d <= 4) {
            const int n2 = count_row(s_o2, u), n3 = count_row(s_o3, u);
            s_cls[u] = (d == 2 && (n3 >= 1 || n2 == 2)) ? LINEAR : ((d <= 3 && n2 >= 1) || s_planar[u]) ? TRIGONAL : TETRAHEDRAL;
            int nbr[4];
            first_members(s_adj, u, -1, nbr, 4);
            int terms = 0;
            for (int q = 1; q < d; ++q) {
                for (int p = 0; p < q; ++p) {
                    const int j = nbr[p], k = nbr[q];
                    if (bit(s_adj, j, k)) continue;              // a three-ring
                    u64 both = 0, reach[WORDS] = {0, 0, 0, 0};
#pragma unroll
                    for (int w = 0; w < WORDS; ++w) both |= s_adj[j * WORDS + w] & s_adj[k * WORDS + w] & ~bit_in_word(u, w);
                    if (both) continue;                          // a four-ring
#pragma unroll
                    for (int w = 0; w < WORDS; ++w) {            // what the neighbours of j other than u are bonded to
                        u64 f = s_adj[j * WORDS + w] & ~bit_in_word(u, w);
                        while (f) {
                            const u64* row = s_adj + (w * 64 + __builtin_ctzll(f)) * WORDS;
                            f &= f - 1;
#pragma unroll
                            for (int t = 0; t < WORDS; ++t) reach[t] |= row[t];
                        }
                    }
#pragma unroll
                    for (int w = 0; w < WORDS; ++w) both |= reach[w] & s_adj[k * WORDS + w] & ~bit_in_word(u, w);
                    if (both) continue;                          // a five-ring
                    terms |= 1 << pair_bit(p, q);
                }
            }
            s_terms[u] = (unsigned char)terms;
        }
        u64 frontier[WORDS], ball[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            frontier[w] = s_adj[u * WORDS + w];
            ball[w] = frontier[w] | bit_in_word(u, w);
        }
        for (int level = 2; level <= 3; ++level) {
            u64 next[WORDS] = {0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = frontier[w];
                while (f) {
                    const u64* row = s_adj + (w * 64 + __builtin_ctzll(f)) * WORDS;
                    f &= f - 1;
#pragma unroll
                    for (int q = 0; q < WORDS; ++q) next[q] |= row[q];
                }
            }
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                frontier[w] = next[w] & ~ball[w];
                ball[w] |= frontier[w];
            }
        }
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            const int left = n_kept - w * 64;                    // kept atoms from bit 0 of this word on
            const u64 valid = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0ull;
            s_far[u * WORDS + w] = ~ball[w] & valid;
        }
    }
    int n_mov;
    const int rank = block_exclusive_scan(int(mov_u), s_scan, n_mov);
    if (mov_u) s_movable[rank] = (unsigned short)u;
    __syncthreads();

    const V3 x0 = mine ? dpoint(s_x, u) : V3{0.0, 0.0, 0.0};

    // L0 of the kept pair (p, q); the lower atom's type first
    auto length0 = [&](int p, int q) -> double {
        const int lo = min(p, q), hi = max(p, q), cell = int(s_type[lo]) * nf + s_type[hi];
        if (bit(s_ar, p, q)) return a.aromatic_length0[cell];
        return a.length0[cell * 3 + (bit(s_o3, p, q) ? 2 : bit(s_o2, p, q) ? 1 : 0)];
    };

    // one pair term of the repulsion form: w = x_u - x_partner
    auto pair_force = [&](V3 w, double r2, double four_k, V3& part) {
        const double d2 = dot(w, w);
        if (d2 < r2) {
            const double s = 1.0 - d2 / r2, g = (four_k * s) / r2;
            part = add(part, times(g, w));
        }
    };
    auto pair_energy = [&](V3 w, double r2, double k, double& part) {
        const double d2 = dot(w, w);
        if (d2 < r2) {
            const double s = 1.0 - d2 / r2;
            part = part + k * (s * s);
        }
    };
    auto wall_point = [&](int q) -> V3 { return point(xs, s_wall[q]); };

    // ---- the five terms by their owners, then the tree over the 256 slots
    auto energies = [&](double* out) {
        double e_bond = 0.0, e_angle = 0.0, e_pos = 0.0;
        if (mine) {
            const V3 xu = dpoint(s_x, u);
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = s_adj[u * WORDS + w];
                while (f) {
                    const int v = w * 64 + __builtin_ctzll(f);
                    f &= f - 1;
                    if (v < u || !(mov_u || s_mov[v])) continue;
                    const double l0 = length0(u, v);
                    if (l0 == 0.0) continue;
                    const V3 r = sub(dpoint(s_x, v), xu);
                    const double d = sqrt(dot(r, r));
                    if (d != 0.0) e_bond = e_bond + a.k_bond * ((d - l0) * (d - l0));
                }
            }
            const int terms = s_terms[u];
            if (terms) {
                int nbr[4];
                const int d = first_members(s_adj, u, -1, nbr, 4);
                const double c0 = a.ideal_cos[s_cls[u]];
                for (int q = 1; q < d; ++q) {
                    for (int p = 0; p < q; ++p) {
                        const int j = nbr[p], k = nbr[q];
                        if (!((terms >> pair_bit(p, q)) & 1) || !(mov_u || s_mov[j] || s_mov[k])) continue;
                        Angle g;
                        if (angle_at(xu, dpoint(s_x, j), dpoint(s_x, k), g)) e_angle = e_angle + a.k_angle * ((g.c - c0) * (g.c - c0));
                    }
                }
            }
            if (mov_u) {
                const V3 r = sub(xu, x0);
                e_pos = a.k_pos * dot(r, r);
            }
        }
        for (int o = wave; o < n_kept; o += WG_WAVES) {            // wave-uniform: the far pairs above o, and its wall
            const V3 xo = dpoint(s_x, o);
            const bool mov_o = s_mov[o];
            const int to = s_type[o];
            double part = 0.0;
#pragma unroll
            for (int i = 0; i < WORDS; ++i) {
                const int p = lane + 64 * i;
                if (p > o && p < n_kept && ((s_far[o * WORDS + i] >> lane) & 1ull) && (mov_o || s_mov[p]))
                    pair_energy(sub(xo, dpoint(s_x, p)), a.reach2[to * nf + s_type[p]], a.k_rep, part);
            }
            const double far = wave_tree_sum(part);
            part = 0.0;
            if (mov_o)
                for (int q = lane; q < n_wall; q += 64) pair_energy(sub(xo, wall_point(q)), a.wall_reach2[to * nf + s_wtype[q]], a.k_wall, part);
            const double wall = wave_tree_sum(part);
            if (lane == 0) {
                s_nb[o * 3] = far;
                s_nb[o * 3 + 1] = wall;
            }
        }
        __syncthreads();
        const double e_rep = mine ? s_nb[u * 3] : 0.0, e_wall = mine ? s_nb[u * 3 + 1] : 0.0;
        const double totals[DL_RELAX_TERMS] = {block_tree_sum(e_bond, s_sum), block_tree_sum(e_angle, s_sum), block_tree_sum(e_rep, s_sum),
                                               block_tree_sum(e_wall, s_sum), block_tree_sum(e_pos, s_sum)};
        if (tid == 0) {
#pragma unroll
            for (int t = 0; t < DL_RELAX_TERMS; ++t) out[t] = totals[t];
        }
    };

    energies(energy);

    // ---- the iteration
    const double two_k_bond = 2.0 * a.k_bond, two_k_angle = 2.0 * a.k_angle, two_k_pos = 2.0 * a.k_pos;
    const double four_k_rep = 4.0 * a.k_rep, four_k_wall = 4.0 * a.k_wall;
    const double infinity = __longlong_as_double(0x7ff0000000000000ll);
    const double overflowed = __longlong_as_double(0x7fefffffffffffffll);   // stands for an |F| of +inf in s_red: no sqrt of a finite sum reaches it
    V3 vel = {0.0, 0.0, 0.0};
    double dt = a.dt0, alpha = a.alpha0, f_last = 0.0;
    int n_pos = 0, done = 0;
    bool diverged = false;
    for (int step = 0; step < a.steps; ++step) {
        V3 acc = {0.0, 0.0, 0.0};
        if (mov_u) {                             // the bond and angle terms of u
            const V3 xu = dpoint(s_x, u);
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                u64 f = s_adj[u * WORDS + w];
                while (f) {
                    const int v = w * 64 + __builtin_ctzll(f);
                    f &= f - 1;
                    const double l0 = length0(u, v);
                    if (l0 == 0.0) continue;
                    const V3 r = sub(dpoint(s_x, v), xu);
                    const double d = sqrt(dot(r, r));
                    if (d == 0.0) continue;
                    const double g = (two_k_bond * (d - l0)) / d;
                    acc = add(acc, times(g, r));
                }
            }
            const int terms = s_terms[u];
            if (terms) {                         // u as the centre, in pair order
                int nbr[4];
                const int d = first_members(s_adj, u, -1, nbr, 4);
                const double c0 = a.ideal_cos[s_cls[u]];
                for (int q = 1; q < d; ++q) {
                    for (int p = 0; p < q; ++p) {
                        V3 f;
                        if (((terms >> pair_bit(p, q)) & 1) && angle_force(xu, dpoint(s_x, nbr[p]), dpoint(s_x, nbr[q]), c0, two_k_angle, 0, f))
                            acc = add(acc, f);
                    }
                }
            }
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {    // u as an end: by centre, then by other end
                u64 f = s_adj[u * WORDS + w];
                while (f) {
                    const int c = w * 64 + __builtin_ctzll(f);
                    f &= f - 1;
                    const int at_c = s_terms[c];
                    if (!at_c) continue;
                    int nbr[4];
                    const int d = first_members(s_adj, c, -1, nbr, 4);
                    int pu = 0;
                    for (int t = 1; t < d; ++t) pu = nbr[t] == u ? t : pu;
                    const double c0 = a.ideal_cos[s_cls[c]];
                    const V3 xc = dpoint(s_x, c);
                    for (int t = 0; t < d; ++t) {
                        if (t == pu) continue;
                        const int lo = min(pu, t), hi = max(pu, t);
                        V3 g;
                        if (((at_c >> pair_bit(lo, hi)) & 1) &&
                            angle_force(xc, dpoint(s_x, nbr[lo]), dpoint(s_x, nbr[hi]), c0, two_k_angle, pu == lo ? 1 : 2, g))
                            acc = add(acc, g);
                    }
                }
            }
        }
        for (int m = wave; m < n_mov; m += WG_WAVES) {           // wave-uniform: the far pairs and the wall of one movable atom
            const int o = s_movable[m], to = s_type[o];
            const V3 xo = dpoint(s_x, o);
            V3 part = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < WORDS; ++i) {
                const int p = lane + 64 * i;
                if (p < n_kept && ((s_far[o * WORDS + i] >> lane) & 1ull)) {
                    const int tp = s_type[p];
                    pair_force(sub(xo, dpoint(s_x, p)), a.reach2[o < p ? to * nf + tp : tp * nf + to], four_k_rep, part);
                }
            }
            const V3 far = wave_tree_sum(part);
            part = {0.0, 0.0, 0.0};
            for (int q = lane; q < n_wall; q += 64) pair_force(sub(xo, wall_point(q)), a.wall_reach2[to * nf + s_wtype[q]], four_k_wall, part);
            const V3 wall = wave_tree_sum(part);
            if (lane == 0) {
                const V3 both = add(far, wall);
                s_nb[o * 3] = both.x;
                s_nb[o * 3 + 1] = both.y;
                s_nb[o * 3 + 2] = both.z;
            }
        }
        __syncthreads();

        V3 F = {0.0, 0.0, 0.0};
        double top = 0.0;
        if (mov_u) {
            const V3 xu = dpoint(s_x, u);
            F = add(add(acc, dpoint(s_nb, u)), times(two_k_pos, sub(x0, xu)));
            top = sqrt(dot(F, F));                  // the atom's |F|: the same in every frame, which a largest component is not
            if (top == infinity) top = overflowed;  // finite components whose squares overflow: f is +inf, no divergence
            if (nonfinite(F.x) || nonfinite(F.y) || nonfinite(F.z)) top = infinity;
        }
        // F.v, F.F, v.v by the tree and the largest |F|, in one pass over s_red
        const double w_p = wave_tree_sum(dot(F, vel)), w_ff = wave_tree_sum(dot(F, F)), w_vv = wave_tree_sum(dot(vel, vel));
        const double w_top = wave_max(top);
        if (lane == 0) {
            s_red[wave * 4] = w_p;
            s_red[wave * 4 + 1] = w_ff;
            s_red[wave * 4 + 2] = w_vv;
            s_red[wave * 4 + 3] = w_top;
        }
        __syncthreads();
        const double P = (s_red[0] + s_red[4]) + (s_red[8] + s_red[12]);
        const double ff = (s_red[1] + s_red[5]) + (s_red[9] + s_red[13]);
        const double vv = (s_red[2] + s_red[6]) + (s_red[10] + s_red[14]);
        double f_now = s_red[3];
#pragma unroll
        for (int k = 1; k < WG_WAVES; ++k) f_now = s_red[k * 4 + 3] > f_now ? s_red[k * 4 + 3] : f_now;
        if (f_now == infinity) {                 // uniform, as everything decided from s_red
            diverged = true;
            break;
        }
        f_last = f_now == overflowed ? infinity : f_now;
        if (f_now < a.f_tol) break;
        if (P > 0.0) {
            ++n_pos;
            const double keep = 1.0 - alpha, mix = (alpha * sqrt(vv)) / sqrt(ff);
            if (mov_u) vel = add(times(keep, vel), times(mix, F));
            if (n_pos > a.n_min) {
                const double longer = dt * a.f_inc;
                dt = longer < a.dt_max ? longer : a.dt_max;
                alpha = alpha * a.f_alpha;
            }
        } else {
            n_pos = 0;
            vel = {0.0, 0.0, 0.0};
            dt = dt * a.f_dec;
            alpha = a.alpha0;
        }
        if (mov_u) {
            vel = add(vel, times(dt, F));
            V3 s = times(dt, vel);
            const double length = sqrt(dot(s, s));
            if (length > a.max_step) s = times(a.max_step / length, s);
            const V3 moved = add(dpoint(s_x, u), s);
            s_x[u * 3] = moved.x;
            s_x[u * 3 + 1] = moved.y;
            s_x[u * 3 + 2] = moved.z;
        }
        ++done;
        __syncthreads();                         // the new positions, and s_red free again
    }
    {
        int bad = 0;
        if (mov_u) bad = nonfinite(s_x[u * 3]) || nonfinite(s_x[u * 3 + 1]) || nonfinite(s_x[u * 3 + 2]);
        diverged = __syncthreads_or(bad) || diverged;
    }
    if (diverged) {
        leave(status0 | DL_RELAX_DIVERGED, done, true);
        return;
    }

    energies(energy + DL_RELAX_TERMS);
    double far2 = 0.0;
    if (mov_u) {
        const V3 r = sub(dpoint(s_x, u), x0);
        far2 = dot(r, r);
    }
    far2 = block_max(far2, s_sum);
    for (int k = tid; k < N; k += WG) {          // every row but the movable ones, which their threads write below
        if (mask[k] != 0.0f && !(drop && drop[k] != 0.0f) && (!mark || mark[k] != 0.0f)) continue;
#pragma unroll
        for (int d = 0; d < 3; ++d) out_bits[k * 3 + d] = x_bits[k * 3 + d];
    }
    if (mov_u) {
        float* row = a.x_out + (size_t(b) * N + s_row[u]) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) row[d] = float(s_x[u * 3 + d]);
    }
    if (tid == 0) {
        a.steps_done[b] = done;
        a.f_max[b] = f_last;
        a.moved2[b] = far2;
        a.status[b] = status0;
    }
}

}  // namespace

extern "C" {

int32_t dl_relax_molecules(const dl_relax_args* a) {
    if (!a || a->B < 0 || a->N < 1 || a->N > MAX_ROWS || a->nf < 1 || a->capacity < 0 || a->steps < 0 || a->steps > DL_RELAX_MAX_STEPS)
        return DL_ERR_BAD_ARG;
    if (a->B == 0) return DL_OK;                 // an empty batch has nothing to point at
    if (!a->x || !a->one_hot || !a->node_mask || !a->length0 || !a->aromatic_length0 || !a->ideal_cos || !a->reach2 ||
        !a->wall_reach2 || !a->n_bonds_in || !a->x_out || !a->energy || !a->steps_done || !a->f_max || !a->moved2 || !a->status ||
        (a->capacity > 0 && !a->bonds))
        return DL_ERR_BAD_ARG;
    hipLaunchKernelGGL(relax_kernel, dim3(a->B), dim3(WG), 0, static_cast<hipStream_t>(a->stream), *a);
    return hipGetLastError() == hipSuccess ? DL_OK : DL_ERR_HIP;
}

}  // extern "C"
