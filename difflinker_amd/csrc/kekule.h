// kekule.h — the Kekule assignment of one ring system of aromatic.hip, for one thread: at most 32 atoms, the graph as one
// 32-bit neighbour mask per atom.  Plain C++ without a HIP construct beyond the DL_HD marker, so a host program can run it.
// The arrays the searches index at run time live in a workspace of WORDS ints that the caller provides: LDS in the kernel,
// where one lane's chain of dependent look-ups costs a tenth of what it costs in scratch memory.
//
// THE TASK (include/difflinker_hip.h, "6. Kekule assignment").  Among the matchings of the graph over the atoms of `can`
// (roles P and F): cover the most atoms of `heavy` (role P), then the most other atoms (role F), then take the matching whose
// sorted list of (min, max) pairs is lexicographically smallest.  Atoms are numbered in ascending order of their atom number,
// so local order is atom order.
//
// HOW.  improve(alive) leaves a matching of the alive atoms of the largest weight 64 * P + F, by the characterisation of
// vertex-weighted matchings: a matching is heaviest exactly when it has no augmenting path and no alternating path of even
// length from an uncovered atom to a covered atom of smaller weight.  Augmenting paths are found by Edmonds' blossom search
// (a breadth-first search with contracted odd cycles: five-rings are odd); an even path from an uncovered P atom v to a
// covered F atom w is found by taking w and its pair out and looking for an augmenting path from v, which can only end at
// w's former partner.  Every augmentation adds a pair and every swap adds a covered P atom, so the loop ends.
// All heaviest matchings have the same number of pairs, so the smallest list is found pair by pair: walk the bonds in sorted
// order; a bond of the current heaviest matching is fixed (no smaller bond is in any heaviest matching that holds the fixed
// ones - each was tried); any other bond is fixed when a heaviest matching of the rest without its two atoms, repaired from
// the current one, loses no weight.
#ifndef DL_KEKULE_H
#define DL_KEKULE_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DL_HD __host__ __device__ __forceinline__
#else
#define DL_HD inline
#endif

namespace kekule {

constexpr int MAXV = 32;
using mask_t = unsigned int;

DL_HD int lowest(mask_t m) { return __builtin_ctz(m); }

constexpr int WORDS = 6 * MAXV;                 // ints of workspace per system: adj, two matchings, par, base, queue

struct Search {
    const mask_t* adj;      // neighbour masks, already restricted to matchable atoms
    int n;                  // atoms of the system: the arrays are used up to here
    int* match;             // partner or -1
    int* par;               // scratch of one search, shared by the two matchings: one search runs at a time
    int* base;
    int* queue;
};

DL_HD int lca(const Search& s, int a, int b) {
    mask_t seen = 0;
    for (;;) {
        a = s.base[a];
        seen |= 1u << a;
        if (s.match[a] < 0) break;
        a = s.par[s.match[a]];
    }
    for (;;) {
        b = s.base[b];
        if (seen >> b & 1) return b;
        b = s.par[s.match[b]];
    }
}

DL_HD void mark_path(Search& s, mask_t& blossom, int v, int b, int child) {
    while (s.base[v] != b) {
        blossom |= 1u << s.base[v];
        blossom |= 1u << s.base[s.match[v]];
        s.par[v] = child;
        child = s.match[v];
        v = s.par[s.match[v]];
    }
}

// an augmenting path from the uncovered atom `root` over the atoms of `alive`; flips it and returns true when there is one
DL_HD bool augment(Search& s, mask_t alive, int root) {
    for (int i = 0; i < s.n; ++i) { s.par[i] = -1; s.base[i] = i; }
    int* queue = s.queue;
    int head = 0, tail = 0;
    mask_t used = 1u << root;
    queue[tail++] = root;
    int end = -1;
    while (head < tail && end < 0) {
        const int v = queue[head++];
        mask_t nb = s.adj[v] & alive;
        while (nb && end < 0) {
            const int to = lowest(nb);
            nb &= nb - 1;
            if (s.base[v] == s.base[to] || s.match[v] == to) continue;
            if (to == root || (s.match[to] >= 0 && s.par[s.match[to]] >= 0)) {
                const int cur = lca(s, v, to);
                mask_t blossom = 0;
                mark_path(s, blossom, v, cur, to);
                mark_path(s, blossom, to, cur, v);
                for (int i = 0; i < s.n; ++i) {
                    if (!(alive >> i & 1) || !(blossom >> s.base[i] & 1)) continue;
                    s.base[i] = cur;
                    if (!(used >> i & 1)) { used |= 1u << i; queue[tail++] = i; }
                }
            } else if (s.par[to] < 0) {
                s.par[to] = v;
                if (s.match[to] < 0) { end = to; break; }
                if (!(used >> s.match[to] & 1)) { used |= 1u << s.match[to]; queue[tail++] = s.match[to]; }
            }
        }
    }
    if (end < 0) return false;
    for (int v = end; v >= 0;) {
        const int pv = s.par[v], next = s.match[pv];
        s.match[v] = pv;
        s.match[pv] = v;
        v = next;
    }
    return true;
}

DL_HD int weight(const Search& s, mask_t alive, mask_t heavy) {
    int w = 0;
    for (mask_t m = alive; m; m &= m - 1) {
        const int v = lowest(m);
        if (s.match[v] >= 0) w += (heavy >> v & 1) ? 64 : 1;
    }
    return w;
}

// turns the matching s.match of the atoms of `alive` (any matching: -1 everywhere else) into a heaviest one.  The fixed point
// is heaviest whatever the start was, so a matching that lost two atoms is repaired with a few searches
DL_HD void improve(Search& s, mask_t alive, mask_t heavy) {
    for (;;) {
        bool changed = false;
        for (mask_t m = alive; m; m &= m - 1) {
            const int v = lowest(m);
            if (s.match[v] < 0 && augment(s, alive, v)) changed = true;
        }
        if (changed) continue;                   // until no augmenting path is left
        for (mask_t m = alive & heavy; m && !changed; m &= m - 1) {
            const int v = lowest(m);
            if (s.match[v] >= 0) continue;
            for (mask_t l = alive & ~heavy; l && !changed; l &= l - 1) {
                const int w = lowest(l), partner = s.match[w];
                if (partner < 0) continue;
                s.match[w] = s.match[partner] = -1;
                if (augment(s, alive & ~(1u << w), v)) changed = true;
                else { s.match[w] = partner; s.match[partner] = w; }
            }
        }
        if (!changed) return;
    }
}

// the assignment: mate[v] = partner or -1 for the n atoms (entries from n on are not written).  The first MAXV words of the
// workspace `ws` hold the neighbour masks on entry: adj[v] must hold only atoms of `can`, and be 0 outside `can`
DL_HD void assign(int* ws, int n, mask_t can, mask_t heavy, int* mate) {
    const mask_t* adj = reinterpret_cast<const mask_t*>(ws);
    Search cur, trial;
    cur.adj = trial.adj = adj;
    cur.n = trial.n = n;
    cur.match = ws + MAXV;
    trial.match = ws + 2 * MAXV;
    cur.par = trial.par = ws + 3 * MAXV;
    cur.base = trial.base = ws + 4 * MAXV;
    cur.queue = trial.queue = ws + 5 * MAXV;
    for (int i = 0; i < n; ++i) mate[i] = -1;
    mask_t alive = can;
    for (int i = 0; i < n; ++i) cur.match[i] = -1;
    improve(cur, alive, heavy);
    for (int u = 0; u < n; ++u) {
        mask_t nb = (alive >> u & 1) ? adj[u] & ~((2u << u) - 1u) : 0u;      // neighbours above u
        while (nb && (alive >> u & 1)) {
            const int v = lowest(nb);
            nb &= nb - 1;
            if (!(alive >> v & 1)) continue;
            const mask_t rest = alive & ~(1u << u) & ~(1u << v);
            bool fix = cur.match[u] == v;
            if (!fix) {
                for (int i = 0; i < n; ++i) trial.match[i] = cur.match[i];          // the current one without u and v
                if (trial.match[u] >= 0) trial.match[trial.match[u]] = -1;
                if (trial.match[v] >= 0) trial.match[trial.match[v]] = -1;
                trial.match[u] = trial.match[v] = -1;
                improve(trial, rest, heavy);
                const int pair = ((heavy >> u & 1) ? 64 : 1) + ((heavy >> v & 1) ? 64 : 1);
                fix = weight(trial, rest, heavy) + pair == weight(cur, alive, heavy);
                if (fix) for (int i = 0; i < n; ++i) cur.match[i] = trial.match[i];
            } else {
                cur.match[u] = cur.match[v] = -1;
            }
            if (fix) { mate[u] = v; mate[v] = u; alive = rest; }
        }
    }
}

}  // namespace kekule

#endif
