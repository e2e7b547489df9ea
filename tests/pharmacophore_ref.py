"""Plain Python restatement of ``csrc/pharmacophore.hip`` (pharmacophore features and the Best-mode feature-map match), used by
tests only.  Python integers and sets for the graph, numpy fp64 for the centroid and numpy fp32 for ``d2``; no package import:
it shares nothing with the kernels or with ``difflinker_amd.metrics`` but the definitions written in
``include/difflinker_hip.h``.  The rule is this project's own, after RDKit's ``BaseFeatures.fdef`` and ``FeatMapParams``
defaults, and NOT RDKit's numbers.
"""
import math

import numpy as np

MAX_ATOMS, MAX_RINGS, FAMILIES = 256, 64, 7
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, MANY_RINGS, OVERFLOW, NONFINITE = 1, 4, 8, 16, 32, 64
DONOR, ACCEPTOR, POSITIVE, NEGATIVE, HYDROPHOBE, AROMATIC, LUMPED = range(FAMILIES)
C, N, O, S, P, F, HALOGEN = range(1, 8)
# the vocabularies of ``difflinker_amd.const`` (C O N F S Cl Br I [P]) restated, so that the tables there are held to these
FEATURE_CLASS = (C, O, N, F, S, HALOGEN, HALOGEN, HALOGEN, P)
DEFAULT_VALENCE = (4, 2, 3, 1, 2, 1, 1, 1, 3)
FIELDS = ('family', 'anchor', 'position', 'marked', 'n_features', 'family_count', 'status')
MATCH_FIELDS = ('best_index', 'best_d2', 'n_a', 'n_b', 'n_matched')


TYPE = {'C': 0, 'O': 1, 'N': 2, 'F': 3, 'S': 4, 'Cl': 5, 'Br': 6, 'I': 7, 'P': 8}


def ring(first, size, doubles):
    """The bonds ``(i, j, order, aromatic)`` of an aromatic ring of atoms ``first .. first + size - 1``; ``doubles`` names the
    positions k whose bond (k, k + 1 mod size) has order 2."""
    return [(first + k, first + (k + 1) % size, 2 if k in doubles else 1, 1) for k in range(size)]


# Hand-built molecules: symbols, bonds (i, j, order, aromatic) with Kekule orders written out, and the feature list that the
# rule of include/difflinker_hip.h gives, worked out by hand, as (family, anchor) in the list's order
EXAMPLES = {
    # CH3-C(=O)-OH: the acid carbon carries the negative centre; =O accepts, -OH donates and accepts
    'acetic acid': ('C C O O'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 1, 0)],
                    [(HYDROPHOBE, 0), (NEGATIVE, 1), (ACCEPTOR, 2), (DONOR, 3), (ACCEPTOR, 3)]),
    # the carboxylate as the distance table may read it: two C=O
    'acetate': ('C C O O'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 2, 0)],
                [(HYDROPHOBE, 0), (NEGATIVE, 1), (ACCEPTOR, 2), (ACCEPTOR, 3)]),
    # CH3-S(=O)(=O)-CH3: two terminal oxygens on S are not enough
    'dimethyl sulfone': ('C S O O C'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 2, 0), (1, 4, 1, 0)],
                         [(ACCEPTOR, 2), (ACCEPTOR, 3)]),
    # CH3-S(=O)(=O)-OH
    'methanesulfonate': ('C S O O O'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 2, 0), (1, 4, 1, 0)],
                         [(NEGATIVE, 1), (ACCEPTOR, 2), (ACCEPTOR, 3), (DONOR, 4), (ACCEPTOR, 4)]),
    'trimethylamine': ('N C C C'.split(), [(0, 1, 1, 0), (0, 2, 1, 0), (0, 3, 1, 0)], [(ACCEPTOR, 0), (POSITIVE, 0)]),
    # CH3-C(=O)-N(CH3)2: the amide N neither accepts nor ionizes
    'dimethylacetamide': ('C C O N C C'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 1, 0), (3, 4, 1, 0), (3, 5, 1, 0)],
                          [(HYDROPHOBE, 0), (ACCEPTOR, 2)]),
    # the ring 0..5, NH2 on atom 0: the N donates and does not accept
    'aniline': ('C C C C C C N'.split(), ring(0, 6, (0, 2, 4)) + [(0, 6, 1, 0)],
                [(HYDROPHOBE, k) for k in range(1, 6)] + [(DONOR, 6), (AROMATIC, 0), (LUMPED, 0)]),
    'pyridine': ('N C C C C C'.split(), ring(0, 6, (0, 2, 4)),
                 [(ACCEPTOR, 0), (HYDROPHOBE, 2), (HYDROPHOBE, 3), (HYDROPHOBE, 4), (AROMATIC, 0)]),
    'pyrrole': ('N C C C C'.split(), ring(0, 5, (1, 3)), [(DONOR, 0), (HYDROPHOBE, 2), (HYDROPHOBE, 3), (AROMATIC, 0)]),
    'furan': ('O C C C C'.split(), ring(0, 5, (1, 3)), [(HYDROPHOBE, 2), (HYDROPHOBE, 3), (AROMATIC, 0)]),
    'benzene': ('C C C C C C'.split(), ring(0, 6, (0, 2, 4)),
                [(HYDROPHOBE, k) for k in range(6)] + [(AROMATIC, 0), (LUMPED, 0)]),
    'chlorobenzene': ('C C C C C C Cl'.split(), ring(0, 6, (0, 2, 4)) + [(0, 6, 1, 0)],
                      [(HYDROPHOBE, k) for k in range(1, 7)] + [(AROMATIC, 0), (LUMPED, 0)]),
    # CH3-C(=NH)-NH2: the positive centre sits on the carbon
    'acetamidine': ('C C N N'.split(), [(0, 1, 1, 0), (1, 2, 2, 0), (1, 3, 1, 0)],
                    [(HYDROPHOBE, 0), (POSITIVE, 1), (DONOR, 2), (DONOR, 3)]),
    # rings 0..5 and 4, 5, 6..9 fused at the bond 4-5; the ten-ring around both is no five- or six-ring
    'naphthalene': (['C'] * 10,
                    [(0, 1, 2, 1), (1, 2, 1, 1), (2, 3, 2, 1), (3, 4, 1, 1), (4, 5, 2, 1), (5, 0, 1, 1), (5, 6, 1, 1), (6, 7, 2, 1),
                     (7, 8, 1, 1), (8, 9, 2, 1), (9, 4, 1, 1)],
                    [(HYDROPHOBE, k) for k in range(10)] + [(AROMATIC, 0), (LUMPED, 0), (AROMATIC, 4), (LUMPED, 4)]),
}


def as_batch(molecules, N=None, capacity=None, seed=0):
    """The arrays ``features`` takes for a list of ``(symbols, bonds)``: one molecule per row of the batch, GEOM vocabulary,
    coordinates drawn from ``seed`` (no rule here reads a distance: the kernel reads the list)."""
    rng = np.random.default_rng(seed)
    B = len(molecules)
    N = N or max(len(symbols) for symbols, _ in molecules)
    capacity = capacity or max(max(len(bonds) for _, bonds in molecules), 1)
    out = {'one_hot': np.zeros((B, N, len(TYPE)), np.float32), 'x': rng.normal(0, 2, (B, N, 3)).astype(np.float32),
           'node_mask': np.zeros((B, N), np.float32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_bonds_in': np.zeros(B, np.int32), 'bond_aromatic': np.zeros((B, capacity), np.int32),
           'status_in': np.zeros(B, np.int32)}
    for b, (symbols, bonds) in enumerate(molecules):
        for k, symbol in enumerate(symbols):
            out['one_hot'][b, k, TYPE[symbol]] = 1
            out['node_mask'][b, k] = 1
        out['n_bonds_in'][b] = len(bonds)
        for e, (i, j, order, aromatic) in enumerate(bonds):
            out['bonds'][b, e] = (i, j, order)
            out['bond_aromatic'][b, e] = aromatic
    return out


def batch_features(arrays, Fcap, drop_mask=None, mark_mask=None):
    """``features`` of the arrays of ``as_batch`` with the tables of this file."""
    return features(arrays['one_hot'], arrays['x'], arrays['node_mask'], arrays['bonds'], arrays['n_bonds_in'],
                    arrays['bond_aromatic'], arrays['status_in'], FEATURE_CLASS, DEFAULT_VALENCE, Fcap, drop_mask, mark_mask)


def aromatic_rings(n, pairs, aromatic):
    """The chordless 5- and 6-cycles of aromatic pairs among atoms ``0..n-1`` in canonical order, sorted.  ``pairs`` and
    ``aromatic`` are sets of ``(lo, hi)``; ring atoms have two or three aromatic pairs."""
    near = [set() for _ in range(n)]
    for u, v in aromatic:
        near[u].add(v)
        near[v].add(u)
    ring_atom = [len(near[u]) in (2, 3) for u in range(n)]
    joined = lambda u, v: (min(u, v), max(u, v)) in pairs      # noqa: E731
    found = []

    def walk(path):
        last = path[-1]
        if len(path) >= 5 and path[0] in near[last] and path[1] < last:
            k = len(path)
            chords = [(p, q) for p in range(k) for q in range(p + 2, k) if not (p == 0 and q == k - 1)]
            if not any(joined(path[p], path[q]) for p, q in chords):
                found.append(tuple(path))
        if len(path) == 6:
            return
        for t in sorted(near[last]):
            if t > path[0] and ring_atom[t] and t not in path:
                walk(path + [t])

    for s in range(n):
        if ring_atom[s]:
            walk([s])
    return sorted(found)


def molecule_features(classes, valences, pairs, x, marks):
    """The feature list of one molecule whose atoms are all kept: ``classes`` and ``valences`` (default valence) per atom,
    ``pairs`` a dict ``(lo, hi) -> (order, aromatic)``, ``x`` fp32 ``[n,3]``, ``marks`` per atom.  Returns
    ``(features, n_rings_found)`` with ``features`` a list of ``(family, anchor atom, position fp32 [3], marked)`` in the list's
    order; more than ``MAX_RINGS`` rings leave the ring features out."""
    n = len(classes)
    near = [set() for _ in range(n)]
    for u, v in pairs:
        near[u].add(v)
        near[v].add(u)
    order = lambda u, v: pairs[(min(u, v), max(u, v))][0]       # noqa: E731
    deg = [len(near[u]) for u in range(n)]
    val = [sum(order(u, v) for v in near[u]) for u in range(n)]
    h = [max(0, valences[u] - val[u]) for u in range(n)]
    arom = [any(pairs[(min(u, v), max(u, v))][1] for v in near[u]) for u in range(n)]
    multi = [any(order(u, v) >= 2 for v in near[u]) for u in range(n)]
    features = []
    for u in range(n):
        c = classes[u]
        quiet = not any(arom[w] or multi[w] for w in near[u])
        all_c = all(classes[w] == C for w in near[u])
        fam = []
        if c in (N, O) and h[u] >= 1:
            fam.append(DONOR)
        if (c == O and not arom[u] and val[u] <= 2) or \
                (c == N and h[u] == 0 and val[u] <= 3 and (multi[u] or (deg[u] == 3 and not arom[u] and quiet))):
            fam.append(ACCEPTOR)
        amine = c == N and not arom[u] and not multi[u] and val[u] <= 3 and deg[u] >= 1 and all_c and quiet
        double = [w for w in near[u] if order(u, w) == 2]
        amidine = (c == C and not arom[u] and len(double) == 1 and classes[double[0]] == N
                   and not any(order(u, w) == 3 for w in near[u])
                   and any(classes[w] == N and order(u, w) == 1 for w in near[u])
                   and not any(classes[w] in (O, S) for w in near[u]))
        if amine or amidine:
            fam.append(POSITIVE)
        terminal = [w for w in near[u] if classes[w] == O and deg[w] == 1]
        if any(order(u, w) == 2 for w in terminal) and \
                ((c in (C, P) and len(terminal) >= 2) or (c == S and len(terminal) >= 3)):
            fam.append(NEGATIVE)
        if (c == C and deg[u] >= 1 and all_c) or (c == HALOGEN and deg[u] == 1) or \
                (c == S and deg[u] == 2 and not multi[u] and not arom[u] and all_c):
            fam.append(HYDROPHOBE)
        features += [(f, u, x[u].copy(), int(bool(marks[u]))) for f in fam]
    rings = aromatic_rings(n, set(pairs), {p for p, (_, a) in pairs.items() if a})
    if len(rings) <= MAX_RINGS:
        for ring in rings:
            total = x[ring[0]].astype(np.float64)
            for u in ring[1:]:
                total = total + x[u].astype(np.float64)
            centre = (total / np.float64(len(ring))).astype(np.float32)
            mark = int(all(marks[u] for u in ring))
            features.append((AROMATIC, ring[0], centre, mark))
            if all(classes[u] == C for u in ring):
                features.append((LUMPED, ring[0], centre, mark))
    return features, len(rings)


def features(one_hot, x, node_mask, bonds, n_bonds_in, bond_aromatic, status_in, feature_class, default_valence, Fcap,
             drop_mask=None, mark_mask=None):
    """Every output of ``dl_pharmacophore_features`` for arrays laid out as ``dl_pharm_args`` takes them: ``one_hot [B,N,nf]``,
    ``x [B,N,3]`` fp32, masks ``[B,N]``, ``bonds [B,capacity,3]``, ``bond_aromatic [B,capacity]``, ``n_bonds_in`` and
    ``status_in`` ``[B]``."""
    B, rows_n = node_mask.shape
    capacity = bonds.shape[1]
    x = np.asarray(x, np.float32)
    out = {'family': np.full((B, Fcap), -1, np.int32), 'anchor': np.full((B, Fcap), -1, np.int32),
           'position': np.zeros((B, Fcap, 3), np.float32), 'marked': np.zeros((B, Fcap), np.int32),
           'n_features': np.zeros(B, np.int32), 'family_count': np.zeros((B, FAMILIES), np.int32), 'status': np.zeros(B, np.int32)}
    for b in range(B):
        rows = [r for r in range(rows_n) if node_mask[b, r] != 0]
        n = len(rows)
        keep = [drop_mask is None or not drop_mask[b, r] != 0 for r in rows]
        n_in = int(n_bonds_in[b])
        status = int(status_in[b]) | (BONDS_OVERFLOW if n_in > capacity else 0)
        if sum(keep) > MAX_ATOMS:
            out['status'][b] = status | TOO_LARGE
            continue
        kept = [k for k in range(n) if keep[k]]                         # kept index -> atom number
        number = {k: q for q, k in enumerate(kept)}
        types = [max(range(one_hot.shape[2]), key=lambda c: (one_hot[b, rows[k], c], -c)) for k in kept]     # the first maximum
        classes = [int(feature_class[t]) if 1 <= int(feature_class[t]) <= 7 else 0 for t in types]
        valences = [int(default_valence[t]) for t in types]
        marks = [mark_mask is not None and mark_mask[b, rows[k]] != 0 for k in kept]
        xs = np.stack([x[b, rows[k]] for k in kept]) if kept else np.zeros((0, 3), np.float32)
        pairs = {}
        for e, (i, j, o) in enumerate(bonds[b, :min(max(n_in, 0), capacity)].tolist()):
            if not (0 <= i < n and 0 <= j < n and i != j and 1 <= o <= 3):
                status |= BAD_BOND
                continue
            if not (keep[i] and keep[j]):
                continue
            pair = (min(number[i], number[j]), max(number[i], number[j]))
            if pair in pairs:
                status |= BAD_BOND                                      # the first entry of the pair has decided
            else:
                pairs[pair] = (o, bool(bond_aromatic[b, e] != 0))
        listed, n_rings = molecule_features(classes, valences, pairs, xs, marks)
        if n_rings > MAX_RINGS:
            status |= MANY_RINGS
        if not np.isfinite(xs).all():
            status |= NONFINITE
        if len(listed) > Fcap:
            status |= OVERFLOW
        for f, (fam, anchor, position, marked) in enumerate(listed):
            out['family_count'][b, fam] += 1
            if f < Fcap:
                out['family'][b, f], out['anchor'][b, f], out['marked'][b, f] = fam, kept[anchor], marked
                out['position'][b, f] = position
        out['n_features'][b], out['status'][b] = len(listed), status
    return out


def feature_match(family_a, position_a, marked_a, n_features_a, family_b, position_b, marked_b, n_features_b, radius2,
                  marked_only=False):
    """Every output of ``dl_feature_match``: lists ``[B,Fa]`` / ``[B,Fb]`` (positions ``[..,3]`` fp32), counts ``[B]``,
    ``radius2`` an fp32 value."""
    B, Fa = family_a.shape
    Fb = family_b.shape[1]
    radius2 = np.float32(radius2)
    position_a, position_b = np.asarray(position_a, np.float32), np.asarray(position_b, np.float32)
    out = {'best_index': np.full((B, Fb), -1, np.int32), 'best_d2': np.full((B, Fb), np.inf, np.float32),
           'n_a': np.zeros(B, np.int32), 'n_b': np.zeros(B, np.int32), 'n_matched': np.zeros(B, np.int32)}
    part = lambda fam, mk: 0 <= fam < FAMILIES and not (marked_only and mk == 0)      # noqa: E731
    for b in range(B):
        in_a = [i for i in range(min(max(int(n_features_a[b]), 0), Fa)) if part(family_a[b, i], marked_a[b, i])]
        in_b = [j for j in range(min(max(int(n_features_b[b]), 0), Fb)) if part(family_b[b, j], marked_b[b, j])]
        out['n_a'][b], out['n_b'][b] = len(in_a), len(in_b)
        for j in in_b:
            best, best_i = np.float32(np.inf), -1
            for i in in_a:
                if family_a[b, i] != family_b[b, j]:
                    continue
                with np.errstate(all='ignore'):
                    d = position_a[b, i] - position_b[b, j]                            # fp32, every operation rounded on its own
                    d2 = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])
                if d2 < radius2 and d2 < best:
                    best, best_i = d2, i
            out['best_index'][b, j], out['best_d2'][b, j] = best_i, best
            out['n_matched'][b] += best_i >= 0
    return out


def feature_score(best_d2, n_a, n_b):
    """``sum_j exp(-best_d2_j) / min(n_a, n_b)`` over the matched features in index order, fp64; ``None`` without features."""
    if min(n_a, n_b) == 0:
        return None
    return sum(math.exp(-float(d)) for d in best_d2 if math.isfinite(float(d))) / min(n_a, n_b)
