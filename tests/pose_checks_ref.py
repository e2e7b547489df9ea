"""The internal-geometry rule of ``dl_pose_checks`` (``include/difflinker_hip.h``, ``csrc/pose_checks.hip``) restated in plain
Python: bond lengths against squared bounds, bond angles against the cosines of the centre's class, and clashes between atoms
with no path of three or fewer bonds between them.  Python floats are IEEE doubles and are never contracted, so every
operation below is rounded on its own in the header's order and the kernel must agree in every output bit.

Atom ``k`` is the k-th row with ``node_mask != 0``; ``drop_mask`` removes atoms after that numbering; an entry
``(i, j, order)`` is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 3``, in either orientation.  It is this
project's own rule after the idea of PoseBusters' intramolecular checks, and it is NOT PoseBusters.

Below the rule: the three tables, a distance-table bond perception for molecules read from files, molecules whose answer is
known by hand, ties on coordinates that are exact in fp32, and builders of random molecules and of batches."""
import math

import numpy as np

MAX_ATOMS = 256
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, NONFINITE = 1, 4, 8, 64
CHECKED, UNTABLED, SHORT, LONG, ANGLES, BAD_ANGLES, PAIRS, CLASHES = range(8)
LINEAR, TRIGONAL, TETRAHEDRAL = 0, 1, 2
FLAG_BOND, FLAG_ANGLE, FLAG_CLASH = 1, 2, 4
IDEALS = (180.0, 120.0, math.degrees(math.acos(-1.0 / 3.0)))
FIELDS = ('counts', 'atom_flags', 'status')
ATOM2IDX = {'C': 0, 'O': 1, 'N': 2, 'F': 3, 'S': 4, 'Cl': 5, 'Br': 6, 'I': 7}
C, O, N_, F, S = (ATOM2IDX[s] for s in ('C', 'O', 'N', 'F', 'S'))


# ---- the tables the host hands to the kernel ---------------------------------------------------------------------------------
def length_bounds2(nf=8, lo=0.75, hi=1.25):
    """``[nf][nf][3][2]``: ``((lo * L0) ** 2, (hi * L0) ** 2)`` of the typical lengths, ``(0, 0)`` without one."""
    from difflinker_amd.const import BOND_LENGTHS
    out = [[[[0.0, 0.0] for _ in range(3)] for _ in range(nf)] for _ in range(nf)]
    for k in range(3):
        for s in range(nf):
            for t in range(nf):
                if BOND_LENGTHS[k][s][t]:
                    length = BOND_LENGTHS[k][s][t] / 100.0
                    out[s][t][k] = [(lo * length) * (lo * length), (hi * length) * (hi * length)]
    return out


def angle_cos(tolerance=25.0):
    """``[3][2]``: ``cos(theta0 + tol)`` (-2 from 180 degrees on) and ``cos(theta0 - tol)`` (2 down from 0)."""
    return [[math.cos(math.radians(t + tolerance)) if t + tolerance < 180.0 else -2.0,
             math.cos(math.radians(t - tolerance)) if t - tolerance > 0.0 else 2.0] for t in IDEALS]


def clash2(nf=8, scale=0.75):
    from difflinker_amd.const import VDW_RADII
    return [[(scale * (VDW_RADII[s] + VDW_RADII[t])) * (scale * (VDW_RADII[s] + VDW_RADII[t])) for t in range(nf)]
            for s in range(nf)]


def default_tables(nf=8):
    return length_bounds2(nf), angle_cos(), clash2(nf)


# ---- the arithmetic: one rounding per operation ------------------------------------------------------------------------------
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cosine(u, v):
    """``(u . v) / sqrt((u . u) * (v . v))`` with IEEE results where Python raises: 0 / 0 is NaN."""
    with np.errstate(all='ignore'):
        return float(np.float64(dot(u, v)) / np.sqrt(np.float64(dot(u, u) * dot(v, v))))


def angle_class(d, n2, n3, planar):
    if d == 2 and (n3 >= 1 or n2 == 2):
        return LINEAR
    if (d <= 3 and n2 >= 1) or planar:
        return TRIGONAL
    return TETRAHEDRAL


def molecule(x, types, mask, entries, n_bonds_in, bounds2, cosines, clashes2, status_in=0, drop=None, mark=None, planar=None,
             detail=None):
    """One molecule: ``x [N][3]`` float32, ``types [N]``, ``mask`` / ``drop`` / ``mark`` ``[N]`` by row, ``entries`` the
    ``capacity`` rows of its list, ``planar [N]`` by atom number.  Returns ``(counts [2][8], atom_flags [N] by atom number,
    status)``.  ``detail``, a dict, receives the items found: ``bonds`` ``(a, j, order, d2, verdict)``, ``angles``
    ``(j, a, k, class, cosine, bad)``, ``pairs`` ``(a, b, d2, clash)``."""
    N, capacity = len(mask), len(entries)
    real = [r for r in range(N) if mask[r] != 0]
    n = len(real)
    kept = [not (drop is not None and drop[r] != 0) for r in real]
    marked = [mark is not None and mark[r] != 0 for r in real]
    counts, flags = [[0] * 8, [0] * 8], [0] * N
    status = int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0)
    if sum(kept) > MAX_ATOMS:
        return counts, flags, status | TOO_LARGE
    pairs, bad = {}, False
    for e in range(min(max(int(n_bonds_in), 0), capacity)):
        i, j, order = (int(v) for v in entries[e])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 3):
            bad = True
            continue
        if not (kept[i] and kept[j]):
            continue
        key = (min(i, j), max(i, j))
        if key in pairs:
            bad = True
            continue
        pairs[key] = order
    status |= BAD_BOND if bad else 0
    pos = {k: tuple(float(x[real[k]][c]) for c in range(3)) for k in range(n) if kept[k]}
    if any(not math.isfinite(v) for p in pos.values() for v in p):
        return counts, flags, status | NONFINITE
    kind = {k: int(types[real[k]]) for k in pos}

    def count(which, *atoms):
        counts[0][which] += 1
        counts[1][which] += any(marked[a] for a in atoms)

    found = {'bonds': [], 'angles': [], 'pairs': []}
    adj = {k: [] for k in pos}
    for (a, j), order in sorted(pairs.items()):
        adj[a].append(j)
        adj[j].append(a)
        lo2, hi2 = bounds2[kind[a]][kind[j]][order - 1]
        if lo2 == 0.0 and hi2 == 0.0:
            count(UNTABLED, a, j)
            found['bonds'].append((a, j, order, None, 'untabled'))
            continue
        count(CHECKED, a, j)
        v = sub(pos[j], pos[a])
        d2 = dot(v, v)
        verdict = 'short' if d2 < lo2 else 'long' if d2 > hi2 else 'ok'
        found['bonds'].append((a, j, order, d2, verdict))
        if verdict != 'ok':
            count(SHORT if verdict == 'short' else LONG, a, j)
            flags[a] |= FLAG_BOND
            flags[j] |= FLAG_BOND
    for a in adj:
        adj[a].sort()
    order_of = lambda a, t: pairs[(min(a, t), max(a, t))]           # noqa: E731
    for a in sorted(pos):
        d = len(adj[a])
        if not 2 <= d <= 4:
            continue
        orders = [order_of(a, t) for t in adj[a]]
        cls = angle_class(d, orders.count(2), orders.count(3), planar is not None and planar[a] != 0)
        for q in range(1, d):
            for p in range(q):
                j, k = adj[a][p], adj[a][q]
                if k in adj[j] or any(t != a for t in adj[j] if t in adj[k]):
                    continue
                count(ANGLES, a, j, k)
                c = cosine(sub(pos[j], pos[a]), sub(pos[k], pos[a]))
                is_bad = c < cosines[cls][0] or c > cosines[cls][1]
                found['angles'].append((j, a, k, cls, c, is_bad))
                if is_bad:
                    count(BAD_ANGLES, a, j, k)
                    flags[a] |= FLAG_ANGLE
    for a in sorted(pos):
        ball = {a}
        for _ in range(3):
            ball |= {t for u in ball for t in adj[u]}
        for b in sorted(pos):
            if b <= a or b in ball:
                continue
            count(PAIRS, a, b)
            v = sub(pos[b], pos[a])
            d2, t2 = dot(v, v), clashes2[kind[a]][kind[b]]
            clash = t2 > 0.0 and d2 < t2
            found['pairs'].append((a, b, d2, clash))
            if clash:
                count(CLASHES, a, b)
                flags[a] |= FLAG_CLASH
                flags[b] |= FLAG_CLASH
    if detail is not None:
        detail.update(found)
    return counts, flags, status


def first_largest(one_hot):
    """Index of the FIRST largest entry of every row (``numpy.argmax`` returns the first of equal maxima)."""
    return np.argmax(np.asarray(one_hot), axis=-1)


def pose_checks(x, one_hot, node_mask, bonds, n_bonds_in, bounds2, cosines, clashes2, status_in=None, drop_mask=None,
                mark_mask=None, atom_planar=None):
    """The whole batch with the entry point's shapes: ``x [B,N,3]`` float32, ``one_hot [B,N,nf]``, ``node_mask [B,N]``,
    ``bonds [B,capacity,3]``.  Returns int32 arrays ``counts [B,2,8]``, ``atom_flags [B,N]`` and ``status [B]``."""
    x, node_mask, bonds = np.asarray(x, dtype=np.float32), np.asarray(node_mask), np.asarray(bonds)
    B, N = node_mask.shape
    types = first_largest(one_hot)
    out = {'counts': np.zeros((B, 2, 8), np.int32), 'atom_flags': np.zeros((B, N), np.int32), 'status': np.zeros(B, np.int32)}
    pick = lambda t, b: None if t is None else np.asarray(t)[b]     # noqa: E731
    for b in range(B):
        counts, flags, status = molecule(x[b], types[b], node_mask[b], bonds[b], int(n_bonds_in[b]), bounds2, cosines, clashes2,
                                         0 if status_in is None else int(status_in[b]), pick(drop_mask, b), pick(mark_mask, b),
                                         pick(atom_planar, b))
        out['counts'][b], out['atom_flags'][b], out['status'][b] = counts, flags, status
    return out


def perceive(types, points, margins=(10, 5, 2)):
    """The distance table's bonds of a molecule read from a file: ``(i, j, order)`` with ``j < i``, from fp64 distances in pm
    against ``BOND_LENGTHS[k] + margins[k]``, the comparisons strict and nested as ``get_bond_order`` nests them."""
    from difflinker_amd.const import BOND_LENGTHS
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    out = []
    for i in range(len(types)):
        for j in range(i):
            d = 100.0 * float(np.sqrt(((p[i] - p[j]) ** 2).sum()))
            order = 0
            for k in range(3):
                length = BOND_LENGTHS[k][types[i]][types[j]]
                if not (length and d < length + margins[k]):
                    break
                order = k + 1
            if order:
                out.append((i, j, order))
    return out


# ---- molecules whose answer is known by hand ---------------------------------------------------------------------------------
TET = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]


def polygon(n, edge):
    r = edge / (2 * math.sin(math.pi / n))
    return [(r * math.cos(2 * math.pi * k / n), r * math.sin(2 * math.pi * k / n), 0.0) for k in range(n)]


def zigzag(n, length=1.54, degrees=IDEALS[2]):
    """``n`` atoms of an all-anti chain in the xy plane."""
    half = math.radians(degrees) / 2
    return [(k * length * math.sin(half), (k % 2) * length * math.cos(half), 0.0) for k in range(n)]


def chain_bonds(n, order=1):
    return [(k + 1, k, order) for k in range(n - 1)]


def _hand():
    """name -> (types, points, entries, planar atoms, expected row 0 of counts)."""
    out = {}
    out['butane'] = ([C] * 4, zigzag(4), chain_bonds(4), [], [3, 0, 0, 0, 2, 0, 0, 0])
    out['hexane'] = ([C] * 6, zigzag(6), chain_bonds(6), [], [5, 0, 0, 0, 4, 0, 3, 0])
    out['benzene'] = ([C] * 6, polygon(6, 1.39), [((k + 1) % 6, k, 2 - k % 2) for k in range(6)], [], [6, 0, 0, 0, 6, 0, 0, 0])
    out['benzene_flagged_planar'] = ([C] * 6, polygon(6, 1.39), [((k + 1) % 6, k, 1) for k in range(6)], list(range(6)),
                                     [6, 0, 0, 0, 6, 0, 0, 0])
    out['propyne'] = ([C, C, C], [(0, 0, 0), (1.20, 0, 0), (2.66, 0, 0)], [(1, 0, 3), (2, 1, 1)], [], [2, 0, 0, 0, 1, 0, 0, 0])
    arm = 1.0 / math.sqrt(3)
    sulfone_points = [(0, 0, 0)] + [tuple(length * arm * v for v in t) for t, length in zip(TET, (1.80, 1.80, 1.45, 1.45))]
    out['sulfone'] = ([S, C, C, O, O], sulfone_points, [(1, 0, 1), (2, 0, 1), (3, 0, 2), (4, 0, 2)], [],
                      [2, 2, 0, 0, 6, 0, 0, 0])                   # the reference has no S=O length: two untabled bonds
    out['cyclopropane'] = ([C] * 3, polygon(3, 1.51), [((k + 1) % 3, k, 1) for k in range(3)], [], [3, 0, 0, 0, 0, 0, 0, 0])
    out['cyclobutane'] = ([C] * 4, polygon(4, 1.55), [((k + 1) % 4, k, 1) for k in range(4)], [], [4, 0, 0, 0, 0, 0, 0, 0])
    bent = [(1.46 * math.cos(math.radians(120)), 1.46 * math.sin(math.radians(120)), 0.0), (0, 0, 0), (1.16, 0, 0)]
    out['bent_nitrile'] = ([C, C, N_], bent, [(1, 0, 1), (2, 1, 3)], [], [2, 0, 0, 0, 1, 1, 0, 0])
    out['square_carbon'] = ([C] * 3, [(1.54, 0, 0), (0, 0, 0), (0, 1.54, 0)], chain_bonds(3), [], [2, 0, 0, 0, 1, 0, 0, 0])
    out['sharp_carbon'] = ([C] * 3, [(1.54, 0, 0), (0, 0, 0), (1.54 * math.cos(math.radians(80)), 1.54 * math.sin(math.radians(80)), 0)],
                           chain_bonds(3), [], [2, 0, 0, 0, 1, 1, 0, 0])
    out['compressed_bond'] = ([C, C], [(0, 0, 0), (0.6, 0, 0)], [(1, 0, 3)], [], [1, 0, 1, 0, 0, 0, 0, 0])
    out['stretched_bond'] = ([C, O], [(0, 0, 0), (0, 1.80, 0)], [(1, 0, 1)], [], [1, 0, 0, 1, 0, 0, 0, 0])
    # a chain of five folded back: an open pentagon, whose ends are four bonds and one bond length apart
    out['folded_chain'] = ([C] * 5, polygon(5, 1.54), chain_bonds(5), [], [4, 0, 0, 0, 3, 0, 1, 1])
    # the same distance between the ends of a chain of four: three bonds apart, no far pair
    out['folded_short_chain'] = ([C] * 4, polygon(4, 1.54), chain_bonds(4), [], [3, 0, 0, 0, 2, 0, 0, 0])
    ethane = [(0, 0, 0), (1.54, 0, 0)]
    out['two_pieces_apart'] = ([C] * 4, ethane + [(x, 6.0, 0.0) for x, _, _ in ethane], [(1, 0, 1), (3, 2, 1)], [],
                               [2, 0, 0, 0, 0, 0, 4, 0])
    out['two_pieces_overlapping'] = ([C] * 4, ethane + [(x, 1.0, 0.0) for x, _, _ in ethane], [(1, 0, 1), (3, 2, 1)], [],
                                     [2, 0, 0, 0, 0, 0, 4, 4])
    five = [(1.4, 0, 0), (-1.4, 0, 0), (0, 1.4, 0), (0, -1.4, 0), (0, 0, 1.4)]
    out['four_bonded_C'] = ([C] + [F] * 4, [(0, 0, 0)] + five[:4], [(k + 1, 0, 1) for k in range(4)], [], [4, 0, 0, 0, 6, 2, 0, 0])
    out['five_bonded_C'] = ([C] + [F] * 5, [(0, 0, 0)] + five, [(k + 1, 0, 1) for k in range(5)], [], [5, 0, 0, 0, 0, 0, 0, 0])
    return out


HAND = _hand()
CLEAN = ('butane', 'hexane', 'benzene', 'benzene_flagged_planar', 'propyne', 'sulfone', 'cyclopropane', 'cyclobutane')


def hand_molecule(name):
    """``dict(types, points, entries, planar, marked, dropped)`` of a hand-made molecule."""
    types, points, entries, planar, _ = HAND[name]
    return dict(types=list(types), points=[tuple(float(v) for v in p) for p in points], entries=list(entries),
                planar=list(planar), marked=[], dropped=[])


# ---- ties: coordinates exact in fp32, thresholds placed on the quantity itself ---------------------------------------------------
def up(v):
    return math.nextafter(v, math.inf)


def down(v):
    return math.nextafter(v, -math.inf)


def flat_bounds(nf, lo2, hi2):
    return [[[[lo2, hi2] for _ in range(3)] for _ in range(nf)] for _ in range(nf)]


def ties(nf=8):
    """name -> (molecule, (bounds2, cosines, clashes2), expected row 0 of counts).  Every coordinate is a small multiple of
    2^-2, so the differences, the products and their sums are exact in fp64 and d2 is the lattice number itself: a bound AT it
    does not fire (both comparisons are strict) and a bound one ulp past it does."""
    wide, nowhere = [[-2.0, 2.0]] * 3, [[0.0] * nf for _ in range(nf)]
    pair = dict(types=[C, O], points=[(0.25, 0.5, -1.0), (1.25, 1.0, -0.75)], entries=[(1, 0, 1)], planar=[], marked=[], dropped=[])
    d2 = 1.0 + 0.25 + 0.0625
    out = {}
    out['length_at_lo'] = (pair, (flat_bounds(nf, d2, 4.0), wide, nowhere), [1, 0, 0, 0, 0, 0, 0, 0])
    out['length_inside_lo'] = (pair, (flat_bounds(nf, up(d2), 4.0), wide, nowhere), [1, 0, 1, 0, 0, 0, 0, 0])
    out['length_at_hi'] = (pair, (flat_bounds(nf, 0.5, d2), wide, nowhere), [1, 0, 0, 0, 0, 0, 0, 0])
    out['length_inside_hi'] = (pair, (flat_bounds(nf, 0.5, down(d2)), wide, nowhere), [1, 0, 0, 1, 0, 0, 0, 0])
    apart = dict(pair, entries=[])
    everywhere = lambda v: [[v] * nf for _ in range(nf)]             # noqa: E731
    out['clash_at'] = (apart, (flat_bounds(nf, 0.5, 4.0), wide, everywhere(d2)), [0, 0, 0, 0, 0, 0, 1, 0])
    out['clash_inside'] = (apart, (flat_bounds(nf, 0.5, 4.0), wide, everywhere(up(d2))), [0, 0, 0, 0, 0, 0, 1, 1])
    # u = (1, 0, 0) and v = (0.75, 1, 0) / ... : a right angle has the cosine 0 exactly, and (3, 4, 0) . (1, 0, 0) / 5 = 0.6
    right = dict(types=[C, C, C], points=[(1.5, 0.25, 0.5), (0.5, 0.25, 0.5), (0.5, 1.5, 0.5)], entries=[(1, 0, 1), (2, 1, 1)],
                 planar=[], marked=[], dropped=[])
    loose = flat_bounds(nf, 0.25, 16.0)
    tetra = lambda lo, hi: [[-2.0, 2.0], [-2.0, 2.0], [lo, hi]]      # noqa: E731
    out['cosine_at_lo'] = (right, (loose, tetra(0.0, 2.0), nowhere), [2, 0, 0, 0, 1, 0, 0, 0])
    out['cosine_inside_lo'] = (right, (loose, tetra(up(0.0), 2.0), nowhere), [2, 0, 0, 0, 1, 1, 0, 0])
    out['cosine_at_hi'] = (right, (loose, tetra(-2.0, 0.0), nowhere), [2, 0, 0, 0, 1, 0, 0, 0])
    out['cosine_inside_hi'] = (right, (loose, tetra(-2.0, down(0.0)), nowhere), [2, 0, 0, 0, 1, 1, 0, 0])
    slanted = dict(right, points=[(1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.75, 1.0, 0.0)])      # (0.75 * 1) / sqrt(1 * 1.5625) = 0.6
    out['cosine_06_at_hi'] = (slanted, (loose, tetra(-2.0, 0.6), nowhere), [2, 0, 0, 0, 1, 0, 0, 0])
    out['cosine_06_inside_hi'] = (slanted, (loose, tetra(-2.0, down(0.6)), nowhere), [2, 0, 0, 0, 1, 1, 0, 0])
    # two atoms at one point: the cosine is 0 / 0, which no comparison flags; the bond is short
    same = dict(right, points=[(0.5, 0.25, 0.5), (0.5, 0.25, 0.5), (0.5, 1.5, 0.5)])
    out['zero_length'] = (same, (loose, tetra(-0.5, 0.5), nowhere), [2, 0, 1, 0, 1, 0, 0, 0])
    return out


# ---- random molecules and batches --------------------------------------------------------------------------------------------------
def random_molecule(rng, max_atoms=40, min_atoms=1, max_degree=5):
    """A random forest of ``min_atoms..max_atoms`` atoms with a few ring closures.  Every atom but the first of a piece lies 0.8
    to 2.2 A from its parent in a random direction, so that short, plausible and long bonds, good and bad angles and clashes
    all occur; orders, planar flags, marks and dropped atoms are drawn at random."""
    n = int(rng.integers(min_atoms, max_atoms + 1))
    types = [int(t) for t in rng.choice([C, C, C, N_, N_, O, S, F], n)]
    points, degree, entries, seen = [], [0] * n, [], set()

    def join(i, j):
        order = int(rng.choice([1, 1, 1, 1, 2, 2, 3]))
        entries.append((i, j, order) if rng.random() < 0.5 else (j, i, order))
        seen.add((min(i, j), max(i, j)))
        degree[i] += 1
        degree[j] += 1

    for i in range(n):
        open_ = [j for j in range(i) if degree[j] < max_degree]
        if open_ and rng.random() < 0.93:
            j = int(rng.choice(open_[-6:]))
            step = rng.normal(0, 1, 3)
            step *= rng.uniform(0.8, 2.2) / np.linalg.norm(step)
            points.append(tuple(float(v) for v in np.asarray(points[j]) + step))
            join(i, j)
        else:                                        # a new piece
            points.append(tuple(float(v) for v in rng.normal(0, 2.5, 3)))
    for _ in range(int(rng.integers(0, 4))):
        if n > 4:
            i, j = (int(v) for v in rng.choice(n, 2, replace=False))
            if (min(i, j), max(i, j)) not in seen and degree[i] < max_degree and degree[j] < max_degree:
                join(i, j)
    order = rng.permutation(len(entries))
    return dict(types=types, points=points, entries=[entries[k] for k in order],
                planar=[k for k in range(n) if rng.random() < 0.3], marked=[k for k in range(n) if rng.random() < 0.3],
                dropped=[k for k in range(n) if rng.random() < 0.2])


def chain(n, fold=7):
    """``n`` carbons on a zigzag that turns back every ``fold`` atoms, so that far pairs come close: a large molecule."""
    points = [(1.25 * (k % fold if (k // fold) % 2 == 0 else fold - 1 - k % fold), 0.75 * (k % 2) + 1.5 * (k // fold), 0.25 * (k % 3))
              for k in range(n)]
    return dict(types=[C if k % 5 else N_ for k in range(n)], points=points, entries=chain_bonds(n), planar=[],
                marked=list(range(n // 3, n // 2)), dropped=[])


def as_batch(molecules, N, capacity=None, nf=8, rng=None, scatter=True, extra_entries=None):
    """The entry point's arrays for a list of molecule dicts: every molecule on ``N`` rows - scattered among unreal rows that
    hold garbage (NaN included) when ``scatter`` - with its list in the first rows of ``capacity``.  ``planar`` is by atom
    number, ``marked`` and ``dropped`` become masks by row.  Returns a dict of numpy arrays."""
    rng = rng or np.random.default_rng(0)
    B = len(molecules)
    capacity = max([len(m['entries']) for m in molecules] + [1]) if capacity is None else capacity
    out = dict(x=np.zeros((B, N, 3), np.float32), one_hot=np.zeros((B, N, nf), np.float32), node_mask=np.zeros((B, N), np.float32),
               drop_mask=np.zeros((B, N), np.float32), mark_mask=np.zeros((B, N), np.float32),
               atom_planar=np.zeros((B, N), np.int32), bonds=np.full((B, capacity, 3), 77, np.int32),
               n_bonds_in=np.zeros(B, np.int32))
    if scatter:
        out['x'][:] = rng.normal(0, 3, (B, N, 3))
        out['x'][rng.random((B, N)) < 0.3] = np.nan
        out['one_hot'][:] = rng.random((B, N, nf))
        out['drop_mask'][:] = rng.random((B, N)) < 0.3
        out['mark_mask'][:] = rng.random((B, N)) < 0.3
    for b, m in enumerate(molecules):
        n = len(m['types'])
        rows = np.sort(rng.choice(N, n, replace=False)) if scatter else np.arange(n)
        out['node_mask'][b, rows] = 1
        out['x'][b, rows] = np.asarray(m['points'], dtype=np.float32).reshape(n, 3)
        out['one_hot'][b, rows] = 0
        out['one_hot'][b, rows, m['types']] = 1
        out['drop_mask'][b, rows] = 0
        out['drop_mask'][b, rows[m['dropped']]] = 1
        out['mark_mask'][b, rows] = 0
        out['mark_mask'][b, rows[m['marked']]] = 1
        out['atom_planar'][b, m['planar']] = 1
        entries = list(m['entries'])[:capacity]
        out['bonds'][b, :len(entries)] = np.asarray(entries, dtype=np.int32).reshape(len(entries), 3)
        out['n_bonds_in'][b] = len(m['entries'])
    return out
