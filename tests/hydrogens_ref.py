"""The hydrogen rule of ``dl_add_hydrogens`` (``include/difflinker_hip.h``, ``csrc/hydrogens.hip``) restated in plain Python
and numpy: the count from default valences, the geometry class, and the fp64 directions with every operation rounded on its
own in the header's order (Python floats are IEEE doubles and are never contracted).  The kernel must agree exactly in its
integers and is expected to agree bit for bit in the positions.

Atom ``k`` is the k-th row with ``node_mask != 0``; ``drop_mask`` removes atoms after that numbering; an entry
``(i, j, order)`` is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 3``, in either orientation.  It is this
project's own rule, not RDKit's ``AddHs(addCoords=True)`` and not OpenBabel's.

Below the rule: molecules whose answer is known by hand, degenerate molecules on exact coordinates, and a builder of random
molecules that rejects those in which a decision lies near its threshold."""
import math

import numpy as np

MAX_ATOMS = 256
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, OVERFLOW, NONFINITE = 1, 4, 8, 32, 64
EPS = 1e-6
SQRT3, SQRT2_3 = float.fromhex('0x1.bb67ae8584caap+0'), float.fromhex('0x1.a20bd700c2c3ep-1')
SQRT8_3, SQRT3_2 = float.fromhex('0x1.e2b7dddfefa67p-1'), float.fromhex('0x1.bb67ae8584caap-1')
T2, T3, T4 = 2, 3, 4                               # a class is its number of sites
FIELDS = ('n_h', 'h_count', 'h_parent', 'h_x', 'status')
FILL = 0x5a5a5a5a                                  # what an element the entry point does not write holds in the tests
FILL_F64 = float(np.frombuffer(b'\x5a' * 8, dtype=np.float64)[0])
ATOM2IDX = {'C': 0, 'O': 1, 'N': 2, 'F': 3, 'S': 4, 'Cl': 5, 'Br': 6, 'I': 7}
DEFAULT_VALENCE = {'C': 4, 'N': 3, 'O': 2, 'F': 1, 'S': 2, 'Cl': 1, 'Br': 1, 'I': 1, 'P': 3}
XH_LENGTH = {'C': 1.09, 'N': 1.01, 'O': 0.96, 'F': 0.92, 'S': 1.34, 'Cl': 1.27, 'Br': 1.41, 'I': 1.61, 'P': 1.42}


def tables(atom2idx=ATOM2IDX):
    """``(default_valence int32 [nf], xh_length float64 [nf])`` by the indices of ``atom2idx``."""
    valence, length = np.zeros(len(atom2idx), dtype=np.int32), np.zeros(len(atom2idx), dtype=np.float64)
    for name, k in atom2idx.items():
        valence[k], length[k] = DEFAULT_VALENCE[name], XH_LENGTH[name]
    return valence, length


# ---- the arithmetic: one rounding per operation ------------------------------------------------------------------------------
def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(s, a):
    return (s * a[0], s * a[1], s * a[2])


def fdiv(p, q):
    """IEEE division of two doubles: x / 0 is an infinity or NaN, as on the device, where Python raises."""
    with np.errstate(all='ignore'):
        return float(np.float64(p) / np.float64(q))


def over(a, s):
    return (fdiv(a[0], s), fdiv(a[1], s), fdiv(a[2], s))


def neg(a):
    return (-a[0], -a[1], -a[2])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def root(v):
    with np.errstate(all='ignore'):
        return float(np.sqrt(np.float64(v)))


def unit(a):
    return over(a, root(dot(a, a)))


def perp(u):
    m, least = 0, abs(u[0])
    if abs(u[1]) < least:
        m, least = 1, abs(u[1])
    if abs(u[2]) < least:
        m = 2
    e = (1.0 if m == 0 else 0.0, 1.0 if m == 1 else 0.0, 1.0 if m == 2 else 0.0)
    return unit(sub(e, scale(u[m], u)))


def directions(a, pos, adj, cls, d, decisions=None):
    """All directions of atom ``a``'s class in the header's order (the caller takes the first ``h``).  ``adj[a]`` is the
    sorted list of neighbours.  ``decisions`` collects ``(name, value, threshold)`` of every comparison with ``EPS`` made."""
    note = (lambda *t: None) if decisions is None else (lambda *t: decisions.append(t))
    xa = pos[a]
    if d == 0:
        g = fdiv(1.0, SQRT3)
        return [(g, g, g), (g, -g, -g), (-g, g, -g), (-g, -g, g)]
    nbr = adj[a][:3]
    u1 = unit(sub(pos[nbr[0]], xa))
    if d == 1:
        if cls == T2:
            return [neg(u1)]
        k = nbr[0]
        others = [t for t in adj[k] if t != a]
        e1 = None
        if others:
            w = sub(pos[others[0]], pos[k])
            p = sub(w, scale(dot(w, u1), u1))
            pp, ww = dot(p, p), dot(w, w)
            note('p.p / w.w', fdiv(pp, ww), EPS)
            if pp > EPS * ww:
                e1 = neg(over(p, root(pp)))
        if e1 is None:
            e1 = perp(u1)
            if not others and a > k:
                e1 = neg(e1)
        if cls == T3:
            back, side = neg(over(u1, 2.0)), scale(SQRT3_2, e1)
            return [add(back, side), sub(back, side)]
        e2, back = cross(u1, e1), neg(over(u1, 3.0))
        return [add(back, scale(SQRT8_3, add(scale(c, e1), scale(s, e2))))
                for c, s in ((1.0, 0.0), (-0.5, SQRT3_2), (-0.5, -SQRT3_2))]
    u2 = unit(sub(pos[nbr[1]], xa))
    if d == 2:
        s, c = add(u1, u2), cross(u1, u2)
        ss = dot(s, s)
        note('s.s', ss, EPS)
        if ss <= EPS:
            b = perp(u1)
            n = cross(u1, b)
        else:
            b = neg(over(s, root(ss)))
            cc = dot(c, c)
            note('c.c', cc, EPS)
            n = over(c, root(cc)) if cc > EPS else perp(u1)
        if cls == T3:
            return [b]
        mid, side = over(b, SQRT3), scale(SQRT2_3, n)
        return [add(mid, side), sub(mid, side)]
    u3 = unit(sub(pos[nbr[2]], xa))
    s = add(add(u1, u2), u3)
    ss = dot(s, s)
    note('s.s', ss, EPS)
    if ss > EPS:
        return [neg(over(s, root(ss)))]
    w = cross(sub(u2, u1), sub(u3, u1))
    ww = dot(w, w)
    note('w.w', ww, EPS)
    return [over(w, root(ww)) if ww > EPS else perp(u1)]


def molecule(x, types, mask, entries, n_bonds_in, default_valence, xh_length, status_in=0, drop=None, planar=None,
             decisions=None):
    """One molecule: ``x [N,3]`` float32, ``types [N]`` and ``mask [N]`` by row, ``entries`` the ``capacity`` rows of its list,
    ``drop [N]`` by row, ``planar [N]`` by atom number.  Returns ``(n_h, h_count by atom number, parents, positions, status,
    cases)``: every hydrogen, and the set of ``(class, d)`` of the atoms that got some."""
    capacity = len(entries)
    real = [r for r in range(len(mask)) if mask[r] != 0]
    n = len(real)
    kept = [not (drop is not None and drop[r] != 0) for r in real]
    status = int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0)
    if sum(kept) > MAX_ATOMS:
        return 0, [0] * n, [], [], status | TOO_LARGE, set()
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
        return 0, [0] * n, [], [], status | NONFINITE, set()
    adj = {k: [] for k in pos}
    for (i, j) in pairs:
        adj[i].append(j)
        adj[j].append(i)
    for a in adj:
        adj[a].sort()
    h_count, parents, points, cases = [0] * n, [], [], set()
    for a in sorted(pos):
        d = len(adj[a])
        orders = [pairs[(min(a, t), max(a, t))] for t in adj[a]]
        t = int(types[real[a]])
        h0 = max(0, int(default_valence[t]) - sum(orders))
        n2, n3 = orders.count(2), orders.count(3)
        if n3 > 0 or n2 >= 2:
            cls = T2
        elif n2 == 1 or (planar is not None and planar[a] != 0 and d == 2 and h0 == 1):
            cls = T3
        else:
            cls = T4
        h = min(h0, max(0, cls - d))
        h_count[a] = h
        if h == 0:
            continue
        cases.add((cls, d))
        length = float(xh_length[t])
        for q in directions(a, pos, adj, cls, d, decisions)[:h]:
            parents.append(a)
            points.append(add(pos[a], scale(length, q)))
    return len(parents), h_count, parents, points, status, cases


def first_largest(one_hot):
    """Index of the FIRST largest entry of every row (``numpy.argmax`` returns the first of equal maxima)."""
    return np.argmax(np.asarray(one_hot), axis=-1)


def add_hydrogens(x, one_hot, node_mask, bonds, n_bonds_in, default_valence, xh_length, Hcap, status_in=None, drop_mask=None,
                  atom_planar=None):
    """The whole batch, with the entry point's shapes and dtypes: ``x [B,N,3]`` float32, ``one_hot [B,N,nf]``, ``node_mask
    [B,N]``, ``bonds [B,capacity,3]``.  ``h_parent`` and ``h_x`` hold ``FILL`` bytes from ``min(n_h, Hcap)`` on, which the
    entry point leaves untouched.  ``cases`` (not an output of the entry point) is the union of the molecules' cases."""
    x, node_mask, bonds = np.asarray(x, dtype=np.float32), np.asarray(node_mask), np.asarray(bonds)
    B, N = node_mask.shape
    types = first_largest(one_hot)
    out = {'n_h': np.zeros(B, np.int32), 'h_count': np.zeros((B, N), np.int32), 'h_parent': np.full((B, Hcap), FILL, np.int32),
           'h_x': np.full((B, Hcap, 3), FILL_F64, np.float64), 'status': np.zeros(B, np.int32), 'cases': set()}
    for b in range(B):
        n_h, h_count, parents, points, status, cases = molecule(
            x[b], types[b], node_mask[b], bonds[b], int(n_bonds_in[b]), default_valence, xh_length,
            0 if status_in is None else int(status_in[b]), None if drop_mask is None else drop_mask[b],
            None if atom_planar is None else atom_planar[b])
        out['n_h'][b] = n_h
        out['h_count'][b, :len(h_count)] = h_count
        listed = min(n_h, Hcap)
        out['h_parent'][b, :listed] = parents[:listed]
        if listed:
            out['h_x'][b, :listed] = np.asarray(points[:listed], dtype=np.float64)
        out['status'][b] = status | (OVERFLOW if n_h > Hcap else 0)
        out['cases'] |= cases
    return out


# ---- measuring a result ----------------------------------------------------------------------------------------------------
def angle(p, centre, q):
    """The angle p - centre - q in degrees."""
    a, b = np.asarray(p, float) - centre, np.asarray(q, float) - centre
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / math.sqrt(float(a @ a) * float(b @ b))))))


def torsion(p0, p1, p2, p3):
    """The dihedral angle p0 - p1 - p2 - p3 in degrees, in (-180, 180]."""
    p0, p1, p2, p3 = (np.asarray(p, float) for p in (p0, p1, p2, p3))
    b0, b1, b2 = p0 - p1, p2 - p1, p3 - p2
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return math.degrees(math.atan2(float(np.cross(b1, v) @ w), float(v @ w)))


# ---- molecules whose answer is known by hand ---------------------------------------------------------------------------------
C, O, N_, F, S = ATOM2IDX['C'], ATOM2IDX['O'], ATOM2IDX['N'], ATOM2IDX['F'], ATOM2IDX['S']
TET = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]


def _bent(length, degrees=109.4712206):
    """Two neighbours of an atom at the origin, ``length`` away and ``degrees`` apart, in the xy plane."""
    half = math.radians(degrees) / 2
    return [(length * math.sin(half), length * math.cos(half), 0.0), (-length * math.sin(half), length * math.cos(half), 0.0)]


def polygon(n, edge):
    r = edge / (2 * math.sin(math.pi / n))
    return [(r * math.cos(2 * math.pi * k / n), r * math.sin(2 * math.pi * k / n), 0.0) for k in range(n)]


def _hand():
    """name -> (types, points, entries, expected h_count, planar atoms or None)."""
    out = {}
    for name, t, h in (('lone_C', C, 4), ('lone_N', N_, 3), ('lone_O', O, 2), ('lone_F', F, 1)):
        out[name] = ([t], [(0.5, -1.0, 2.0)], [], [h], None)
    out['ethane'] = ([C, C], [(0, 0, 0), (1.54, 0, 0)], [(1, 0, 1)], [3, 3], None)
    out['methanol'] = ([C, O], [(0, 0, 0), (0.3, 1.4, 0.1)], [(1, 0, 1)], [3, 1], None)
    out['methylamine'] = ([N_, C], [(0, 0, 0), (-0.2, 0.3, 1.42)], [(0, 1, 1)], [2, 3], None)
    a, b = _bent(1.53)
    out['propane'] = ([C, C, C], [a, (0, 0, 0), b], [(1, 0, 1), (2, 1, 1)], [3, 2, 3], None)
    a, b = _bent(1.46, 112.0)
    out['dimethylamine'] = ([C, N_, C], [a, (0, 0, 0), b], [(1, 0, 1), (2, 1, 1)], [3, 1, 3], None)
    arm = 1.53 / math.sqrt(3)
    out['isobutane'] = ([C, C, C, C], [(0, 0, 0)] + [tuple(arm * v for v in TET[k]) for k in range(3)],
                        [(1, 0, 1), (2, 0, 1), (3, 0, 1)], [1, 3, 3, 3], None)
    out['ethene'] = ([C, C], [(0, 0, 0), (0, 1.34, 0)], [(1, 0, 2)], [2, 2], None)
    a, b = _bent(1.0, 120.0)
    out['propene'] = ([C, C, C], [tuple(1.34 * v for v in a), (0, 0, 0), tuple(1.50 * v for v in b)], [(1, 0, 2), (2, 1, 1)],
                      [2, 1, 3], None)
    out['benzene'] = ([C] * 6, polygon(6, 1.39), [((k + 1) % 6, k, 2 - k % 2) for k in range(6)], [1] * 6, None)
    ring = [((k + 1) % 5, k, o) for k, o in enumerate((1, 2, 1, 2, 1))]
    out['pyrrole'] = ([N_, C, C, C, C], polygon(5, 1.38), ring, [1] * 5, [0])
    out['pyrrole_unflagged'] = ([N_, C, C, C, C], polygon(5, 1.38), ring, [1] * 5, None)
    out['propyne'] = ([C, C, C], [(0, 0, 0), (1.25, 0, 0), (2.75, 0, 0)], [(1, 0, 3), (2, 1, 1)], [1, 0, 3], None)
    out['acetonitrile'] = ([C, C, N_], [(0, 0, 0), (0, 0, 1.46), (0, 0, 2.62)], [(1, 0, 1), (2, 1, 3)], [3, 0, 0], None)
    out['formaldehyde'] = ([C, O], [(0, 0, 0), (1.2, 0.1, 0)], [(1, 0, 2)], [2, 0], None)
    arm = 1.6 / math.sqrt(3)
    out['sulfone'] = ([S, C, C, O, O], [(0, 0, 0)] + [tuple(arm * v for v in t) for t in TET],
                      [(1, 0, 1), (2, 0, 1), (3, 0, 2), (4, 0, 2)], [0, 3, 3, 0, 0], None)
    five = [(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5)]
    out['five_bonded_C'] = ([C] + [F] * 5, [(0, 0, 0)] + five, [(k + 1, 0, 1) for k in range(5)], [0] * 6, None)
    return out


def _degenerate():
    """Coordinates that are small multiples of a power of two (or, for ``trigonal_planar``, sum to zero within rounding): the
    quantity a branch is decided on is exact, or orders of magnitude from ``EPS``."""
    out = {}
    out['antiparallel'] = ([C, C, C], [(1, 0, 0), (0, 0, 0), (-1, 0, 0)], [(1, 0, 1), (2, 1, 1)], [3, 2, 3], None)
    out['t_shaped'] = ([C, C, C, C], [(0, 0, 0), (1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0)], [(1, 0, 1), (2, 0, 1), (3, 0, 1)],
                       [1, 3, 3, 3], None)
    third = [(1.5 * math.cos(2 * math.pi * k / 3), 1.5 * math.sin(2 * math.pi * k / 3), 0.0) for k in range(3)]
    out['trigonal_planar'] = ([C, C, C, C], [(0, 0, 0)] + third, [(1, 0, 1), (2, 0, 1), (3, 0, 1)], [1, 3, 3, 3], None)
    out['collinear_r'] = HAND['propyne']
    out['no_r'] = ([C, N_], [(0.25, 0.5, -1), (0.25, 2, -1)], [(0, 1, 1)], [3, 2], None)
    out['diagonal'] = ([C, C], [(0, 0, 0), (1, 1, 1)], [(1, 0, 1)], [3, 3], None)
    out['diagonal_pair'] = ([O, C, C], [(1, 1, 1), (0, 0, 0), (-1, -1, -1)], [(1, 0, 1), (2, 1, 1)], [1, 2, 3], None)
    return out


HAND = _hand()
DEGENERATE = _degenerate()


def hand_molecule(name):
    """``dict(types, points, entries, planar)`` of a hand-made or degenerate molecule."""
    types, points, entries, _, planar = (HAND.get(name) or DEGENERATE[name])
    return dict(types=list(types), points=[tuple(float(v) for v in p) for p in points], entries=list(entries),
                planar=list(planar or []))


def chain(n):
    """``n`` carbons in a zigzag with single bonds, every one numbered after its neighbour."""
    points = [(1.25 * k, 0.75 * (k % 2), 0.0) for k in range(n)]
    return dict(types=[C] * n, points=points, entries=[(k + 1, k, 1) for k in range(n - 1)], planar=[])


def random_molecule(rng, max_atoms=40):
    """A random tree of 1..``max_atoms`` atoms with a few ring closures, orders drawn so that every class occurs, random 3D
    coordinates, random planar flags and, for ``dropped``, a random subset of its atoms."""
    n = int(rng.integers(1, max_atoms + 1))
    types = [int(t) for t in rng.choice([C, C, C, N_, N_, O, S, F], n)]
    points = [tuple(float(v) for v in rng.normal(0, 2.5, 3)) for _ in range(n)]
    degree, entries, seen = [0] * n, [], set()

    def join(i, j):
        order = int(rng.choice([1, 1, 1, 1, 2, 2, 3]))
        entries.append((i, j, order) if rng.random() < 0.5 else (j, i, order))
        seen.add((min(i, j), max(i, j)))
        degree[i] += 1
        degree[j] += 1

    for i in range(1, n):
        open_ = [j for j in range(i) if degree[j] < 3]
        if open_ and rng.random() < 0.95:            # else: a new piece
            join(i, int(rng.choice(open_[-6:])))
    for _ in range(int(rng.integers(0, 3))):
        if n > 4:
            i, j = (int(v) for v in rng.choice(n, 2, replace=False))
            if (min(i, j), max(i, j)) not in seen and degree[i] < 3 and degree[j] < 3:
                join(i, j)
    order = rng.permutation(len(entries))
    return dict(types=types, points=points, entries=[entries[k] for k in order],
                planar=[k for k in range(n) if rng.random() < 0.3], dropped=[k for k in range(n) if rng.random() < 0.2])


def near_threshold(decisions, factor=10.0):
    """Is a decision quantity within ``factor`` of its threshold (or not a number)?  Such a molecule is not drawn: no case of
    the random test may hinge on one ulp."""
    return any(not (value < threshold / factor or value > threshold * factor) for _, value, threshold in decisions)


def random_molecules(rng, count, max_atoms=40, with_drop=lambda b: b % 2 == 1):
    """``count`` random molecules none of which decides anything near ``EPS``, and how many draws that took.  ``dropped`` is
    emptied unless ``with_drop(b)``."""
    valence, length = tables()
    molecules, draws = [], 0
    while len(molecules) < count:
        m = random_molecule(rng, max_atoms)
        draws += 1
        if not with_drop(len(molecules)):
            m['dropped'] = []
        n = len(m['types'])
        drop = np.zeros(n)
        drop[m['dropped']] = 1
        planar = np.zeros(n)
        planar[m['planar']] = 1
        decisions = []
        molecule(np.asarray(m['points'], dtype=np.float32), m['types'], np.ones(n), m['entries'], len(m['entries']), valence,
                 length, drop=drop, planar=planar, decisions=decisions)
        if not near_threshold(decisions):
            molecules.append(m)
    return molecules, draws
