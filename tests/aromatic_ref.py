"""The aromatic-ring rule of ``dl_aromatic_rings`` (``include/difflinker_hip.h``, ``csrc/aromatic.hip``) restated in plain
Python and numpy: eligible atoms, chordless 5- and 6-cycles, the fp64 planarity test with every operation rounded on its own
(Python floats are IEEE doubles and are never contracted), systems, roles, the Kekule assignment by its definition, the new
orders and the aromatic rings.  The kernel must agree exactly.

Atom ``k`` is the k-th row with ``node_mask != 0``; ``drop_mask`` removes atoms after that numbering; an entry
``(i, j, order)`` is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 3``, in either orientation.  It is this
project's own rule, not RDKit's aromaticity and not OpenBabel's bond typing.

Below the rule: molecules whose answer is known by hand (regular polygons with 1.39 A edges) and a builder of random fused
ring systems."""
import math
from functools import lru_cache

import numpy as np

MAX_ATOMS, MAX_RINGS, MAX_SYSTEM = 256, 64, 32
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, MANY_RINGS, BIG_SYSTEM = 1, 4, 8, 16, 32
TOL2_RING, TOL2_SUB = 0.1 ** 2, 0.5 ** 2
FIELDS = ('order_out', 'bond_aromatic', 'atom_aromatic', 'valence_out', 'n_planar_rings', 'n_aromatic_rings',
          'n_aromatic_marked', 'status')
PER_MOLECULE = ('atom_aromatic', 'valence_out', 'n_planar_rings', 'n_aromatic_rings', 'n_aromatic_marked', 'status')
ROLE_D, ROLE_X, ROLE_P, ROLE_F = 'D', 'X', 'P', 'F'


def ring_class_table(atom2idx):
    """int32 ``[nf]``: 1 for C, 2 for N, 3 for O and S, 0 for anything else, by the indices of ``atom2idx``."""
    cls = {'C': 1, 'N': 2, 'O': 3, 'S': 3}
    table = np.zeros(len(atom2idx), dtype=np.int32)
    for name, k in atom2idx.items():
        table[k] = cls.get(name, 0)
    return table


def candidate_rings(adj, eligible):
    """Chordless simple cycles of 5 or 6 eligible atoms, each once in canonical order: from its smallest atom, in the
    direction whose second atom is smaller than its last."""
    found = []

    def walk(path):
        last = path[-1]
        if len(path) in (5, 6) and path[0] in adj[last] and path[1] < last:
            n = len(path)
            chord = any(path[l] in adj[path[k]] for k in range(n) for l in range(k + 2, n) if not (k == 0 and l == n - 1))
            if not chord:
                found.append(tuple(path))
        if len(path) == 6:
            return
        for t in sorted(adj[last]):
            if t > path[0] and eligible[t] and t not in path:
                walk(path + [t])

    for s in sorted(adj):
        if eligible[s]:
            walk([s])
    return found


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def ring_plane(points):
    """``(c, q, m, mm)`` of the rule for the fp64 points of a cycle in canonical order."""
    n = len(points)
    c = []
    for d in range(3):
        s = points[0][d]
        for k in range(1, n):
            s = s + points[k][d]
        c.append(s / n)
    q = [tuple(p[d] - c[d] for d in range(3)) for p in points]
    m = cross(q[0], q[1])
    for k in range(1, n):
        t = cross(q[k], q[(k + 1) % n])
        m = (m[0] + t[0], m[1] + t[1], m[2] + t[2])
    return c, q, m, (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]


def is_planar(cycle, adj, pos, tol2_ring=TOL2_RING, tol2_sub=TOL2_SUB):
    c, q, m, mm = ring_plane([pos[k] for k in cycle])
    if not mm > 0:
        return False
    limit_ring, limit_sub = tol2_ring * mm, tol2_sub * mm
    for v in q:
        d = dot(v, m)
        if not d * d <= limit_ring:
            return False
    for k in cycle:
        for s in adj[k]:
            if s in cycle:
                continue
            d = dot(tuple(pos[s][t] - c[t] for t in range(3)), m)
            if not d * d <= limit_sub:
                return False
    return True


def kekule(atoms, ring_adj, role):
    """The assignment M of one system by its definition: among the sets of ring bonds with both ends ``P`` or ``F`` and no
    atom twice, the most ``P`` covered, then the most ``F``, then the smallest sorted list of ``(min, max)`` pairs.  Take the
    smallest atom left: it stays uncovered, or it is paired with a neighbour that is left; a pair with the smallest atom
    sorts before every pair without it, so comparing ``(-P, -F, list)`` of the alternatives is comparing by the definition."""
    atoms = tuple(sorted(atoms))
    free = {a for a in atoms if role[a] in (ROLE_P, ROLE_F)}

    @lru_cache(maxsize=None)
    def best(left):
        if not left:
            return (0, 0, ())
        u, rest = left[0], left[1:]
        options = [best(rest)]
        if u in free:
            for v in sorted(ring_adj[u]):
                if v in rest and v in free:
                    p, f, pairs = best(tuple(a for a in rest if a != v))
                    gain_p = (role[u] == ROLE_P) + (role[v] == ROLE_P)
                    options.append((p - gain_p, f - (2 - gain_p), ((u, v),) + pairs))
        return min(options)

    return list(best(atoms)[2])


def kekule_brute(atoms, ring_adj, role):
    """The same by listing every admissible set of bonds (small systems only)."""
    edges = sorted({(min(u, v), max(u, v)) for u in atoms for v in ring_adj[u]
                    if role[u] in (ROLE_P, ROLE_F) and role[v] in (ROLE_P, ROLE_F)})
    best = None
    for bits in range(1 << len(edges)):
        chosen = [e for k, e in enumerate(edges) if bits >> k & 1]
        ends = [a for e in chosen for a in e]
        if len(set(ends)) != len(ends):
            continue
        key = (-sum(role[a] == ROLE_P for a in ends), -sum(role[a] == ROLE_F for a in ends), chosen)
        best = key if best is None or key < best else best
    return best[2]


def molecule(x, types, mask, entries, n_bonds_in, ring_class, status_in=0, drop=None, mark=None, tol2_ring=TOL2_RING,
             tol2_sub=TOL2_SUB, detail=None):
    """One molecule: ``x [N][3]`` (fp32 values), ``types [N]`` (index of the first largest one-hot entry), ``mask`` / ``drop`` /
    ``mark`` rows of ``N`` numbers, ``entries`` the whole list ``[capacity][3]``.  Returns a dict of ``FIELDS``.  ``detail``, a
    dict, receives the rings, roles and the assignment for the tests that look at them."""
    N, capacity = len(mask), len(entries)
    rows = [r for r in range(N) if mask[r] != 0]
    n = len(rows)
    kept = [drop is None or drop[r] == 0 for r in rows]
    marked = [mark is not None and mark[r] != 0 for r in rows]
    out = {'order_out': [0] * capacity, 'bond_aromatic': [0] * capacity, 'atom_aromatic': [0] * N, 'valence_out': [0] * N,
           'n_planar_rings': 0, 'n_aromatic_rings': 0, 'n_aromatic_marked': 0,
           'status': int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0)}
    nb = min(max(int(n_bonds_in), 0), capacity)
    valid = {}
    for e in range(nb):
        i, j, order = (int(v) for v in entries[e])
        if 0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 3:
            valid[e] = (i, j, order)
            out['order_out'][e] = order
        else:
            out['status'] |= BAD_BOND
    if sum(kept) > MAX_ATOMS:                    # orders pass through; the list is not searched for repeated pairs
        out['status'] |= TOO_LARGE
        return out
    adj = {k: set() for k in range(n) if kept[k]}
    first = {}                                   # pair -> input order of its first entry
    for e, (i, j, order) in valid.items():
        if not (kept[i] and kept[j]):
            continue
        pair = (min(i, j), max(i, j))
        if pair in first:
            out['status'] |= BAD_BOND
            continue
        first[pair] = order
        adj[i].add(j)
        adj[j].add(i)
    cls = {k: (int(ring_class[types[rows[k]]]) if 0 <= types[rows[k]] < len(ring_class) else 0) for k in adj}
    eligible = {k: (cls[k] in (1, 2) and len(adj[k]) in (2, 3)) or (cls[k] == 3 and len(adj[k]) == 2) for k in adj}
    pos = {k: tuple(float(np.float32(v)) for v in x[rows[k]]) for k in adj}
    planar = [c for c in candidate_rings(adj, eligible) if is_planar(c, adj, pos, tol2_ring, tol2_sub)]

    def valences(order_of):
        for (i, j) in first:
            out['valence_out'][i] += order_of[(i, j)]
            out['valence_out'][j] += order_of[(i, j)]

    if len(planar) > MAX_RINGS:
        out['status'] |= MANY_RINGS
        valences(first)
        return out
    out['n_planar_rings'] = len(planar)
    ring_bonds = {(min(c[k], c[(k + 1) % len(c)]), max(c[k], c[(k + 1) % len(c)])) for c in planar for k in range(len(c))}
    ring_adj = {}
    for u, v in ring_bonds:
        ring_adj.setdefault(u, set()).add(v)
        ring_adj.setdefault(v, set()).add(u)
    label = {a: a for a in ring_adj}             # systems: the smallest atom of the piece
    changed = True
    while changed:
        changed = False
        for u, v in ring_bonds:
            low = min(label[u], label[v])
            changed = changed or label[u] != low or label[v] != low
            label[u] = label[v] = low
    role = {}
    for a in ring_adj:
        if cls[a] == 3 or (cls[a] == 2 and len(adj[a]) == 3):
            role[a] = ROLE_D
        elif any(first[(min(a, s), max(a, s))] >= 2 and s not in ring_adj[a] for s in adj[a]):
            role[a] = ROLE_X
        else:
            role[a] = ROLE_P if cls[a] == 1 else ROLE_F
    new = dict(first)
    covered, big = set(), set()
    for root in sorted(set(label.values())):
        atoms = [a for a in ring_adj if label[a] == root]
        if len(atoms) > MAX_SYSTEM:
            out['status'] |= BIG_SYSTEM
            big.add(root)
            continue
        chosen = kekule(atoms, ring_adj, role)
        for u in atoms:
            for v in ring_adj[u]:
                if u < v:
                    new[(u, v)] = 2 if (u, v) in chosen else 1
        covered.update(a for pair in chosen for a in pair)
    valences(new)
    aromatic_bonds = set()
    for c in planar:
        if label[c[0]] in big:
            continue
        if any(role[a] == ROLE_P and a not in covered for a in c):
            continue
        total = sum(2 if role[a] == ROLE_D else 0 if role[a] == ROLE_X else 1 if a in covered else
                    (0 if role[a] == ROLE_P else 2) for a in c)
        if total != 6:
            continue
        out['n_aromatic_rings'] += 1
        out['n_aromatic_marked'] += all(marked[a] for a in c)
        for k, a in enumerate(c):
            out['atom_aromatic'][a] = 1
            b = c[(k + 1) % len(c)]
            aromatic_bonds.add((min(a, b), max(a, b)))
    for e, (i, j, order) in valid.items():
        pair = (min(i, j), max(i, j))
        if kept[i] and kept[j] and pair in ring_bonds and label[pair[0]] not in big:
            out['order_out'][e] = new[pair]
            out['bond_aromatic'][e] = int(pair in aromatic_bonds)
    if detail is not None:
        detail.update(planar=planar, role=role, new=new, covered=covered, label=label, ring_bonds=ring_bonds)
    return out


def first_largest(one_hot):
    """Index of the first largest entry of every row of ``one_hot [..., nf]``."""
    return np.argmax(np.asarray(one_hot), axis=-1)


def aromatic_rings(x, one_hot, node_mask, bonds, n_bonds_in, ring_class, status_in=None, drop_mask=None, mark_mask=None,
                   tol2_ring=TOL2_RING, tol2_sub=TOL2_SUB):
    """A batch: ``x [B,N,3]``, ``one_hot [B,N,nf]``, ``node_mask [B,N]``, ``bonds [B,capacity,3]``, ``n_bonds_in [B]``
    (array-likes).  Returns a dict of int32 numpy arrays shaped as the kernel's outputs."""
    node_mask = np.asarray(node_mask).reshape(len(node_mask), -1)
    B, N = node_mask.shape
    x = np.asarray(x, dtype=np.float32).reshape(B, N, 3)
    types = first_largest(np.asarray(one_hot).reshape(B, N, -1))
    bonds = np.asarray(bonds, dtype=np.int64)
    bonds = bonds.reshape(B, bonds.size // (3 * B) if B else 0, 3)
    row = lambda m, b: None if m is None else np.asarray(m).reshape(B, N)[b].tolist()      # noqa: E731
    each = [molecule(x[b], types[b].tolist(), node_mask[b].tolist(), bonds[b].tolist(), int(n_bonds_in[b]), ring_class,
                     0 if status_in is None else int(status_in[b]), row(drop_mask, b), row(mark_mask, b), tol2_ring, tol2_sub)
            for b in range(B)]
    shape = {'order_out': (B, bonds.shape[1]), 'bond_aromatic': (B, bonds.shape[1]), 'atom_aromatic': (B, N),
             'valence_out': (B, N)}
    return {name: np.array([m[name] for m in each], dtype=np.int32).reshape(shape.get(name, (B,))) for name in FIELDS}


# ---- geometry builders -------------------------------------------------------------------------------------------------
EDGE = 1.39
C, O, N_, S = 0, 1, 2, 4                          # const.ATOM2IDX


def polygon(n, edge=EDGE):
    """A regular n-gon in the plane z = 0, centred on the origin, atom 0 on the x axis, counter-clockwise."""
    r = edge / (2 * math.sin(math.pi / n))
    return [(r * math.cos(2 * math.pi * k / n), r * math.sin(2 * math.pi * k / n), 0.0) for k in range(n)]


def fuse(a, b, centre, n, edge=None):
    """The ``n - 2`` new points of a regular n-gon on the edge ``a -> b``, on the side away from ``centre`` (z is a's)."""
    ax, ay, bx, by = a[0], a[1], b[0], b[1]
    edge = math.hypot(bx - ax, by - ay) if edge is None else edge
    side = (bx - ax) * (centre[1] - ay) - (by - ay) * (centre[0] - ax)      # > 0: the centre is left of a -> b
    turn = (-1 if side > 0 else 1) * 2 * math.pi / n
    heading = math.atan2(by - ay, bx - ax)
    px, py, out = bx, by, []
    for _ in range(n - 2):
        heading += turn
        px, py = px + edge * math.cos(heading), py + edge * math.sin(heading)
        out.append((px, py, a[2]))
    return out


def outward(p, centre, length):
    """A point ``length`` beyond ``p`` on the ray from ``centre``, in the plane z = p's."""
    dx, dy = p[0] - centre[0], p[1] - centre[1]
    d = math.hypot(dx, dy)
    return (p[0] + length * dx / d, p[1] + length * dy / d, p[2])


def centroid(points):
    return tuple(sum(p[d] for p in points) / len(points) for d in range(3))


def cycle_bonds(atoms, order=1):
    return [(atoms[k], atoms[(k + 1) % len(atoms)], order) for k in range(len(atoms))]


def _hand():
    """name: (types, points, bonds (i, j, order), expected) with expected = dict(planar, aromatic, doubles) where doubles is
    the sorted list of pairs of new order 2 among ALL bonds."""
    hand = {}
    hexagon, pentagon = polygon(6), polygon(5)
    origin = (0.0, 0.0, 0.0)
    hand['benzene'] = ([C] * 6, hexagon, cycle_bonds(range(6)), dict(planar=1, aromatic=1, doubles=[(0, 1), (2, 3), (4, 5)]))
    hand['benzene_all_double'] = ([C] * 6, hexagon, cycle_bonds(range(6), 2),
                                  dict(planar=1, aromatic=1, doubles=[(0, 1), (2, 3), (4, 5)]))
    chair = [(p[0], p[1], 0.25 if k % 2 else -0.25) for k, p in enumerate(hexagon)]
    hand['cyclohexane_chair'] = ([C] * 6, chair, cycle_bonds(range(6)), dict(planar=0, aromatic=0, doubles=[]))
    # two neighbours pushed 0.132 A up and down: the plane of the rule tilts after them and leaves them 0.11 A off it
    bent = [(p[0], p[1], (0.132, -0.132)[k] if k < 2 else 0.0) for k, p in enumerate(hexagon)]
    hand['ring_off_plane'] = ([C] * 6, bent, cycle_bonds(range(6)), dict(planar=0, aromatic=0, doubles=[]))
    hand['cyclopentadiene'] = ([C] * 5, pentagon, cycle_bonds(range(5)), dict(planar=1, aromatic=0, doubles=[(0, 1), (2, 3)]))
    hand['pyrrole'] = ([N_, C, C, C, C], pentagon, cycle_bonds(range(5)), dict(planar=1, aromatic=1, doubles=[(1, 2), (3, 4)]))
    hand['furan'] = ([O, C, C, C, C], pentagon, cycle_bonds(range(5)), dict(planar=1, aromatic=1, doubles=[(1, 2), (3, 4)]))
    hand['imidazole_n0'] = ([N_, C, N_, C, C], pentagon, cycle_bonds(range(5)),
                            dict(planar=1, aromatic=1, doubles=[(0, 1), (3, 4)]))
    hand['imidazole_c0'] = ([C, N_, C, N_, C], pentagon, cycle_bonds(range(5)),
                            dict(planar=1, aromatic=1, doubles=[(0, 4), (1, 2)]))
    hand['pyridine'] = ([N_] + [C] * 5, hexagon, cycle_bonds(range(6)), dict(planar=1, aromatic=1, doubles=[(0, 1), (2, 3), (4, 5)]))
    # 2-pyridone: N0 with a methyl (6), C1 with the carbonyl oxygen (7)
    hand['pyridone'] = ([N_] + [C] * 6 + [O], hexagon + [outward(hexagon[0], origin, 1.47), outward(hexagon[1], origin, 1.23)],
                        cycle_bonds(range(6)) + [(0, 6, 1), (1, 7, 2)],
                        dict(planar=1, aromatic=1, doubles=[(1, 7), (2, 3), (4, 5)]))
    hand['dioxin'] = ([O, C, C, O, C, C], hexagon, cycle_bonds(range(6)), dict(planar=1, aromatic=0, doubles=[(1, 2), (4, 5)]))
    second = fuse(hexagon[0], hexagon[1], origin, 6)                      # atoms 6..9, ring 0 1 9 8 7 6 ... in walk order
    naphthalene = cycle_bonds(range(6)) + [(1, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 0, 1)]
    hand['naphthalene'] = ([C] * 10, hexagon + second, naphthalene,
                           dict(planar=2, aromatic=2, doubles=[(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)]))
    far = outward(hexagon[0], origin, 1.48)
    shift = (far[0] + EDGE, 0.0, 0.0)                                     # the second ring's centre: its atom 3 is `far`
    other = [(p[0] + shift[0], p[1], 0.0) for p in hexagon]              # atom 6 + 3 sits at `far`
    hand['biphenyl'] = ([C] * 12, hexagon + other, cycle_bonds(range(6)) + cycle_bonds(range(6, 12)) + [(0, 9, 1)],
                        dict(planar=2, aromatic=2, doubles=[(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)]))
    up = outward(pentagon[0], origin, 0.8)
    hand['spiro_substituents'] = ([C] * 7, pentagon + [(up[0], up[1], 1.26), (up[0], up[1], -1.26)],
                                  cycle_bonds(range(5)) + [(0, 5, 1), (0, 6, 1)], dict(planar=0, aromatic=0, doubles=[]))
    return hand


HAND = _hand()


def as_batch(molecules, N=None, capacity=None, nf=8):
    """``(x, one_hot, node_mask, bonds, n_bonds)`` numpy arrays of a ragged batch of ``(types, points, bonds)`` triples."""
    B = len(molecules)
    N = max(len(m[0]) for m in molecules) if N is None else N
    capacity = max([len(m[2]) for m in molecules] + [1]) if capacity is None else capacity
    x = np.zeros((B, N, 3), dtype=np.float32)
    one_hot = np.zeros((B, N, nf), dtype=np.float32)
    node_mask = np.zeros((B, N), dtype=np.float32)
    bonds = np.zeros((B, capacity, 3), dtype=np.int32)
    n_bonds = np.zeros(B, dtype=np.int32)
    for b, (types, points, entries) in enumerate(molecules):
        n = len(types)
        x[b, :n] = np.asarray(points, dtype=np.float64).reshape(n, 3)
        one_hot[b, np.arange(n), types] = 1
        node_mask[b, :n] = 1
        n_bonds[b] = len(entries)
        if entries:
            bonds[b, :len(entries)] = np.asarray(entries, dtype=np.int32)
    return x, one_hot, node_mask, bonds, n_bonds


def hand_molecule(name):
    types, points, entries, _ = HAND[name]
    return types, points, entries


def strip(n_rings, last=6):
    """A straight strip of ``n_rings`` fused rings, hexagons (an acene, 4 n + 2 atoms) except that the last one has ``last``
    atoms: ``(types, points, bonds)``."""
    points = list(polygon(6))
    entries = cycle_bonds(range(6))
    a, b, centre = 0, 1, (0.0, 0.0, 0.0)
    for k in range(n_rings - 1):
        size = last if k == n_rings - 2 else 6
        new = fuse(points[a], points[b], centre, size)
        base = len(points)
        points += new
        chain = [b] + list(range(base, base + size - 2)) + [a]
        entries += [(chain[t], chain[t + 1], 1) for t in range(size - 1)]
        centre = centroid([points[t] for t in chain])
        a, b = base + 1, base + 2                 # the edge opposite the shared one
    return [C] * len(points), points, entries


def flake(rows, columns):
    """A parallelogram of ``rows x columns`` hexagons cut from the honeycomb: ``(types, points, bonds)`` with
    ``2 (rows + 1) (columns + 1) - 2`` carbon atoms; its chordless 6-cycles are its hexagons."""
    index, points, pairs = {}, [], set()
    for i in range(rows):
        for j in range(columns):
            cx, cy = math.sqrt(3) * EDGE * (j + 0.5 * i), 1.5 * EDGE * i
            ring = []
            for k in range(6):
                px = cx + EDGE * math.cos(math.radians(30 + 60 * k))
                py = cy + EDGE * math.sin(math.radians(30 + 60 * k))
                key = (round(px, 3), round(py, 3))
                if key not in index:
                    index[key] = len(points)
                    points.append((px, py, 0.0))
                ring.append(index[key])
            pairs.update((min(ring[k], ring[(k + 1) % 6]), max(ring[k], ring[(k + 1) % 6])) for k in range(6))
    return [C] * len(points), points, [(i, j, 1) for i, j in sorted(pairs)]


def random_fused(rng, max_atoms=40, noise=0.03):
    """A random fused system of hexagons and pentagons with per-atom noise, random hetero atoms, substituents and exocyclic
    double bonds: ``(types, points, bonds)``."""
    n0 = 6 if rng.random() < 0.7 else 5
    points = list(polygon(n0))
    entries = cycle_bonds(range(n0))
    rings = [list(range(n0))]
    degree = {k: 2 for k in range(n0)}
    target = int(rng.integers(1, 6))
    for _ in range(20):
        if len(rings) >= target:
            break
        ring = rings[int(rng.integers(len(rings)))]
        k = int(rng.integers(len(ring)))
        a, b = ring[k], ring[(k + 1) % len(ring)]
        if degree[a] > 2 or degree[b] > 2:
            continue
        n = 6 if rng.random() < 0.7 else 5
        new = fuse(points[a], points[b], centroid([points[t] for t in ring]), n)
        if len(points) + len(new) > max_atoms - 6:
            break
        if any(math.dist(p, q) < 1.2 for p in new for q in points):
            continue
        base = len(points)
        points += new
        chain = [b] + list(range(base, base + n - 2)) + [a]
        entries += [(chain[t], chain[t + 1], 1) for t in range(n - 1)]
        for t in range(base, base + n - 2):
            degree[t] = 2
        degree[a] += 1
        degree[b] += 1
        rings.append(chain)
    types = [C] * len(points)
    for k in range(len(points)):
        if rng.random() < 0.2:
            types[k] = [N_, N_, O, S][int(rng.integers(4))]
    middle = centroid(points)
    for k in list(degree):
        if degree[k] == 2 and rng.random() < 0.25 and len(points) < max_atoms:
            sub = outward(points[k], middle, 1.4)
            if any(math.dist(sub, q) < 1.2 for q in points):
                continue
            lift = float(rng.choice([0.0, 0.0, 0.0, 0.3, 1.0]))
            points.append((sub[0], sub[1], lift))
            types.append([C, O, N_][int(rng.integers(3))])
            entries.append((len(points) - 1, k, int(rng.choice([1, 1, 2]))))
    shake = rng.normal(0.0, noise, size=(len(points), 3))
    points = [tuple(float(v) for v in np.asarray(p) + s) for p, s in zip(points, shake)]
    return types, points, entries
