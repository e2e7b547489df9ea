"""The stereo rule of ``dl_stereo_perceive`` (``include/difflinker_hip.h``, ``csrc/stereo.hip``) restated in plain Python and
numpy: the classes by the root refinement of ``canon_ref``, the tetrahedral centres and the stereo double bonds, with every
fp64 operation rounded on its own in the header's order (Python floats are IEEE doubles and are never contracted).  The
kernel must agree in every output bit.  It is this project's own rule, NOT RDKit's stereo perception and NOT CIP.

Below the rule: ``read_stereo``, a reader for exactly the subset of SMILES that ``molecule_builder.smiles`` writes with
stereo; the labels a string states, re-expressed in the rule's terms; molecules with analytically placed atoms whose labels
are known from first principles; and a builder of random molecules."""
import math

import numpy as np

from canon_ref import _Graph

MAX_ATOMS, MAX_BONDS = 256, 2048
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, NONFINITE = 1, 4, 8, 64
FLAT, TWIST = 0.25, 0.5
V_IDEAL4, V_IDEAL3 = 16.0 / (3.0 * math.sqrt(3.0)), 4.0 / (3.0 * math.sqrt(3.0))
SHORT_ARM = 0.1
FIELDS = ('atom_class', 'atom_stereo', 'bond_stereo', 'counts', 'status')
FILL = 0x5a5a5a5a                                  # what an element the entry point does not write holds in the tests
C, O, N, F, S, CL, BR, I, P = range(9)             # the GEOM vocabulary
SYMBOL = ('C', 'O', 'N', 'F', 'S', 'Cl', 'Br', 'I', 'P')
DEFAULT_VALENCE = (4, 2, 3, 1, 2, 1, 1, 1, 3)


def default_valence(nf=8):
    return np.array(DEFAULT_VALENCE[:nf], dtype=np.int32)


# ---- the arithmetic: one rounding per operation ------------------------------------------------------------------------------
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def unit(v):
    """``v / |v|``, or None when ``v`` has zero length."""
    l2 = dot(v, v)
    if l2 == 0.0:
        return None
    n = math.sqrt(l2)
    return (v[0] / n, v[1] / n, v[2] / n)


def centre_volume(pos, c, ordered):
    """``(V, V_ideal)`` of centre ``c`` with its neighbours in class order, or None when one is at zero distance."""
    u = [unit(sub(pos[k], pos[c])) for k in ordered]
    if any(v is None for v in u):
        return None
    if len(u) == 4:
        return dot(sub(u[1], u[0]), cross(sub(u[2], u[0]), sub(u[3], u[0]))), V_IDEAL4
    return dot(u[0], cross(u[1], u[2])), V_IDEAL3


def bond_cosine(pos, lo, hi, ra, rb):
    """``(cos, |p|, |q|)`` of the double bond ``lo < hi`` with the reference neighbours ``ra`` of ``lo`` and ``rb`` of ``hi``;
    ``cos`` is None when an arm is shorter than ``SHORT_ARM``; None when the bond has zero length."""
    e = unit(sub(pos[hi], pos[lo]))
    if e is None:
        return None
    wa, wb = sub(pos[ra], pos[lo]), sub(pos[rb], pos[hi])
    sa, sb = dot(wa, e), dot(wb, e)
    p, q = sub(wa, (sa * e[0], sa * e[1], sa * e[2])), sub(wb, (sb * e[0], sb * e[1], sb * e[2]))
    lp, lq = math.sqrt(dot(p, p)), math.sqrt(dot(q, q))
    if lp < SHORT_ARM or lq < SHORT_ARM:
        return None, lp, lq
    return dot(p, q) / (lp * lq), lp, lq


def ring_path(adj, u, v):
    """Bonds of the shortest path from ``u`` to ``v`` that does not use the pair ``(u, v)``, or -1."""
    seen, frontier, level = {u}, [t for t in adj[u] if t != v], 1
    seen.update(frontier)
    while frontier:
        if v in frontier:
            return level
        nxt = []
        for a in frontier:
            for t in adj[a]:
                if t not in seen:
                    seen.add(t)
                    nxt.append(t)
        frontier, level = nxt, level + 1
    return -1


def molecule(x, types, mask, entries, n_bonds_in, valences, flat=FLAT, twist=TWIST, status_in=0, drop=None, mark=None,
             planar=None, aromatic=None, detail=None):
    """One molecule: ``x [N][3]`` float32, ``types [N]``, ``mask`` / ``drop`` / ``mark`` ``[N]`` by row, ``entries`` the
    ``capacity`` rows of its list, ``planar [N]`` by atom number, ``aromatic [capacity]`` by entry.  Returns ``(atom_class [N],
    atom_stereo [N], bond_stereo [capacity], counts [2][4], status)``.  ``detail``, a dict, receives the decision quantities:
    ``centres`` ``(atom, neighbours by class, V, V_ideal)`` and ``bonds`` ``(lo, hi, ra, rb, cos, |p|, |q|)``."""
    N, capacity = len(mask), len(entries)
    real = [r for r in range(N) if mask[r] != 0]
    n = len(real)
    kept = [not (drop is not None and drop[r] != 0) for r in real]
    marked = [mark is not None and mark[r] != 0 for r in real]
    counts = [[0] * 4, [0] * 4]
    status = int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0)
    neutral = ([-1] * N, [-1] * N, [0] * capacity, counts)
    if sum(kept) > MAX_ATOMS:
        return neutral + (status | TOO_LARGE,)
    new = {}
    for k in range(n):
        if kept[k]:
            new[k] = len(new)
    pairs, no_bond, repeated, every = {}, False, False, []
    for e in range(min(max(int(n_bonds_in), 0), capacity)):
        i, j, order = (int(v) for v in entries[e])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 3):
            no_bond = True
            continue
        if not (kept[i] and kept[j]):
            continue
        every.append((new[i], new[j], order))
        key = (min(i, j), max(i, j))
        if key in pairs:
            repeated = True
            continue
        pairs[key] = (order, e)
    if len(every) > MAX_BONDS:
        return neutral + (status | TOO_LARGE | (BAD_BOND if no_bond else 0),)
    status |= BAD_BOND if no_bond or repeated else 0
    atoms = sorted(new)
    kind = {k: int(types[real[k]]) for k in atoms}
    tied = _Graph([kind[k] for k in atoms], every).root() if atoms else []
    cls = {k: tied[new[k]] for k in atoms}
    atom_class = [cls.get(k, -1) for k in range(N)]
    atom_stereo = [0 if k in cls else -1 for k in range(N)]
    bond_stereo = [0] * capacity
    pos = {k: tuple(float(x[real[k]][c]) for c in range(3)) for k in atoms}
    if any(not math.isfinite(v) for p in pos.values() for v in p):
        return atom_class, atom_stereo, bond_stereo, counts, status | NONFINITE

    def count(which, *members):
        counts[0][which] += 1
        counts[1][which] += any(marked[a] for a in members)

    found = {'centres': [], 'bonds': []}
    adj = {k: [] for k in atoms}
    for a, j in sorted(pairs):
        adj[a].append(j)
        adj[j].append(a)
    order_of = lambda a, t: pairs[(min(a, t), max(a, t))][0]          # noqa: E731
    for c in atoms:
        orders = [order_of(c, t) for t in adj[c]]
        d, h = len(orders), max(0, int(valences[kind[c]]) - sum(orders))
        if (planar is not None and planar[c] != 0) or any(o != 1 for o in orders) or (d, h) not in ((4, 0), (3, 1)):
            continue
        ordered = sorted(adj[c], key=lambda t: cls[t])
        if len({cls[t] for t in ordered}) != d:
            continue
        volume = centre_volume(pos, c, ordered)
        label = 3
        if volume is not None:
            V, ideal = volume
            T = flat * ideal
            label = 1 if V > T else 2 if V < -T else 3
        found['centres'].append((c, ordered) + (volume or (None, None)))
        atom_stereo[c] = label
        count(1 if label == 3 else 0, c, *ordered)

    def reference(u, v):
        others = [t for t in adj[u] if t != v]
        if not 1 <= len(others) <= 2 or any(order_of(u, t) != 1 for t in others):
            return None
        if len(others) == 2 and cls[others[0]] == cls[others[1]]:
            return None
        return max(others, key=lambda t: cls[t])

    for (lo, hi), (order, e) in sorted(pairs.items()):
        if order != 2 or (aromatic is not None and aromatic[e] != 0):
            continue
        ra, rb = reference(lo, hi), reference(hi, lo)
        if ra is None or rb is None:
            continue
        path = ring_path(adj, lo, hi)
        if path >= 0 and path + 1 < 8:
            continue
        got = bond_cosine(pos, lo, hi, ra, rb)
        label = 3
        if got is not None and got[0] is not None:
            label = 1 if got[0] > twist else 2 if got[0] < -twist else 3
        found['bonds'].append((lo, hi, ra, rb) + (got or (None, None, None)))
        bond_stereo[e] = label
        count(3 if label == 3 else 2, lo, hi, ra, rb)
    if detail is not None:
        detail.update(found)
    return atom_class, atom_stereo, bond_stereo, counts, status


def first_largest(one_hot):
    return np.argmax(np.asarray(one_hot), axis=-1)


def perceive(x, one_hot, node_mask, bonds, n_bonds_in, valences=None, flat=FLAT, twist=TWIST, status_in=None, drop_mask=None,
             mark_mask=None, atom_planar=None, bond_aromatic=None):
    """The whole batch with the entry point's shapes.  Returns int32 arrays by the names of ``FIELDS``."""
    x, node_mask, bonds = np.asarray(x, dtype=np.float32), np.asarray(node_mask), np.asarray(bonds)
    B, N = node_mask.shape
    capacity = bonds.shape[1]
    types = first_largest(one_hot)
    valences = default_valence(np.asarray(one_hot).shape[2]) if valences is None else valences
    out = {'atom_class': np.zeros((B, N), np.int32), 'atom_stereo': np.zeros((B, N), np.int32),
           'bond_stereo': np.zeros((B, capacity), np.int32), 'counts': np.zeros((B, 2, 4), np.int32), 'status': np.zeros(B, np.int32)}
    pick = lambda t, b: None if t is None else np.asarray(t)[b]     # noqa: E731
    for b in range(B):
        got = molecule(x[b], types[b], node_mask[b], bonds[b], int(n_bonds_in[b]), valences, flat, twist,
                       0 if status_in is None else int(status_in[b]), pick(drop_mask, b), pick(mark_mask, b),
                       pick(atom_planar, b), pick(bond_aromatic, b))
        for name, value in zip(FIELDS, got):
            out[name][b] = value
    return out


def perceive_one(m, flat=FLAT, twist=TWIST, detail=None):
    """``molecule`` on a molecule dict (``types``, ``points``, ``entries``; optional ``planar``, ``marked``, ``dropped`` by atom
    number and ``aromatic`` by entry), every atom on its own row.  Returns a dict by ``FIELDS``."""
    n, entries = len(m['types']), [tuple(e) for e in m['entries']]
    flags = lambda name, size: [1 if k in m.get(name, ()) else 0 for k in range(size)]       # noqa: E731
    x = np.asarray(m['points'], dtype=np.float32).reshape(n, 3)
    got = molecule(x, m['types'], [1] * n, entries, len(entries), DEFAULT_VALENCE, flat, twist, 0, flags('dropped', n),
                   flags('marked', n), flags('planar', n), flags('aromatic', len(entries)), detail)
    return dict(zip(FIELDS, got))


def clearance(detail, flat=FLAT, twist=TWIST):
    """The smallest distance of a decision quantity from its threshold: ``||V| - flat V_ideal|``, ``||cos| - twist||`` and
    ``|p|, |q| - 0.1`` (inf without decisions; 0 for a zero-length vector)."""
    least = math.inf
    for _, _, V, ideal in detail['centres']:
        least = min(least, abs(abs(V) - flat * ideal) if V is not None else 0.0)
    for _, _, _, _, c, lp, lq in detail['bonds']:
        if lp is None:
            return 0.0
        least = min(least, abs(lp - SHORT_ARM), abs(lq - SHORT_ARM))
        if c is not None:
            least = min(least, abs(abs(c) - twist))
    return least


# ---- the widened types of the stereo-aware codes -------------------------------------------------------------------------------
def wide_types(types, entries, atom_stereo, bond_stereo, mirror=False):
    """``type * 16 + atom_label * 4 + bond_label`` per atom, as ``metrics.stereo_types`` forms it."""
    swap = {1: 2, 2: 1} if mirror else {1: 1, 2: 2}
    on_bond = [0] * len(types)
    for (i, j, _), label in zip(entries, bond_stereo):
        if label in (1, 2):
            on_bond[i] += label
            on_bond[j] += label
    return [t * 16 + swap.get(s, 0) * 4 + b for t, s, b in zip(types, atom_stereo, on_bond)]


# ---- the reader ------------------------------------------------------------------------------------------------------------------
_ELEMENTS = sorted(SYMBOL, key=len, reverse=True)


def read_stereo(text):
    """What a string of ``molecule_builder.smiles`` (with stereo) says, atoms numbered in written order: a dict with ``types``,
    ``bonds`` ``(i, j, order)``, ``centres`` ``{atom: (neighbours in string order, -1 for the implicit H; sign)}`` with sign
    -1 for ``@`` (anticlockwise seen from the first, a negative determinant) and +1 for ``@@``, and ``double_bonds``
    ``[(a, b, na, nb, cis)]``: the neighbours ``na`` of ``a`` and ``nb`` of ``b`` whose single bonds carry a direction symbol,
    and whether the string puts them on one side.  Exactly the subset the writer emits; anything else is a ``ValueError``."""
    types, bonds, centres, neighbours = [], [], {}, []
    direction = {}                                   # (first written, second written) -> +1 for '/', -1 for '\'
    open_rings, branch, previous, order, symbol, at = {}, [], None, 1, 0, 0

    def fail(why):
        raise ValueError(f'{why} at {at} in {text!r}')

    while at < len(text):
        ch = text[at]
        at += 1
        if ch == '.':
            if branch or order != 1 or symbol:
                fail('a dangling bond')
            previous = None
        elif ch == '(':
            branch.append(previous)
        elif ch == ')':
            previous = branch.pop()
        elif ch in '=#':
            order = 2 if ch == '=' else 3
        elif ch in '/\\':
            symbol = 1 if ch == '/' else -1
        elif ch.isdigit() or ch == '%':
            k = int(ch) if ch != '%' else int(text[at:at + 2])
            at += 0 if ch != '%' else 2
            if k in open_rings:
                other, opened, said, slot = open_rings.pop(k)
                if order != 1:
                    fail('the closing end carries no order')
                if symbol and said and said != -symbol:
                    fail('the two ends of a ring closure disagree')
                said = said or -symbol
                bonds.append((other, previous, opened))
                if said:
                    direction[(other, previous)] = said
                neighbours[other][slot] = previous
                neighbours[previous].append(other)
            else:
                open_rings[k] = (previous, order, symbol, len(neighbours[previous]))
                neighbours[previous].append(None)
            order, symbol = 1, 0
        else:
            sign, hydrogen = 0, False
            if ch == '[':
                close = text.index(']', at)
                inside, at = text[at:close], close + 1
                name = next((el for el in _ELEMENTS if inside.startswith(el)), None)
                if name is None:
                    fail('an unknown element')
                rest = inside[len(name):]
                if rest.startswith('@@'):
                    sign, rest = 1, rest[2:]
                elif rest.startswith('@'):
                    sign, rest = -1, rest[1:]
                if rest not in ('', 'H'):
                    fail('an unknown bracket atom')
                hydrogen = rest == 'H'
            else:
                name = next((el for el in _ELEMENTS if text.startswith(el, at - 1)), None)
                if name is None:
                    fail('an unknown character')
                at += len(name) - 1
            me = len(types)
            types.append(SYMBOL.index(name))
            neighbours.append([])
            if previous is not None:
                bonds.append((previous, me, order))
                if symbol:
                    if order != 1:
                        fail('a direction on a multiple bond')
                    direction[(previous, me)] = symbol
                neighbours[previous].append(me)
                neighbours[me].append(previous)
            if hydrogen:
                neighbours[me].append(-1)
            if sign:
                centres[me] = sign
            previous, order, symbol = me, 1, 0
    if open_rings or branch:
        fail('an open ring or branch')
    for c in centres:
        if len(neighbours[c]) != 4:
            fail(f'centre {c} without four neighbours')
    outward = {}                                     # (double-bond atom, neighbour) -> the symbol read from the atom outward
    for (first, second), said in direction.items():
        outward[(first, second)] = said
        outward[(second, first)] = -said
    double_bonds = []
    for a, b, o in bonds:
        if o != 2:
            continue
        arms = [[t for t in neighbours[u] if t not in (v, -1) and (u, t) in outward] for u, v in ((a, b), (b, a))]
        if not arms[0] or not arms[1]:
            continue
        for u, mine in zip((a, b), arms):            # two symbols at one end must put their atoms on opposite sides
            if len(mine) == 2 and outward[(u, mine[0])] == outward[(u, mine[1])]:
                fail(f'the two symbols at atom {u} contradict each other')
        na, nb = arms[0][0], arms[1][0]
        double_bonds.append((a, b, na, nb, outward[(a, na)] == outward[(b, nb)]))
    return dict(types=types, bonds=bonds, centres={c: (neighbours[c], s) for c, s in centres.items()}, double_bonds=double_bonds)


def parity(sequence):
    """+1 for an even permutation, -1 for an odd one: the sign of the number of inversions."""
    s = list(sequence)
    return -1 if sum(1 for q in range(len(s)) for p in range(q) if s[p] > s[q]) % 2 else 1


def written_order(n, bonds, rank):
    """The order in which ``molecule_builder.smiles`` writes the atoms: depth first from the atom of smallest rank of every
    piece, neighbours in ascending rank.  ``order[k]`` is the atom written k-th."""
    adj = [set() for _ in range(n)]
    for i, j, _ in bonds:
        adj[i].add(j)
        adj[j].add(i)
    order, seen = [], set()
    for root in sorted(range(n), key=lambda u: rank[u]):
        stack = [root]
        while stack:
            u = stack.pop()
            if u in seen:
                continue
            seen.add(u)
            order.append(u)
            stack.extend(sorted((w for w in adj[u] if w not in seen), key=lambda w: -rank[w]))
    return order


def stated_labels(read, order, classes, n, pairs):
    """The labels a string states, in the rule's terms: ``read`` of ``read_stereo``, ``order`` of ``written_order`` (written
    position -> atom), ``classes`` per atom, ``pairs`` the molecule's ``{(lo, hi): order}``.  Returns ``(atom labels [n] with
    0 where the string says nothing, {(lo, hi): label})``."""
    atom = [0] * n
    for c, (around, sign) in read['centres'].items():
        keys = [-1 if t == -1 else classes[order[t]] for t in around]         # the H is a class below all others
        atom[order[c]] = 1 if sign * parity(keys) > 0 else 2
    adj = {}
    for lo, hi in pairs:
        adj.setdefault(lo, []).append(hi)
        adj.setdefault(hi, []).append(lo)
    bond = {}
    for a, b, na, nb, cis in read['double_bonds']:
        a, b, na, nb = order[a], order[b], order[na], order[nb]
        for u, v, t in ((a, b, na), (b, a, nb)):     # an arm that is not the reference neighbour is across from it
            others = [w for w in adj[u] if w != v]
            if t != max(others, key=lambda w: classes[w]):
                cis = not cis
        bond[(min(a, b), max(a, b))] = 1 if cis else 2
    return atom, bond


# ---- molecules with analytically placed atoms ----------------------------------------------------------------------------------
TET = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]     # det[t1 - t0, t2 - t0, t3 - t0] = -16 and det[t1, t2, t3] = -4
TET_SIGN = -1                                                # the sign of both: NEGATIVE in the order 0, 1, 2, 3


def tet(centre, k, length=1.5):
    g = length / math.sqrt(3.0)
    return tuple(c + g * t for c, t in zip(centre, TET[k]))


def arm(origin, degrees, length=1.4):
    """A point in the plane z = 0 at ``degrees`` from +x."""
    return (origin[0] + length * math.cos(math.radians(degrees)), origin[1] + length * math.sin(math.radians(degrees)), 0.0)


def mol(types, points, entries, **more):
    return dict(types=list(types), points=[tuple(float(v) for v in p) for p in points], entries=[tuple(e) for e in entries], **more)


def olefin(left, right, cis, twist_degrees=0.0):
    """``left`` and ``right``: the types of the substituents at the two ends, one or two each, the FIRST at +-120 degrees on
    the upper side of atom 0 (and of atom 1 when ``cis``).  Atoms: 0 = 1 the double bond, then left's, then right's.  The right
    end is turned about the bond by ``twist_degrees``."""
    a, b = (0.0, 0.0, 0.0), (1.34, 0.0, 0.0)
    points, types, entries = [a, b], [C, C], [(0, 1, 2)]
    for k, t in enumerate(left):
        points.append(arm(a, 120 if k == 0 else -120))
        types.append(t)
        entries.append((0, len(types) - 1, 1))
    c, s = math.cos(math.radians(twist_degrees)), math.sin(math.radians(twist_degrees))
    for k, t in enumerate(right):
        up = (k == 0) == bool(cis)
        x, y, _ = arm(b, 60 if up else -60)
        points.append((x, y * c, y * s))
        types.append(t)
        entries.append((1, len(types) - 1, 1))
    return mol(types, points, entries)


def ring(n, double_at=(0,), radius=None):
    """A planar ring of ``n`` carbons with double bonds after the atoms of ``double_at``."""
    radius = radius or 1.4 / (2 * math.sin(math.pi / n))
    points = [(radius * math.cos(2 * math.pi * k / n), radius * math.sin(2 * math.pi * k / n), 0.0) for k in range(n)]
    return mol([C] * n, points, [(k, (k + 1) % n, 2 if k in double_at else 1) for k in range(n)])


def hexadiene(first_cis, second_cis):
    """CH3-CH=CH-CH=CH-CH3 in a plane, atoms 0..5 along the chain; each double bond cis or trans as asked."""
    points, heading, turn = [(0.0, 0.0, 0.0)], 0.0, 1
    cis = {1: first_cis, 3: second_cis}              # the bond k -> k+1 that is double
    for k in range(5):
        points.append(arm(points[-1], heading))
        if k < 4:
            turn = turn if cis.get(k, False) else -turn              # cis: turn the same way twice; single bonds: s-trans
            heading += 60 * turn
    return mol([C] * 6, points, [(k, k + 1, 2 if k in (1, 3) else 1) for k in range(5)])


def tartaric(first, second):
    """HOOC-CH(OH)-CH(OH)-COOH as the skeleton C(O)(=O) C(O) C(O) C(O)(=O): centres 1 and 2 with the hand ``first`` and
    ``second`` (+1 or -1) choosing which of two tetrahedral slots the acid C and the O take.  Centre 2's frame is the point
    inversion of centre 1's, and an inversion exchanges the hands: EQUAL signs give the meso compound (it has an inversion
    centre), in its two numberings; DIFFERENT signs give the two enantiomers of the chiral one."""
    c1, c2 = (0.0, 0.0, 0.0), tet((0.0, 0.0, 0.0), 0)
    # centre 1: the other centre at TET[0]; acid C, O and the implicit H among TET[1..3]
    slots1 = (1, 2) if first > 0 else (2, 1)
    acid1, o1 = tet(c1, slots1[0]), tet(c1, slots1[1])
    # centre 2 looks back along -TET[0]; its other three directions are the negatives of TET[1..3]
    back = lambda k: tuple(c - (p - q) for c, p, q in zip(c2, tet(c1, k), c1))               # noqa: E731
    slots2 = (1, 2) if second > 0 else (2, 1)
    acid2, o2 = back(slots2[0]), back(slots2[1])
    points = [acid1, c1, c2, acid2, o1, o2]
    types, entries = [C, C, C, C, O, O], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 4, 1), (2, 5, 1)]
    for acid, at in ((0, acid1), (3, acid2)):        # the acid's =O and -OH, out of the way of everything else
        away = tuple(2 * p - q for p, q in zip(at, c1 if acid == 0 else c2))
        points += [tuple(v + dv for v, dv in zip(away, (0.0, 0.0, 0.6))), tuple(v + dv for v, dv in zip(away, (0.0, 0.0, -0.6)))]
        types += [O, O]
        entries += [(acid, len(types) - 2, 2), (acid, len(types) - 1, 1)]
    return mol(types, points, entries)


def _hand():
    o = (0.0, 0.0, 0.0)
    out = {}
    # CHFClBr: F, Cl, Br on TET[1..3] in that order, the H on TET[0]
    out['chfclbr_a'] = mol([C, F, CL, BR], [o, tet(o, 1), tet(o, 2), tet(o, 3)], [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
    out['chfclbr_b'] = mol([C, F, CL, BR], [o, tet(o, 2), tet(o, 1), tet(o, 3)], [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
    # L-alanine, (S): looking from the H (TET[0]) ... see test_stereo_host for the derivation.  Atoms: N, CA, CB, C, O, OH
    ca = o
    c_acid = tet(ca, 3)
    away = tuple(2 * p for p in c_acid)
    out['l_alanine'] = mol([N, C, C, C, O, O],
                           [tet(ca, 1), ca, tet(ca, 2), c_acid, tuple(v + dv for v, dv in zip(away, (0.0, 0.0, 0.6))),
                            tuple(v + dv for v, dv in zip(away, (0.0, 0.0, -0.6)))],
                           [(0, 1, 1), (1, 2, 1), (1, 3, 1), (3, 4, 2), (3, 5, 1)])
    out['e_butene'], out['z_butene'] = olefin([C], [C], cis=False), olefin([C], [C], cis=True)
    out['e_difluoroethene'], out['z_difluoroethene'] = olefin([F], [F], cis=False), olefin([F], [F], cis=True)
    for name, cis in (('oxime_e', False), ('oxime_z', True)):        # C-C=N-O
        m = olefin([C], [O], cis=cis)
        m['types'][1] = N
        out[name] = m
    out['cyclohexene'], out['cyclooctene'] = ring(6), ring(8)
    out['benzene'] = dict(ring(6, (0, 2, 4)), aromatic=list(range(6)), planar=list(range(6)))
    out['isobutene'], out['methylbutene'] = olefin([C, C], [], cis=True), olefin([C, C], [C], cis=True)
    # 3-pentyl: a CH with two ethyls and an O: two neighbours tie
    c = o
    out['pentan_3_ol'] = mol([C, C, C, O, C, C], [c, tet(c, 1), tet(c, 2), tet(c, 3), tet(tet(c, 1), 0), tet(tet(c, 2), 0)],
                             [(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 5, 1)])
    out['trimethylamine'] = mol([N, C, C, C], [o, tet(o, 1), tet(o, 2), tet(o, 3)], [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
    out['amine'] = mol([N, C, O, F], [o, tet(o, 1), tet(o, 2), tet(o, 3)], [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
    out['ammonium'] = mol([N, C, O, F, S], [o, tet(o, 0), tet(o, 1), tet(o, 2), tet(o, 3)], [(0, k, 1) for k in (1, 2, 3, 4)])
    out['sulfoxide'] = mol([S, O, C, C, C], [o, tet(o, 1), tet(o, 2), tet(o, 3), tet(tet(o, 3), 0)],
                           [(0, 1, 2), (0, 2, 1), (0, 3, 1), (3, 4, 1)])
    out['allene'] = mol([C, C, C, F, F], [(0.0, 0.0, 0.0), (1.3, 0.0, 0.0), (2.6, 0.0, 0.0), arm(o, 120), (3.3, 0.0, 1.2)],
                        [(0, 1, 2), (1, 2, 2), (0, 3, 1), (2, 4, 1)])
    for name, a, b in (('hexadiene_ee', False, False), ('hexadiene_ez', False, True), ('hexadiene_zz', True, True)):
        out[name] = hexadiene(a, b)
    for name, a, b in (('tartaric_meso_12', 1, 1), ('tartaric_meso_21', -1, -1), ('tartaric_chiral_a', 1, -1),
                       ('tartaric_chiral_b', -1, 1)):
        out[name] = tartaric(a, b)
    return out


HAND = _hand()
# what the rule must find, from first principles.  CENTRES: atom -> its neighbours on TET[1], TET[2], TET[3] of ``tet`` (the
# fourth neighbour or the implicit H is on TET[0]): the determinant of the rule in THAT order has the sign TET_SIGN, so the
# label follows from the parity of the permutation that sorts those neighbours by class.  DOUBLE BONDS: (lo, hi) -> 1 cis, 2
# trans; every end has ONE other neighbour in these molecules, which is its reference neighbour whatever the classes are
CENTRES = {'chfclbr_a': {0: (1, 2, 3)}, 'chfclbr_b': {0: (2, 1, 3)}, 'l_alanine': {1: (0, 2, 3)}, 'ammonium': {0: (2, 3, 4)}}
DOUBLE_BONDS = {
    'e_butene': {(0, 1): 2}, 'z_butene': {(0, 1): 1}, 'e_difluoroethene': {(0, 1): 2}, 'z_difluoroethene': {(0, 1): 1},
    'oxime_e': {(0, 1): 2}, 'oxime_z': {(0, 1): 1}, 'cyclooctene': {(0, 1): 1},
    'hexadiene_ee': {(1, 2): 2, (3, 4): 2}, 'hexadiene_ez': {(1, 2): 2, (3, 4): 1}, 'hexadiene_zz': {(1, 2): 1, (3, 4): 1},
}
NOTHING = ('cyclohexene', 'benzene', 'isobutene', 'methylbutene', 'pentan_3_ol', 'trimethylamine', 'amine', 'sulfoxide', 'allene')


def expected_centre(classes, on_tet123, fourth=None):
    """The label of a centre whose neighbours ``on_tet123`` sit on TET[1..3] and ``fourth`` (None: the implicit H, the lowest
    class) on TET[0]."""
    keys = [-1 if fourth is None else classes[fourth]] + [classes[t] for t in on_tet123]
    return 1 if TET_SIGN * parity(keys) > 0 else 2


# ---- random molecules ------------------------------------------------------------------------------------------------------------
def random_molecule(rng, max_atoms=24, min_atoms=1):
    """A random forest of ``min_atoms..max_atoms`` atoms with a few ring closures, of at most four bonds per atom: every atom
    but the first of a piece lies 1.1 to 1.7 A from its parent in a random direction that leans away from the parent's other
    neighbours, so that centres of both hands, flat
    centres, cis, trans and twisted double bonds all occur; orders, flags, marks and dropped atoms are drawn at random."""
    n = int(rng.integers(min_atoms, max_atoms + 1))
    types = [int(t) for t in rng.choice([C, C, C, C, C, C, C, N, O, O, S, F, CL], n)]
    points, degree, entries, seen = [], [0] * n, [], set()

    def join(i, j):
        order = int(rng.choice([1, 1, 1, 1, 1, 1, 1, 2, 2, 3]))
        entries.append((i, j, order) if rng.random() < 0.5 else (j, i, order))
        seen.add((min(i, j), max(i, j)))
        degree[i] += 1
        degree[j] += 1

    for i in range(n):
        open_ = [j for j in range(i) if degree[j] < 4]
        if open_ and rng.random() < 0.95:
            near = open_[-5:]
            weight = np.array([1.0 + 2.0 * degree[j] for j in near])  # branch: centres need three or four neighbours
            j = int(rng.choice(near, p=weight / weight.sum()))
            step = rng.normal(0, 1, 3)
            for i_, j_, _ in entries:                 # away from the parent's other neighbours, more or less
                if j in (i_, j_):
                    away = np.asarray(points[j]) - np.asarray(points[i_ + j_ - j])
                    step += rng.uniform(0.0, 2.0) * away / np.linalg.norm(away)
            step *= rng.uniform(1.1, 1.7) / np.linalg.norm(step)
            points.append(tuple(float(v) for v in np.asarray(points[j]) + step))
            join(i, j)
        else:                                        # a new piece
            points.append(tuple(float(v) for v in rng.normal(0, 2.5, 3)))
    for _ in range(int(rng.integers(0, 3))):
        if n > 8:
            i, j = (int(v) for v in rng.choice(n, 2, replace=False))
            if (min(i, j), max(i, j)) not in seen and degree[i] < 4 and degree[j] < 4:
                join(i, j)
    shuffled = rng.permutation(len(entries))
    return dict(types=types, points=points, entries=[entries[k] for k in shuffled],
                planar=[k for k in range(n) if rng.random() < 0.1], marked=[k for k in range(n) if rng.random() < 0.3],
                dropped=[k for k in range(n) if rng.random() < 0.1],
                aromatic=[e for e in range(len(entries)) if rng.random() < 0.1])


def random_molecules(seed, count, max_atoms=24, margin=2e-3):
    """``count`` molecules drawn one by one from ``seed``; a molecule with a decision quantity within ``margin`` of its
    threshold is drawn again."""
    rng, out = np.random.default_rng(seed), []
    while len(out) < count:
        m, detail = random_molecule(rng, max_atoms), {}
        perceive_one(m, detail=detail)
        if clearance(detail) >= margin:
            out.append(m)
    return out


def renumbered(m, rng):
    """``m`` with its atoms renumbered by a random permutation and its entries shuffled; ``(molecule, new number of atom k)``."""
    n = len(m['types'])
    sigma = [int(v) for v in rng.permutation(n)]
    types, points = [None] * n, [None] * n
    for k in range(n):
        types[sigma[k]], points[sigma[k]] = m['types'][k], m['points'][k]
    order = [int(v) for v in rng.permutation(len(m['entries']))]
    out = dict(types=types, points=points, entries=[(sigma[m['entries'][e][0]], sigma[m['entries'][e][1]], m['entries'][e][2]) for e in order])
    for name in ('planar', 'marked', 'dropped'):
        out[name] = sorted(sigma[k] for k in m.get(name, ()))
    out['aromatic'] = sorted(order.index(e) for e in m.get('aromatic', ()))
    return out, sigma


def as_batch(molecules, N, capacity=None, nf=8, rng=None, scatter=True):
    """``pose_checks_ref.as_batch`` plus ``bond_aromatic [B,capacity]`` from the molecules' ``aromatic`` entries."""
    import pose_checks_ref
    full = [{'planar': [], 'marked': [], 'dropped': [], **m, 'types': np.asarray(m['types'], dtype=np.int64)} for m in molecules]
    out = pose_checks_ref.as_batch(full, N, capacity, nf, rng, scatter)
    out['bond_aromatic'] = np.zeros(out['bonds'].shape[:2], np.int32)
    for b, m in enumerate(molecules):
        for e in m.get('aromatic', ()):
            if e < out['bonds'].shape[1]:
                out['bond_aromatic'][b, e] = 1
    return out
