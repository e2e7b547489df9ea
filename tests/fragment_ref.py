"""The double-cut rule of ``dl_fragment_cuts`` (``include/difflinker_hip.h``, ``csrc/fragment.hip``) restated in plain
Python: flood fills with a bond removed, a breadth-first search for the path, a double loop over bond pairs.  The kernel must
agree exactly: integers, order of records, labels, status.

Atom ``k`` is the k-th row with ``node_mask != 0``, its type the first largest entry of its ``one_hot`` row; an entry
``(i, j, order)`` is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 4``, in either orientation; of a
repeated pair the first entry counts."""
from collections import deque

import numpy as np

MAX_ATOMS, CUT_FIELDS = 256, 10
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, DISCONNECTED, TRUNCATED = 1, 4, 8, 16, 32
FIELDS = ('n_atoms', 'n_bonds', 'n_cuttable', 'n_cuts', 'status', 'bond_side', 'cuts', 'labels')
DEFAULTS = {'min_linker': 3, 'min_fragment': 5, 'min_path_atoms': 2, 'linker_leq_frags': 1}
CARBON = 0                                       # the type the hand molecules call carbon
C, N_, O = 0, 1, 2                               # types of the hand molecules


def reachable(adj, start, without=None):
    """Atoms that can be reached from ``start``; ``without`` is a bond ``(u, v)`` that may not be walked."""
    seen = {start}
    queue = deque([start])
    while queue:
        w = queue.popleft()
        for t in adj[w]:
            if without is not None and {w, t} == set(without):
                continue
            if t not in seen:
                seen.add(t)
                queue.append(t)
    return seen


def distance(adj, start, goal):
    dist = {start: 0}
    queue = deque([start])
    while queue:
        w = queue.popleft()
        if w == goal:
            return dist[w]
        for t in adj[w]:
            if t not in dist:
                dist[t] = dist[w] + 1
                queue.append(t)
    return -1


def first_largest(row):
    best = 0
    for t in range(1, len(row)):
        if row[t] > row[best]:
            best = t
    return best


def molecule(mask, one_hot, entries, n_bonds_in, R, charge=None, status_in=0, carbon_type=CARBON, **rule):
    """One molecule: ``mask [N]``, ``one_hot [N][nf]``, ``charge [N]`` by row, ``entries`` the whole list ``[capacity][3]``.
    Returns a dict of ``FIELDS``: ints, ``bond_side [capacity]``, ``cuts [R][10]``, ``labels [R][N]``."""
    rule = dict(DEFAULTS, **rule)
    N, capacity = len(mask), len(entries)
    rows = [r for r in range(N) if mask[r] != 0]
    n = len(rows)
    out = {'n_atoms': n, 'n_bonds': 0, 'n_cuttable': 0, 'n_cuts': 0,
           'status': int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0),
           'bond_side': [0] * capacity, 'cuts': [[0] * CUT_FIELDS for _ in range(R)], 'labels': [[255] * N for _ in range(R)]}
    if n > MAX_ATOMS:
        out['status'] |= TOO_LARGE
        return out
    carbon = [first_largest(one_hot[r]) == carbon_type for r in rows]
    neutral = [charge is None or int(charge[r]) == 0 for r in rows]

    bonds, bad = {}, False                       # (lo, hi) -> (first entry, i, j, order), in list order
    for e in range(min(max(int(n_bonds_in), 0), capacity)):
        i, j, order = (int(v) for v in entries[e])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 4):
            bad = True
        elif (min(i, j), max(i, j)) in bonds:
            bad = True
        else:
            bonds[(min(i, j), max(i, j))] = (e, i, j, order)
    out['n_bonds'] = len(bonds)
    out['status'] |= BAD_BOND if bad else 0
    adj = {k: set() for k in range(n)}
    hetero_multiple = [False] * n                # a double or triple bond to an atom that is no carbon
    for e, i, j, order in bonds.values():
        adj[i].add(j)
        adj[j].add(i)
        if order in (2, 3):
            hetero_multiple[i] = hetero_multiple[i] or not carbon[j]
            hetero_multiple[j] = hetero_multiple[j] or not carbon[i]

    def carbon_end(k):
        return carbon[k] and neutral[k] and not hetero_multiple[k]

    everything = set(range(n))
    cuttable = []                                # (entry, i, j, the atoms on i's side, the atoms on j's side)
    for e, i, j, order in bonds.values():
        if order != 1 or not (carbon_end(i) or carbon_end(j)):
            continue
        side = reachable(adj, i, without=(i, j))
        if j in side:                            # a ring bond
            continue
        cuttable.append((e, i, j, side, everything - side))
        out['bond_side'][e] = len(side)
    out['n_cuttable'] = len(cuttable)
    if n and len(reachable(adj, 0)) != n:
        out['status'] |= DISCONNECTED
        return out

    for a in range(len(cuttable)):
        for b in range(a + 1, len(cuttable)):
            (e1, i1, j1, side1, other1), (e2, i2, j2, side2, other2) = cuttable[a], cuttable[b]
            # fragment 1 is the side of e1 that does not hold e2
            anchor1, exit1, frag1 = (j1, i1, other1) if i2 in side1 else (i1, j1, side1)
            anchor2, exit2, frag2 = (j2, i2, other2) if i1 in side2 else (i2, j2, side2)
            n_linker = n - len(frag1) - len(frag2)
            if n_linker < rule['min_linker'] or min(len(frag1), len(frag2)) < rule['min_fragment']:
                continue
            if rule['linker_leq_frags'] and n_linker > min(len(frag1), len(frag2)):
                continue
            path_atoms = distance(adj, exit1, exit2) + 1
            if path_atoms < rule['min_path_atoms']:
                continue
            r = out['n_cuts']
            out['n_cuts'] += 1
            if r < R:
                out['cuts'][r] = [e1, e2, anchor1, exit1, anchor2, exit2, len(frag1), len(frag2), n_linker, path_atoms]
                out['labels'][r] = [(0 if k in frag1 else 1 if k in frag2 else 2) if k < n else 255 for k in range(N)]
    out['status'] |= TRUNCATED if out['n_cuts'] > R else 0
    return out


def fragment_cuts(node_mask, one_hot, bonds, n_bonds_in, R, charge=None, status_in=None, carbon_type=CARBON, **rule):
    """A batch: ``node_mask [B,N]``, ``one_hot [B,N,nf]``, ``bonds [B,capacity,3]``, ``n_bonds_in [B]`` (array-likes).
    Returns a dict of numpy arrays shaped and typed as the kernel's outputs."""
    node_mask = np.asarray(node_mask)
    B, N = node_mask.shape[:2]
    one_hot = np.asarray(one_hot).reshape(B, N, -1)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(B, -1, 3)
    each = [molecule(node_mask[b].reshape(N).tolist(), one_hot[b].tolist(), bonds[b].tolist(), int(n_bonds_in[b]), R,
                     None if charge is None else np.asarray(charge)[b].reshape(N).tolist(),
                     0 if status_in is None else int(status_in[b]), carbon_type, **rule) for b in range(B)]
    shape = {'bond_side': (B, bonds.shape[1]), 'cuts': (B, R, CUT_FIELDS), 'labels': (B, R, N)}
    return {name: np.array([m[name] for m in each], dtype=np.uint8 if name == 'labels' else np.int32)
            .reshape(shape.get(name, (B,))) for name in FIELDS}


# ---- molecules whose answer is known by hand: types, bonds (i, j, order), charges --------------------------------------------
def chain(n, start=0, order=1):
    return [(start + k, start + k + 1, order) for k in range(n - 1)]


def ring(n, start=0, order=1):
    return [(start + k, start + (k + 1) % n, order) for k in range(n)]


def tail(root, first, length):
    """A chain of ``length`` new atoms ``first..`` hanging on ``root``."""
    return [(root, first, 1)] + chain(length, first)


HAND = {
    'chain12': ([C] * 12, chain(12), {}),
    'chain13': ([C] * 13, chain(13), {}),
    'chain14': ([C] * 14, chain(14), {}),
    # C5 - C(=O) - N - C5: atoms 0-4, carbonyl C 5, O 6, N 7, 8-12
    'amide': ([C] * 6 + [O, N_] + [C] * 5, chain(6) + [(5, 6, 2), (5, 7, 1), (7, 8, 1)] + chain(5, 8), {}),
    # C5 - C(=O) - O - C5
    'ester': ([C] * 6 + [O, O] + [C] * 5, chain(6) + [(5, 6, 2), (5, 7, 1), (7, 8, 1)] + chain(5, 8), {}),
    # C5 - N - O - C5: the N-O bond 5-6
    'n_o': ([C] * 5 + [N_, O] + [C] * 5, chain(12), {}),
    # atoms 5 and 6 are carbons with a charge: the bond between them has no end that qualifies
    'charged': ([C] * 12, chain(12), {5: 1, 6: -1}),
    # the bonds 5-6 (double), 6-7 (triple), 7-8 (aromatic) of a chain are never cut
    'orders': ([C] * 14, chain(5) + [(4, 5, 1), (5, 6, 2), (6, 7, 3), (7, 8, 4), (8, 9, 1)] + chain(5, 9), {}),
    # two six-rings 0-5 and 6-11 joined by 5-6, with tails of five atoms on atoms 2 (12-16) and 9 (17-21)
    'biphenyl_tails': ([C] * 22, ring(6) + [(5, 6, 1)] + ring(6, 6) + tail(2, 12, 5) + tail(9, 17, 5), {}),
    # a linker that holds a five-ring 5-9 with a branch atom 10 on it: fragment 0-4 on atom 5, fragment 11-15 on atom 7
    'ring_linker': ([C] * 16, chain(5) + [(4, 5, 1)] + ring(5, 5) + [(9, 10, 1), (7, 11, 1)] + chain(5, 11), {}),
    # a core atom 0 with three arms of five atoms
    'star': ([C] * 16, tail(0, 1, 5) + tail(0, 6, 5) + tail(0, 11, 5), {}),
}


def hand_molecule(name, nf=3):
    """``(mask, one_hot, entries, n_bonds_in, charge)`` of a hand molecule: every row real, the list exactly full."""
    types, entries, charged = HAND[name]
    one_hot = [[1.0 if t == k else 0.0 for k in range(nf)] for t in types]
    return [1.0] * len(types), one_hot, entries, len(entries), [charged.get(k, 0) for k in range(len(types))]


def hand(name, R=64, **rule):
    mask, one_hot, entries, n_in, charge = hand_molecule(name)
    return molecule(mask, one_hot, entries, n_in, R, charge, **rule)
