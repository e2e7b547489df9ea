"""The ring rule of ``dl_ring_scores`` (``include/difflinker_hip.h``, ``csrc/rings.hip``) restated in plain Python: a
breadth-first search per bond, pieces by flood fill, the histograms and the status bits.  The kernel must agree exactly.

Atom ``k`` is the k-th row with ``node_mask != 0``; ``drop_mask`` removes atoms after that numbering; an entry
``(i, j, order)`` is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 3``, in either orientation."""
from collections import deque

import numpy as np

MAX_ATOMS, BINS = 256, 7
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND = 1, 4, 8
FIELDS = ('n_atoms', 'n_bonds', 'n_components', 'n_rings', 'bond_ring', 'atom_ring', 'ring_hist', 'status')
PER_MOLECULE = ('n_atoms', 'n_bonds', 'n_components', 'n_rings', 'atom_ring', 'ring_hist', 'status')


def ring_bin(ring):
    return 0 if ring == 0 else (ring - 2 if ring <= 7 else BINS - 1)


def smallest_ring(adj, u, v):
    """Atoms of the smallest cycle through the bond ``(u, v)`` of the adjacency sets ``adj``; 0 for a bridge."""
    dist = {u: 0}
    queue = deque([u])
    while queue:
        w = queue.popleft()
        for t in adj[w]:
            if w == u and t == v:                # the bond itself; it leaves u, so it can be walked nowhere else
                continue
            if t not in dist:
                dist[t] = dist[w] + 1
                if t == v:
                    return dist[t] + 1
                queue.append(t)
    return 0


def components(adj, atoms):
    seen, pieces = set(), 0
    for root in atoms:
        if root in seen:
            continue
        pieces += 1
        seen.add(root)
        queue = deque([root])
        while queue:
            w = queue.popleft()
            for t in adj[w]:
                if t not in seen:
                    seen.add(t)
                    queue.append(t)
    return pieces


def molecule(mask, entries, n_bonds_in, status_in=0, drop=None, mark=None):
    """One molecule: ``mask`` / ``drop`` / ``mark`` rows of ``N`` numbers, ``entries`` the whole list ``[capacity][3]``.
    Returns a dict of ``FIELDS``: ints, ``bond_ring [capacity]``, ``atom_ring [N]``, ``ring_hist [2][BINS]``."""
    N, capacity = len(mask), len(entries)
    rows = [r for r in range(N) if mask[r] != 0]
    n = len(rows)
    kept = [drop is None or drop[r] == 0 for r in rows]
    marked = [mark is not None and mark[r] != 0 for r in rows]
    status = int(status_in) | (BONDS_OVERFLOW if n_bonds_in > capacity else 0)
    out = {'n_atoms': sum(kept), 'n_bonds': 0, 'n_components': 0, 'n_rings': 0, 'bond_ring': [0] * capacity,
           'atom_ring': [0] * N, 'ring_hist': [[0] * BINS, [0] * BINS], 'status': status}
    if out['n_atoms'] > MAX_ATOMS:
        out['status'] |= TOO_LARGE
        return out
    nb = min(max(int(n_bonds_in), 0), capacity)
    adj = {k: set() for k in range(n) if kept[k]}
    bonds, pairs, bad = {}, set(), False
    for e in range(nb):
        i, j, order = (int(v) for v in entries[e])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 3):
            bad = True
            continue
        if not (kept[i] and kept[j]):
            continue
        bonds[e] = (i, j)
        pair = (min(i, j), max(i, j))
        bad = bad or pair in pairs
        pairs.add(pair)
        adj[i].add(j)
        adj[j].add(i)
    for e, (i, j) in bonds.items():
        ring = smallest_ring(adj, i, j)
        out['bond_ring'][e] = ring
        out['ring_hist'][0][ring_bin(ring)] += 1
        if marked[i] or marked[j]:
            out['ring_hist'][1][ring_bin(ring)] += 1
        for k in (i, j):
            if ring and (out['atom_ring'][k] == 0 or ring < out['atom_ring'][k]):
                out['atom_ring'][k] = ring
    out['n_bonds'] = len(pairs)
    out['n_components'] = components(adj, sorted(adj))
    out['n_rings'] = out['n_bonds'] - out['n_atoms'] + out['n_components']
    out['status'] |= BAD_BOND if bad else 0
    return out


def ring_scores(node_mask, bonds, n_bonds_in, status_in=None, drop_mask=None, mark_mask=None):
    """A batch: ``node_mask [B,N]``, ``bonds [B,capacity,3]``, ``n_bonds_in [B]`` (array-likes).  Returns a dict of int32
    numpy arrays shaped as the kernel's outputs."""
    node_mask = np.asarray(node_mask).reshape(len(node_mask), -1)
    B, N = node_mask.shape
    bonds = np.asarray(bonds, dtype=np.int64)
    bonds = bonds.reshape(B, bonds.size // (3 * B) if B else 0, 3)
    row = lambda m, b: None if m is None else np.asarray(m).reshape(B, N)[b].tolist()      # noqa: E731
    each = [molecule(node_mask[b].tolist(), bonds[b].tolist(), int(n_bonds_in[b]), 0 if status_in is None else int(status_in[b]),
                     row(drop_mask, b), row(mark_mask, b)) for b in range(B)]
    shape = {'bond_ring': (B, bonds.shape[1]), 'atom_ring': (B, N), 'ring_hist': (B, 2, BINS)}
    return {name: np.array([m[name] for m in each], dtype=np.int32).reshape(shape.get(name, (B,))) for name in FIELDS}


# ---- molecules whose answer is known by hand: (atoms, bonds as (i, j) pairs) ------------------------------------------------
def ring(n, start=0):
    return [(start + k, start + (k + 1) % n) for k in range(n)]


HAND = {
    # a branched tree
    'tree': (7, [(0, 1), (1, 2), (1, 3), (3, 4), (3, 5), (5, 6)]),
    # benzene 0-5, bond 5-6 to cyclopropane 6-8
    'cyclopropylbenzene': (9, ring(6) + [(5, 6)] + ring(3, 6)),
    # two fused six-rings sharing bond 0-5
    'naphthalene': (10, ring(6) + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 0)]),
    # bicyclo[2.2.1]heptane: bridgeheads 0 and 3, bridges 1-2, 4-5 and 6
    'norbornane': (7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 6), (6, 3)]),
    # two five-rings sharing atom 0
    'spiro[4.4]nonane': (9, ring(5) + [(0, 5), (5, 6), (6, 7), (7, 8), (8, 0)]),
    'cubane': (8, ring(4) + ring(4, 4) + [(k, k + 4) for k in range(4)]),
    # a 12-ring with one more atom on it
    'macrocycle_tail': (13, ring(12) + [(0, 12)]),
}
HAND_ANSWERS = {                                 # name: (sorted bond_ring values, n_rings)
    'tree': ([0] * 6, 0),
    'cyclopropylbenzene': ([0] + [3] * 3 + [6] * 6, 2),
    'naphthalene': ([6] * 11, 2),
    'norbornane': ([5] * 8, 2),
    'spiro[4.4]nonane': ([5] * 10, 2),
    'cubane': ([4] * 12, 5),
    'macrocycle_tail': ([0] + [12] * 12, 1),
}


def hand_molecule(name, order=1):
    """``(mask, entries, n_bonds_in)`` of a hand molecule for ``molecule``: every row real, the list exactly full."""
    atoms, pairs = HAND[name]
    return [1.0] * atoms, [(i, j, order) for i, j in pairs], len(pairs)
