"""The multi-cut rule of ``dl_fragment_multicuts`` (``include/difflinker_hip.h``, ``csrc/fragment.hip``) restated in plain
Python, by another route than the kernel's: every set of ``k`` cuttable bonds is REMOVED, the pieces that remain are labelled,
and the set is a star when one piece touches all ``k`` bonds.  The kernel must agree exactly: integers, order of records,
labels, status.  No run of the reference pins the rule (RDKit is not needed here): the header is the authority.

Atoms, bonds, cuttable bonds, "one piece" and the status bits they set are those of ``fragment_ref.molecule``, which is asked
for them; what is new is the gates, the 64-bond limit and the stars.

The pieces are labelled on the graph whose nodes are the pieces left when ALL cuttable bonds are removed (a tree of at most
``n_cuttable + 1`` nodes, its edges the cuttable bonds): removing ``k`` of them there and joining the rest is the same thing
as removing them from the molecule, at a cost that lets a test look at every set of a 30-atom molecule."""
from itertools import combinations

import numpy as np

import fragment_ref

FIELDS_PER_CUT, MIN_CUTS, MAX_CUTS, MAX_CUTTABLE, LINKER = 22, 3, 5, 64, 5
MANY_CUTTABLE = 64
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND, DISCONNECTED, TRUNCATED = (fragment_ref.BONDS_OVERFLOW, fragment_ref.TOO_LARGE,
                                                                fragment_ref.BAD_BOND, fragment_ref.DISCONNECTED,
                                                                fragment_ref.TRUNCATED)
FIELDS = ('n_atoms', 'n_bonds', 'n_cuttable', 'n_cuts', 'status', 'n_cuts_k', 'cuts', 'labels')
DEFAULTS = {'min_cuts': 3, 'max_cuts': 5, 'min_linker': 3, 'min_fragment': 3, 'max_atoms': 40, 'min_rings': 3}
GATES_OFF = {'max_atoms': 256, 'min_rings': 0}
NEVER = 1 << 30                                  # a linker size no pair of fragment_ref reaches: its double loop keeps nothing


def find(parent, v):
    while parent[v] != v:
        parent[v] = parent[parent[v]]
        v = parent[v]
    return v


def molecule(mask, one_hot, entries, n_bonds_in, R, charge=None, status_in=0, carbon_type=fragment_ref.CARBON, **rule):
    """One molecule, the arguments of ``fragment_ref.molecule``.  Returns a dict of ``FIELDS``: ints, ``n_cuts_k [3]``,
    ``cuts [R][22]``, ``labels [R][N]``."""
    rule = dict(DEFAULTS, **rule)
    assert MIN_CUTS <= rule['min_cuts'] <= rule['max_cuts'] <= MAX_CUTS
    N = len(mask)
    front = fragment_ref.molecule(mask, one_hot, entries, n_bonds_in, 0, charge, status_in, carbon_type, min_linker=NEVER)
    n = front['n_atoms']
    out = {'n_atoms': n, 'n_bonds': front['n_bonds'], 'n_cuttable': front['n_cuttable'], 'n_cuts': 0, 'status': front['status'],
           'n_cuts_k': [0, 0, 0], 'cuts': [[0] * FIELDS_PER_CUT for _ in range(R)], 'labels': [[255] * N for _ in range(R)]}
    if out['status'] & TOO_LARGE:
        return out
    if n > rule['max_atoms'] or out['n_bonds'] - n + 1 < rule['min_rings']:
        return out                               # a gate: no cuts, no bit
    if out['n_cuttable'] > MAX_CUTTABLE:
        out['status'] |= MANY_CUTTABLE
        return out
    if out['status'] & DISCONNECTED or n == 0:
        return out

    cuttable = [(e,) + tuple(int(v) for v in entries[e][:2]) for e, side in enumerate(front['bond_side']) if side]
    where = {(min(i, j), max(i, j)) for _, i, j in cuttable}
    # the bonds of the molecule once more: the first entry of every pair that is a bond
    seen, parent = set(), list(range(n))
    for e in range(min(max(int(n_bonds_in), 0), len(entries))):
        i, j, order = (int(v) for v in entries[e])
        pair = (min(i, j), max(i, j))
        if 0 <= i < n and 0 <= j < n and i != j and 1 <= order <= 4 and pair not in seen:
            seen.add(pair)
            if pair not in where:
                parent[find(parent, i)] = find(parent, j)
    block = [find(parent, v) for v in range(n)]               # the piece of every atom with ALL cuttable bonds removed
    names = sorted(set(block))
    block = [names.index(v) for v in block]
    members = [[v for v in range(n) if block[v] == k] for k in range(len(names))]
    ends = [(block[i], block[j]) for _, i, j in cuttable]

    for k in range(rule['min_cuts'], rule['max_cuts'] + 1):
        for chosen in combinations(range(len(cuttable)), k):
            gone = set(chosen)
            piece = list(range(len(names)))
            for c, (u, v) in enumerate(ends):
                if c not in gone:
                    piece[find(piece, u)] = find(piece, v)
            touching = None                      # the pieces that touch every removed bond
            for c in chosen:
                both = {find(piece, ends[c][0]), find(piece, ends[c][1])}
                touching = both if touching is None else touching & both
            if not touching:
                continue
            centre, = touching
            label = [None] * n
            anchors, exits, sizes = [], [], []
            for q, c in enumerate(chosen):
                _, i, j = cuttable[c]
                anchor, leave = (j, i) if find(piece, block[i]) == centre else (i, j)
                beyond = find(piece, block[anchor])
                atoms = [v for b in range(len(names)) if find(piece, b) == beyond for v in members[b]]
                for v in atoms:
                    label[v] = q
                anchors.append(anchor)
                exits.append(leave)
                sizes.append(len(atoms))
            n_linker = n - sum(sizes)
            if n_linker < rule['min_linker'] or min(sizes) < rule['min_fragment']:
                continue
            r = out['n_cuts']
            out['n_cuts'] += 1
            out['n_cuts_k'][k - MIN_CUTS] += 1
            if r < R:
                pad = [-1] * (MAX_CUTS - k)
                out['cuts'][r] = [k, n_linker] + [cuttable[c][0] for c in chosen] + pad + anchors + pad + exits + pad + sizes + pad
                out['labels'][r] = [(LINKER if label[v] is None else label[v]) if v < n else 255 for v in range(N)]
    out['status'] |= TRUNCATED if out['n_cuts'] > R else 0
    return out


def multicuts(node_mask, one_hot, bonds, n_bonds_in, R, charge=None, status_in=None, carbon_type=fragment_ref.CARBON, **rule):
    """A batch, as ``fragment_ref.fragment_cuts``.  Returns a dict of numpy arrays shaped and typed as the kernel's outputs."""
    node_mask = np.asarray(node_mask)
    B, N = node_mask.shape[:2]
    one_hot = np.asarray(one_hot).reshape(B, N, -1)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(B, -1, 3)
    each = [molecule(node_mask[b].reshape(N).tolist(), one_hot[b].tolist(), bonds[b].tolist(), int(n_bonds_in[b]), R,
                     None if charge is None else np.asarray(charge)[b].reshape(N).tolist(),
                     0 if status_in is None else int(status_in[b]), carbon_type, **rule) for b in range(B)]
    shape = {'n_cuts_k': (B, 3), 'cuts': (B, R, FIELDS_PER_CUT), 'labels': (B, R, N)}
    return {name: np.array([m[name] for m in each], dtype=np.uint8 if name == 'labels' else np.int32)
            .reshape(shape.get(name, (B,))) for name in FIELDS}


def arms(m, length=1):
    """A centre atom 0 with ``m`` arms of ``length`` carbons: ``(types, entries)``."""
    entries = []
    for a in range(m):
        entries += fragment_ref.tail(0, 1 + a * length, length)
    return [fragment_ref.C] * (1 + m * length), entries


def hand(name, R=64, **rule):
    mask, one_hot, entries, n_in, charge = fragment_ref.hand_molecule(name)
    return molecule(mask, one_hot, entries, n_in, R, charge, **dict(GATES_OFF, **rule))


def of_types(types, entries, R, nf=3, **rule):
    one_hot = [[1.0 if t == k else 0.0 for k in range(nf)] for t in types]
    return molecule([1.0] * len(types), one_hot, entries, len(entries), R, **rule)
