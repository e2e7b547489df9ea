"""Plain restatement of ``csrc/canon.hip`` (canonical ranks and code by an individualisation-refinement search), used by
tests only.  The rule is the one written in ``include/difflinker_hip.h``; the mixing functions are those of
``mol_keys_ref.py``.  The rounds of a refinement run on numpy ``uint64`` arrays (which wrap modulo 2^64), everything that
steers the search is plain Python.  It shares nothing with the kernel or with ``difflinker_amd``.
"""
import numpy as np

from mol_keys_ref import M, SEED_COLOUR, SEED_KEY, mix2

MAX_ATOMS, MAX_BONDS, MAX_DEPTH, MAX_LEAVES = 256, 2048, 32, 65536
TOO_LARGE, BAD_BOND, BUDGET = 4, 8, 256
_U = np.uint64


def _mix64(z):
    z = z + _U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def _mix2(a, b):
    return _mix64(a + b * _U(0xD6E8FEB86659FD93))


class _Graph:
    """The kept graph: ``types`` by kept index, ``ends``/``other``/``order`` one row per END of a kept list entry."""

    def __init__(self, types, bonds):
        self.n = len(types)
        self.types = list(types)
        self.bonds = list(bonds)
        ends = [i for i, j, o in bonds] + [j for i, j, o in bonds]
        self.ends = np.array(ends, dtype=np.int64)
        self.other = np.array([j for i, j, o in bonds] + [i for i, j, o in bonds], dtype=np.int64)
        self.order = np.array([o for i, j, o in bonds] * 2, dtype=_U)
        self.row = [[] for _ in types]                       # per atom: (neighbour, order) of its entries
        for i, j, o in bonds:
            self.row[i].append((j, o))
            self.row[j].append((i, o))

    def refine_and_rank(self, start):
        c = np.array(start, dtype=_U)
        with np.errstate(over='ignore'):
            for _ in range(self.n):
                s = np.zeros(self.n, dtype=_U)
                if len(self.ends):
                    np.add.at(s, self.ends, _mix2(c[self.other], self.order))
                c = _mix2(c, s)
        c = [int(v) for v in c]
        return [sum(1 for w in c if w < v) for v in c]

    def root(self):
        return self.refine_and_rank([mix2(SEED_COLOUR, t + 1) for t in self.types])

    def child(self, rank, v):
        return self.refine_and_rank([mix2(SEED_COLOUR, 2 * rank[i] + (0 if i == v else 1)) for i in range(self.n)])

    def leaf_code(self, rank):
        a = sum(mix2(rank[i], self.types[i] + 1) for i in range(self.n)) & M
        b = sum(mix2(mix2(min(rank[i], rank[j]), max(rank[i], rank[j])), o) for i, j, o in self.bonds) & M
        return mix2(mix2(SEED_KEY, a), b)


def _tied_cell(rank):
    """(rank, members ascending) of the tied cell with the smallest rank, or None."""
    count = {}
    for r in rank:
        count[r] = count.get(r, 0) + 1
    tied = [r for r, c in count.items() if c > 1]
    if not tied:
        return None
    cell = min(tied)
    return cell, [i for i, r in enumerate(rank) if r == cell]


def search(types, bonds, max_leaves=256, max_depth=MAX_DEPTH, branch=True):
    """The search over a graph given by kept index.  Returns ``(rank, code, n_leaves, budget)``.  ``branch=False`` is the
    variant that always takes the lowest member (for the test that shows branching matters); it is not the rule."""
    g = _Graph(types, bonds)
    rank = g.root()
    stack = []                                               # per branching level: (saved ranks, cell members, position)
    leaves, budget, best, best_rank = 0, False, None, None
    while True:
        for step in range(g.n + 1):                          # descend to a leaf
            found = _tied_cell(rank)
            if found is None:
                break
            if step == g.n:                                  # only after a collision of two 64-bit colours: see the header
                budget = True
                break
            cell, members = found
            v = members[0]
            rows = [g.row[m] for m in members]
            twin = all(len(r) == 1 for r in rows) and len({r[0] for r in rows}) == 1
            if not twin and branch:
                if len(stack) >= max_depth:
                    budget = True
                else:
                    stack.append([rank, members, 0])
            rank = g.child(rank, v)
        leaves += 1
        code = g.leaf_code(rank)
        if best is None or code < best:
            best, best_rank = code, rank
        while stack and stack[-1][2] + 1 >= len(stack[-1][1]):
            stack.pop()
        if not stack:
            break
        if leaves >= max_leaves:
            budget = True
            break
        top = stack[-1]
        top[2] += 1
        rank = g.child(top[0], top[1][top[2]])
    return best_rank, best, leaves, budget


def canonical_ranks(types, entries, keep=None, max_leaves=256, status_in=0):
    """What ``dl_canonical_ranks`` answers for one molecule: ``types`` per atom, ``entries`` the bond list as given (any
    triples), ``keep`` per atom (False = dropped).  Returns ``dict(rank, code, n_leaves, status)``, ``rank`` by atom
    number with -1 for dropped atoms."""
    n_atoms = len(types)
    keep = [True] * n_atoms if keep is None else [bool(k) for k in keep]
    new = {}
    for k in range(n_atoms):
        if keep[k]:
            new[k] = len(new)
    too_large = dict(rank=[-1] * n_atoms, code=0, n_leaves=0, status=status_in | TOO_LARGE)
    if len(new) > MAX_ATOMS:                                 # the list is not looked at
        return too_large
    no_bond, repeated, kept, seen = False, False, [], set()
    for i, j, o in entries:
        if not (0 <= i < n_atoms and 0 <= j < n_atoms and i != j and 1 <= o <= 3):
            no_bond = True
            continue
        if i in new and j in new:
            repeated |= (min(i, j), max(i, j)) in seen
            seen.add((min(i, j), max(i, j)))
            kept.append((new[i], new[j], o))
    if len(kept) > MAX_BONDS:                                # repeated pairs are not looked for
        too_large['status'] |= BAD_BOND if no_bond else 0
        return too_large
    rank, code, leaves, budget = search([types[k] for k in new], kept, max_leaves)
    return dict(rank=[rank[new[k]] if k in new else -1 for k in range(n_atoms)], code=code, n_leaves=leaves,
                status=status_in | (BAD_BOND if no_bond or repeated else 0) | (BUDGET if budget else 0))


def form(types, bonds, rank):
    """The canonical form of a molecule given by kept index: the types by rank and the sorted (rank, rank, order) triples."""
    by_rank = [None] * len(types)
    for i, r in enumerate(rank):
        by_rank[r] = types[i]
    return tuple(by_rank), tuple(sorted((min(rank[i], rank[j]), max(rank[i], rank[j]), o) for i, j, o in bonds))
