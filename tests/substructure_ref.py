"""The rule of ``dl_substructure_match`` (``include/difflinker_hip.h``) restated in plain Python from the compiled tables of
``difflinker_amd.patterns``: the graph and the atom properties, the three-level predicates, the depth-first search in the
order the pattern is written, the step count and its budget, ``first_root`` and the marked variant.  One molecule at a time,
nothing shared with the kernel's text; ``tests/test_gpu_substructure.py`` holds the kernel against it bit for bit."""
from collections import deque

from difflinker_amd import patterns as P

TOO_LARGE, BAD_BOND, BUDGET, OVERFLOW = 4, 8, 512, 1
MAX_ATOMS, MAX_BONDS = 256, 2048


class Molecule:
    """The kept graph: ``z`` and ``dv`` by atom number, ``entries`` the bond list ``(i, j, order)``, ``flags`` one aromatic flag
    per entry (or None), ``keep`` and ``marked`` by atom number (or None: all kept, none marked)."""

    def __init__(self, z, dv, entries, flags=None, keep=None, marked=None):
        n_real = len(z)
        keep = [True] * n_real if keep is None else keep
        self.atoms = [k for k in range(n_real) if keep[k]]                 # kept index -> atom number
        index = {k: i for i, k in enumerate(self.atoms)}
        self.n = len(self.atoms)
        self.status, self.too_large = 0, self.n > MAX_ATOMS
        if self.too_large:
            return
        valid, bad = [], False
        for e, (i, j, o) in enumerate(entries):
            if not (0 <= i < n_real and 0 <= j < n_real and i != j and 1 <= o <= 3):
                bad = True
            elif i in index and j in index:
                valid.append((e, index[i], index[j], o))
        if len(valid) > MAX_BONDS:
            self.too_large, self.status = True, BAD_BOND if bad else 0
            return
        self.pair = {}                                                     # (lo, hi) -> [order, aromatic, ring size or 0]
        for e, u, v, o in valid:
            key = (min(u, v), max(u, v))
            if key in self.pair:
                bad = True                                                 # the first entry stands
            else:
                self.pair[key] = [o, bool(flags is not None and flags[e]), 0]
        self.status = BAD_BOND if bad else 0
        self.nbrs = [[] for _ in range(self.n)]
        for u, v in self.pair:
            self.nbrs[u].append(v)
            self.nbrs[v].append(u)
        for row in self.nbrs:
            row.sort()
        for (u, v), record in self.pair.items():
            record[2] = self.ring_size(u, v)
        sat = lambda value: min(value, 255)
        clamp = lambda value: min(max(value, 0), 255)
        self.z = [clamp(z[k]) for k in self.atoms]
        self.marked = [bool(marked is not None and marked[k]) for k in self.atoms]
        self.d, self.h, self.x, self.v, self.arom, self.xr, self.rs = [], [], [], [], [], [], []
        for u in range(self.n):
            bonds = [self.bond(u, v) for v in self.nbrs[u]]
            order_sum = sum(b[0] for b in bonds)
            h = max(0, clamp(dv[self.atoms[u]]) - order_sum)
            rings = [b[2] for b in bonds if b[2]]
            self.d.append(sat(len(bonds)))
            self.h.append(sat(h))
            self.x.append(sat(len(bonds) + h))
            self.v.append(sat(order_sum + h))
            self.arom.append(any(b[1] for b in bonds))
            self.xr.append(sat(len(rings)))
            self.rs.append(sat(min(rings)) if rings else 0)
        self.hist = {}
        for value in self.z:
            self.hist[value] = self.hist.get(value, 0) + 1

    def bond(self, u, v):
        return self.pair.get((min(u, v), max(u, v)))

    def state(self, u, v):
        order, aromatic, ring = self.bond(u, v)
        return P.bond_state(order, aromatic, ring > 0)

    def ring_size(self, u, v):
        """The shortest path from u to v that does not use the bond itself, in atoms (0: a bridge)."""
        dist, queue = {u: 0}, deque([u])
        while queue:
            a = queue.popleft()
            for w in self.nbrs[a]:
                if (a == u and w == v) or w in dist:
                    continue
                dist[w] = dist[a] + 1
                if w == v:
                    return dist[w] + 1
                queue.append(w)
        return 0


class _Stop(Exception):
    pass


class Matcher:
    def __init__(self, patterns):
        self.pat = patterns.pat.tolist()
        self.atoms = patterns.atoms.tolist()
        self.closures = patterns.closures.tolist()
        self.preds = patterns.preds.tolist()
        self.n_sub, self.n_top, self.level_end = patterns.n_sub, patterns.n_top, list(patterns.level_end)

    def atom_ok(self, mol, sub_bits, record, v):
        result, alternative, conjunction = True, False, True
        for tok in self.preds[record[2]:record[2] + record[3]]:
            op, arg = tok & 0xFF, tok >> 8 & 0xFFFF
            value = {P.P_TRUE: lambda: True, P.P_ELEM: lambda: mol.z[v] == arg,
                     P.P_ELEM_ALIPH: lambda: mol.z[v] == arg and not mol.arom[v],
                     P.P_ELEM_AROM: lambda: mol.z[v] == arg and mol.arom[v], P.P_AROM: lambda: mol.arom[v],
                     P.P_D: lambda: mol.d[v] == arg, P.P_H: lambda: mol.h[v] == arg, P.P_HMIN: lambda: mol.h[v] >= arg,
                     P.P_X: lambda: mol.x[v] == arg, P.P_V: lambda: mol.v[v] == arg, P.P_RING: lambda: mol.xr[v] > 0,
                     P.P_RSIZE: lambda: mol.rs[v] == arg, P.P_XRING: lambda: mol.xr[v] == arg,
                     P.P_REC: lambda: v in sub_bits[arg]}.get(op, lambda: False)()
            conjunction = conjunction and (not value if tok & P.NEG else bool(value))
            if tok & P.END_AND:
                alternative, conjunction = alternative or conjunction, True
            if tok & P.END_OR:
                result, alternative = result and alternative, False
        return result

    def searchable(self, mol, q):
        off, m, _, *screen = self.pat[q][:7]
        if not 1 <= m <= P.MAX_PATTERN_ATOMS or m > mol.n:
            return False
        return all(w == 0 or mol.hist.get(w & 0xFF, 0) >= w >> 8 for w in screen)

    def search(self, mol, sub_bits, q, root, to_mark, max_steps):
        """``(any, marked, budget, steps)`` of pattern ``q`` from the kept atom ``root``."""
        off, m = self.pat[q][:2]
        records = self.atoms[off:off + m]
        found = dict(any=False, marked=False, budget=False, steps=0)

        def step():
            if found['steps'] >= max_steps:
                found['budget'] = True
                raise _Stop
            found['steps'] += 1

        def extend(k, image):
            if k == m:
                found['any'] = True
                if not to_mark:
                    raise _Stop
                if any(mol.marked[v] for v in image):
                    found['marked'] = True
                    raise _Stop
                return
            parent, mask, _, _, c_off, c_len = records[k]
            at = image[parent]
            for v in mol.nbrs[at]:
                step()
                if v in image or not mask >> mol.state(at, v) & 1 or not self.atom_ok(mol, sub_bits, records[k], v):
                    continue
                if all(mol.bond(v, image[j]) is not None and cmask >> mol.state(v, image[j]) & 1
                       for j, cmask in self.closures[c_off:c_off + c_len]):
                    extend(k + 1, image + [v])
        try:
            step()
            if self.atom_ok(mol, sub_bits, records[0], root):
                extend(1, [root])
        except _Stop:
            pass
        return found['any'], found['marked'], found['budget'], found['steps']

    def match(self, mol, rows=None, max_steps=4096, status_in=0, with_marks=False):
        """The kernel's outputs for one molecule as a dict, plus ``steps`` (per top-level pattern and root that was searched)
        ``screened`` (the top-level patterns not searched at all) and ``roots`` / ``roots_marked`` (per pattern the atom numbers
        that root a match).  ``rows``: the original row of every atom number."""
        out = dict(first_root=[-1] * self.n_top, first_root_marked=[-1] * self.n_top, n_hits=0, n_hits_marked=0,
                   status=status_in | mol.status, steps={}, screened=0,
                   roots=[set() for _ in range(self.n_top)], roots_marked=[set() for _ in range(self.n_top)])
        if mol.too_large:
            out['status'] |= TOO_LARGE
            return out
        budget = False
        sub_bits = [set() for _ in range(self.n_sub)]
        lo = 0
        for hi in self.level_end:
            new = [set() for _ in range(self.n_sub)]
            for s in range(lo, hi):
                if not self.searchable(mol, s):
                    continue
                for root in range(mol.n):
                    hit, _, over, _ = self.search(mol, sub_bits, s, root, False, max_steps)
                    budget |= over
                    if hit:
                        new[s].add(root)
            for s in range(lo, hi):
                sub_bits[s] = new[s]
            lo = hi
        for p in range(self.n_top):
            q = self.n_sub + p
            if not self.searchable(mol, q):
                out['screened'] += 1
                continue
            for root in range(mol.n):
                hit, marked, over, steps = self.search(mol, sub_bits, q, root, with_marks, max_steps)
                out['steps'][p, root] = steps
                budget |= over
                row = mol.atoms[root] if rows is None else rows[mol.atoms[root]]
                if hit:
                    out['roots'][p].add(mol.atoms[root])
                if marked:
                    out['roots_marked'][p].add(mol.atoms[root])
                if hit and out['first_root'][p] < 0:
                    out['first_root'][p] = row
                if marked and out['first_root_marked'][p] < 0:
                    out['first_root_marked'][p] = row
        out['n_hits'] = sum(1 for r in out['first_root'] if r >= 0)
        out['n_hits_marked'] = sum(1 for r in out['first_root_marked'] if r >= 0)
        out['status'] |= BUDGET if budget else 0
        return out
