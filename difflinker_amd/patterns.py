"""The pattern compiler of the substructure search (``csrc/substructure.hip``, ``metrics.match_patterns``): a subset of
SMARTS, compiled on the host to the int32 tables the kernel reads.  The language and the matching rule are this project's own
statement (``include/difflinker_hip.h`` has both in full; ``tests/substructure_ref.py`` restates the search) - NOT RDKit's
parser or matcher: no charges, no stereo, no isotopes, no explicit hydrogens, no SSSR ring counts.

ATOMS   ``#n``; an upper-case element symbol (the element, aliphatic); ``c n o s p`` (the element, aromatic); ``*`` ``a``
        ``A``; ``D<n>`` kept heavy neighbours; ``H<n>`` / ``h<n>`` open valences ``max(0, default valence - order sum)`` (``H``
        alone is ``H1``, ``h`` alone is "at least one"); ``X<n>`` = D + H; ``v<n>`` = order sum + H; ``R`` on a ring bond,
        ``R0`` on none (``R<n>``, n >= 1, is rejected); ``r`` in a ring, ``r<n>`` the smallest ring through the atom has n
        atoms; ``x<n>`` ring bonds (``x`` alone: at least one); ``+<n>`` / ``-<n>``: every atom has charge 0; ``$(...)``.
        ``!``, ``&``, juxtaposition, ``,`` and ``;`` with SMARTS precedence: every expression is an AND (``;``) of ORs (``,``)
        of ANDs (``&``) of possibly negated primitives, and is compiled to exactly that form.  An atom is aromatic when one of
        its kept bonds is flagged aromatic.
BONDS   ``-`` ``=`` ``#`` the Kekule order of a bond that is not flagged aromatic; ``:`` a flagged bond; ``~`` any; ``@`` on a
        cycle; ``!`` ``&`` ``,`` ``;``; no written bond: ``-`` or ``:``.  A bond expression is compiled to a 12-bit mask over the
        states ``(order - 1) + 3 * aromatic + 6 * ring``.
[#1]    a pattern atom written exactly ``[#1]`` that is a leaf joined by ``-`` or no written bond is removed, and its
        neighbour gains the clause "H >= the number of such leaves"; any other hydrogen is rejected.
$(...)  every distinct body (by text) is a sub-pattern of its own whose first atom is the root; bodies nest; sub-patterns are
        ordered by nesting level, a body after everything it uses.

The search order is part of the rule: atoms in the order written (after the hydrogen merge), atom 0 the root, atom k > 0
with the atom it was written after as its parent, ring closures as checks against earlier atoms.
"""
import csv
from collections import namedtuple

import torch

# the limits of include/difflinker_hip.h (DL_SUB_*)
MAX_PATTERN_ATOMS, MAX_SUBPATTERNS, MAX_LEVELS, MAX_PRED = 48, 256, 4, 32

# predicate tokens: op | arg << 8 | NEG | END_AND | END_OR
(P_TRUE, P_ELEM, P_ELEM_ALIPH, P_ELEM_AROM, P_AROM, P_D, P_H, P_HMIN, P_X, P_V, P_RING, P_RSIZE, P_XRING, P_REC) = range(14)
NEG, END_AND, END_OR = 1 << 24, 1 << 25, 1 << 26
PAT_FIELDS, ATOM_FIELDS, SCREEN_SLOTS = 8, 6, 4       # pat: atom_off, n_atoms, level, screen[4], 0;  atoms: parent, bond mask,
#                                                       pred_off, pred_len, closure_off, closure_len;  closures: atom, mask

BOND_STATES = 12
ANY_BOND = (1 << BOND_STATES) - 1


def bond_state(order, aromatic, ring):
    return (order - 1) + 3 * int(bool(aromatic)) + 6 * int(bool(ring))


def _mask(test):
    return sum(1 << bond_state(o, a, r) for o in (1, 2, 3) for a in (0, 1) for r in (0, 1) if test(o, a, r))


BOND_PRIMITIVES = {'-': _mask(lambda o, a, r: o == 1 and not a), '=': _mask(lambda o, a, r: o == 2 and not a),
                   '#': _mask(lambda o, a, r: o == 3 and not a), ':': _mask(lambda o, a, r: a), '~': ANY_BOND,
                   '@': _mask(lambda o, a, r: r)}
DEFAULT_BOND = BOND_PRIMITIVES['-'] | BOND_PRIMITIVES[':']

SYMBOLS = ('H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc '
           'Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi '
           'Po At Rn').split()
ATOMIC_NUMBER = {s: z + 1 for z, s in enumerate(SYMBOLS)}
AROMATIC_SYMBOLS = {'c': 6, 'n': 7, 'o': 8, 's': 16, 'p': 15}
ORGANIC = ('Cl', 'Br', 'B', 'C', 'N', 'O', 'P', 'S', 'F', 'I')       # written without brackets; two letters first

Patterns = namedtuple('Patterns', 'pat atoms closures preds n_sub n_top level_end names sub_texts sub_levels')


class PatternError(ValueError):
    """A row that does not compile: ``row`` (its number in the input, from 0), ``column`` (the offset into its SMARTS) and
    ``construct`` (the name of what is not supported)."""

    def __init__(self, row, column, construct):
        super().__init__(f'row {row}, column {column}: {construct}')
        self.row, self.column, self.construct = row, column, construct


class _Fail(Exception):
    def __init__(self, column, construct):
        self.column, self.construct = column, construct


def token(op, arg=0, neg=False):
    return op | arg << 8 | (NEG if neg else 0)


class _Atom:
    def __init__(self, expr, parent, bond, hydrogen, column):
        self.expr, self.parent, self.bond, self.hydrogen, self.column = expr, parent, bond, hydrogen, column
        self.closures = []                         # (earlier atom, mask)
        self.degree = 0
        self.ring_closed, self.exactly_h, self.bond_text = False, False, ''


class _Parser:
    """One SMARTS string (a row, or the body of a ``$(...)``) to atoms with three-level expressions.  ``subs`` maps body text to
    its index in order of first appearance and is shared by a whole catalogue; ``offset`` is where the text starts in its row."""

    def __init__(self, text, offset, subs):
        self.s, self.at, self.offset, self.subs = text, 0, offset, subs
        self.used = set()

    def fail(self, construct, at=None):
        raise _Fail(self.offset + (self.at if at is None else at), construct)

    def peek(self):
        return self.s[self.at] if self.at < len(self.s) else ''

    def number(self):
        start = self.at
        while self.peek().isdigit():
            self.at += 1
        return int(self.s[start:self.at]) if self.at > start else None

    # ---- atoms
    def primitive(self, neg):
        s, c = self.s, self.peek()
        start = self.at
        if c == '$':
            if s[self.at:self.at + 2] != '$(':
                self.fail('$ without (')
            depth, end = 0, self.at + 1
            while end < len(s):
                depth += (s[end] == '(') - (s[end] == ')')
                if depth == 0:
                    break
                end += 1
            if end >= len(s):
                self.fail('unclosed $(')
            body = s[self.at + 2:end]
            if body not in self.subs:
                self.subs[body] = (len(self.subs), self.offset + self.at + 2)
            self.used.add(body)
            self.at = end + 1
            return ('rec', body, neg)
        if c.isdigit():
            self.fail('isotope')
        if c == '@':
            self.fail('stereo')
        if c == '^':
            self.fail('^n hybridisation')
        if c == ':':
            self.fail('atom map')
        self.at += 1
        if c == '#':
            z = self.number()
            if z is None or not 1 <= z <= 255:
                self.fail('#n without a number', start)
            return token(P_ELEM, z, neg)
        if c == '*':
            return token(P_TRUE, 0, neg)
        if c == 'a':
            return token(P_AROM, 0, neg)
        if c == 'A':
            if self.peek() in ('l', 'r', 's', 'u', 'g', 't'):            # Al Ar As Au Ag At
                self.at += 1
                return token(P_ELEM_ALIPH, ATOMIC_NUMBER['A' + s[self.at - 1]], neg)
            return token(P_AROM, 0, not neg)
        if c in 'DHhXvRrx':
            n = self.number()
            if n is not None and n > 255:                                # the properties saturate at 255, and a token holds 16 bits
                self.fail('count above 255', start)
            if c == 'D':
                return token(P_D, 1 if n is None else n, neg)
            if c == 'H':
                return token(P_H, 1 if n is None else n, neg)
            if c == 'h':
                return token(P_HMIN, 1, neg) if n is None else token(P_H, n, neg)
            if c == 'X':
                return token(P_X, 1 if n is None else n, neg)
            if c == 'v':
                return token(P_V, 1 if n is None else n, neg)
            if c == 'R':
                if n is not None and n >= 1:
                    self.fail('R<n> ring count', start)
                return token(P_RING, 0, neg != (n == 0))
            if c == 'r':
                return token(P_RING, 0, neg != (n == 0)) if not n else token(P_RSIZE, n, neg)
            return token(P_RING, 0, neg) if n is None else token(P_XRING, n, neg)
        if c in '+-':
            n = self.number()
            if n is None:
                n = 1
                while self.peek() == c:
                    n += 1
                    self.at += 1
            return token(P_TRUE, 0, neg != (n != 0))                       # every atom has charge 0
        if c in AROMATIC_SYMBOLS:
            return token(P_ELEM_AROM, AROMATIC_SYMBOLS[c], neg)
        if c.isupper():
            two = s[start:start + 2]
            if two in ATOMIC_NUMBER and two != 'H' and len(two) == 2 and two[1].islower():
                self.at += 1
                return token(P_ELEM_ALIPH, ATOMIC_NUMBER[two], neg)
            if c in ATOMIC_NUMBER:
                return token(P_ELEM_ALIPH, ATOMIC_NUMBER[c], neg)
        self.fail(f'atom primitive {c!r}', start)

    def expression(self):
        """The bracket's content up to ``]``: a list (;) of lists (,) of lists (&) of tokens."""
        clauses, ors, ands = [], [], []
        while True:
            neg = False
            while self.peek() == '!':
                neg = not neg
                self.at += 1
            if self.peek() in ('', ']', ',', ';', '&'):
                self.fail('empty atom expression')
            ands.append(self.primitive(neg))
            c = self.peek()
            if c == '&':
                self.at += 1
            elif c in (',', ';', ']'):
                ors.append(ands)
                ands = []
                if c != ',':
                    clauses.append(ors)
                    ors = []
                if c == ']':
                    self.at += 1
                    return clauses
                self.at += 1
            elif c == '':
                self.fail('unclosed [')

    def atom(self):
        """An atom at the cursor, or None: ``(expression, written exactly [#1])``."""
        c = self.peek()
        if c == '[':
            start = self.at
            self.at += 1
            expr = self.expression()
            return expr, self.s[start:self.at] == '[#1]'
        for symbol in ORGANIC:
            if self.s.startswith(symbol, self.at):
                self.at += len(symbol)
                return [[[token(P_ELEM_ALIPH, ATOMIC_NUMBER[symbol])]]], False
        if c in AROMATIC_SYMBOLS:
            self.at += 1
            return [[[token(P_ELEM_AROM, AROMATIC_SYMBOLS[c])]]], False
        if c in ('*', 'a', 'A'):
            self.at += 1
            return [[[token(P_TRUE) if c == '*' else token(P_AROM, 0, c == 'A')]]], False
        return None

    # ---- bonds
    def bond(self):
        """A bond expression at the cursor as ``(mask, written text)``, or ``(None, '')`` when none is written."""
        start = self.at
        clauses, ors, ands, wrote = [], [], ANY_BOND, False
        while self.peek() and self.peek() in '-=#:~@!&,;/\\':
            c = self.peek()
            if c in '/\\':
                self.fail('stereo')
            if c in '&,;':
                if not wrote:
                    self.fail('empty bond expression')
                if c != '&':
                    ors.append(ands)
                    ands = ANY_BOND
                    if c == ';':
                        clauses.append(ors)
                        ors = []
                wrote = False
                self.at += 1
                continue
            neg = False
            while self.peek() == '!':
                neg = not neg
                self.at += 1
            c = self.peek()
            if c not in BOND_PRIMITIVES:
                self.fail('empty bond expression')
            self.at += 1
            ands &= (ANY_BOND & ~BOND_PRIMITIVES[c]) if neg else BOND_PRIMITIVES[c]
            wrote = True
        if self.at == start:
            return None, ''
        if not wrote:
            self.fail('empty bond expression')
        ors.append(ands)
        clauses.append(ors)
        mask = ANY_BOND
        for clause in clauses:
            any_of = 0
            for m in clause:
                any_of |= m
            mask &= any_of
        return mask, self.s[start:self.at]

    # ---- the string
    def parse(self):
        atoms, stack, prev, open_rings = [], [], None, {}
        pending = (None, '')
        while self.at < len(self.s):
            c = self.peek()
            if c == '.':
                self.fail('. components')
            if c == '(':
                if prev is None:
                    self.fail('branch before an atom')
                stack.append(prev)
                self.at += 1
                continue
            if c == ')':
                if not stack or pending[0] is not None:
                    self.fail('unbalanced )')
                prev = stack.pop()
                self.at += 1
                continue
            if c.isdigit() or c == '%':
                start = self.at
                if prev is None:
                    self.fail('ring closure before an atom')
                if c == '%':
                    self.at += 1
                    if not (self.s[self.at:self.at + 2].isdigit() and len(self.s[self.at:self.at + 2]) == 2):
                        self.fail('%nn ring closure', start)
                    label = int(self.s[self.at:self.at + 2])
                    self.at += 2
                else:
                    label = int(c)
                    self.at += 1
                if label in open_rings:
                    other, (mask, text) = open_rings.pop(label)
                    if mask is not None and pending[0] is not None and mask != pending[0]:
                        self.fail('ring closure bonds differ', start)
                    if other == prev:
                        self.fail('ring closure on one atom', start)
                    chosen = pending if pending[0] is not None else (mask, text)
                    final = DEFAULT_BOND if chosen[0] is None else chosen[0]
                    lo, hi = min(prev, other), max(prev, other)           # a check on the later atom against the earlier one,
                    if atoms[hi].parent == lo or any(j == lo for j, _ in atoms[hi].closures):     # whichever end closes
                        self.fail('two bonds between one pair', start)
                    atoms[hi].closures.append((lo, final))
                    atoms[prev].degree += 1
                    atoms[other].degree += 1
                    atoms[prev].ring_closed = True
                    atoms[other].ring_closed = True
                else:
                    open_rings[label] = (prev, pending)
                pending = (None, '')
                continue
            bond = self.bond()
            if bond[0] is not None:
                if pending[0] is not None or prev is None:
                    self.fail('bond without an atom')
                pending = bond
                continue
            column = self.offset + self.at
            got = self.atom()
            if got is None:
                self.fail(f'unexpected {c!r}')
            expr, hydrogen = got
            mask, text = pending
            atom = _Atom(expr, prev, DEFAULT_BOND if mask is None else mask, hydrogen and text in ('', '-'), column)
            atom.exactly_h = hydrogen
            atom.bond_text = text
            atoms.append(atom)
            if prev is not None:
                atom.degree += 1
                atoms[prev].degree += 1
            prev = len(atoms) - 1
            pending = (None, '')
        if stack:
            self.fail('unclosed (')
        if open_rings:
            self.fail('unclosed ring closure')
        if pending[0] is not None:
            self.fail('bond without an atom')
        if not atoms:
            self.fail('zero-atom pattern', 0)
        return self.merge_hydrogens(atoms)

    def merge_hydrogens(self, atoms):
        """Remove the ``[#1]`` leaves (see the module's text) and renumber; any other hydrogen is rejected."""
        n = len(atoms)
        children = [[] for _ in range(n)]
        for k, a in enumerate(atoms):
            if a.parent is not None:
                children[a.parent].append(k)
        removed, gained = set(), [0] * n
        for k, a in enumerate(atoms):
            if not a.exactly_h:
                continue
            if a.degree != 1 or a.ring_closed:
                raise _Fail(a.column, 'explicit hydrogen that is no leaf')
            if a.parent is not None:                                     # hangs off its parent
                other, text = a.parent, a.bond_text
            else:                                                        # the first atom written: its only child hangs off it
                other, text = children[k][0], atoms[children[k][0]].bond_text
            if text not in ('', '-') or atoms[other].exactly_h:
                raise _Fail(a.column, 'explicit hydrogen not joined by a single bond to a heavy atom')
            removed.add(k)
            gained[other] += 1
        for k, a in enumerate(atoms):
            if k in removed:
                continue
            for clause in a.expr:
                for ands in clause:
                    for t in ands:
                        if not isinstance(t, tuple) and not t & NEG and (t & 0xFF) in (P_ELEM, P_ELEM_ALIPH, P_ELEM_AROM) \
                                and (t >> 8 & 0xFFFF) == 1:             # (`!#1`, "no hydrogen", holds for every atom)
                            raise _Fail(a.column, 'explicit hydrogen')
            if gained[k]:
                a.expr = a.expr + [[[token(P_HMIN, gained[k])]]]
        new = {}
        for k in range(n):
            if k not in removed:
                new[k] = len(new)
        out = []
        for k, a in enumerate(atoms):
            if k in removed:
                continue
            a.parent = None if a.parent is None or a.parent in removed else new[a.parent]
            a.closures = [(new[j], m) for j, m in a.closures]
            out.append(a)
        if not out:
            raise _Fail(0, 'zero-atom pattern')
        if any(a.parent is None for a in out[1:]):
            raise _Fail(out[1].column, '. components')
        return out


def _required_element(expr):
    """The atomic number every atom matching the expression must have, or 0: a ``;`` clause all of whose alternatives hold an
    unnegated element primitive of one element."""
    for clause in expr:
        found = set()
        for ands in clause:
            here = {t >> 8 & 0xFFFF for t in ands if not isinstance(t, tuple) and not t & NEG
                    and (t & 0xFF) in (P_ELEM, P_ELEM_ALIPH, P_ELEM_AROM)}
            found.add(min(here) if len(here) == 1 else 0 if not here else -1)
        if len(found) == 1 and min(found) > 0:
            return min(found)
    return 0


def screen_of(atoms):
    """At most ``SCREEN_SLOTS`` words ``Z | count << 8``: a molecule with fewer than ``count`` atoms of element ``Z`` cannot
    hold the pattern (the map is injective).  The rarer elements first: everything but C, N, O, then O, N, C."""
    counts = {}
    for a in atoms:
        z = _required_element(a.expr)
        if z:
            counts[z] = counts.get(z, 0) + 1
    order = sorted(counts, key=lambda z: ({8: 1, 7: 2, 6: 3}.get(z, 0), -counts[z], z))[:SCREEN_SLOTS]
    return [z | min(counts[z], 0xFFFF) << 8 for z in order] + [0] * (SCREEN_SLOTS - len(order))


def _levels(uses):
    """body -> nesting level: 0 for a body without ``$(...)``, else one more than the highest level it uses (a body's text
    holds the bodies it uses, so there is no cycle)."""
    levels = {}

    def level(body):
        if body not in levels:
            levels[body] = 1 + max([level(u) for u in uses[body]], default=-1)
        return levels[body]
    for body in uses:
        level(body)
    return levels


def _compile_one(text, offset, subs):
    parser = _Parser(text, offset, subs)
    atoms = parser.parse()
    if len(atoms) > MAX_PATTERN_ATOMS:
        raise _Fail(offset, f'more than {MAX_PATTERN_ATOMS} pattern atoms')
    for a in atoms:
        if sum(len(ands) for clause in a.expr for ands in clause) > MAX_PRED:
            raise _Fail(a.column, f'more than {MAX_PRED} primitives on one atom')
    return atoms, parser.used


def compile_patterns(rows):
    """``(smarts, name)`` rows (a name may be ``None``: the row number) to a ``Patterns``: host int32 tensors ``pat [Q,8]``
    (sub-patterns first, by level, then the rows), ``atoms [A,6]``, ``closures [C,2]``, ``preds [T]``, and ``n_sub``, ``n_top``,
    ``level_end`` (sub-patterns ``[level_end[L-1], level_end[L])`` have nesting level ``L``), ``names``, ``sub_texts`` and
    ``sub_levels`` in table order.  Raises ``PatternError``."""
    rows = [(r, None) if isinstance(r, str) else tuple(r) for r in rows]
    subs = {}                                      # body text -> (first-appearance index, offset of the body in its row)
    tops, names, uses = [], [], {}
    compiled = {}
    for row, (smarts, name) in enumerate(rows):
        try:
            atoms, used = _compile_one(smarts.strip(), 0, subs)
            tops.append(atoms)
            pending = list(used)
            while pending:                         # the bodies this row brought in, and theirs
                body = pending.pop()
                if body in compiled:
                    continue
                compiled[body], uses[body] = _compile_one(body, subs[body][1], subs)
                pending.extend(uses[body])
        except _Fail as e:
            raise PatternError(row, e.column, e.construct) from None
        except RecursionError:
            raise PatternError(row, 0, 'recursion too deep') from None
        if len(subs) > MAX_SUBPATTERNS:
            raise PatternError(row, 0, f'more than {MAX_SUBPATTERNS} distinct sub-patterns')
        names.append(str(row) if name is None else str(name))
        levels = _levels(uses)
        for body in compiled:
            if levels[body] >= MAX_LEVELS:
                raise PatternError(row, subs[body][1], f'more than {MAX_LEVELS} nesting levels')
    levels = _levels(uses)

    def level(body):
        return levels[body]
    ordered = sorted(compiled, key=lambda body: (level(body), subs[body][0]))
    index = {body: k for k, body in enumerate(ordered)}
    n_levels = max([levels[b] for b in ordered], default=-1) + 1
    level_end = [sum(1 for b in ordered if levels[b] <= L) for L in range(n_levels)]

    pat, atom_rows, closures, preds = [], [], [], []
    for atoms in [compiled[b] for b in ordered] + tops:
        pat.append([len(atom_rows), len(atoms), levels[ordered[len(pat)]] if len(pat) < len(ordered) else n_levels]
                   + screen_of(atoms) + [0])
        for a in atoms:
            pred_off = len(preds)
            for clause in a.expr:
                for i, ands in enumerate(clause):
                    for j, t in enumerate(ands):
                        if isinstance(t, tuple):
                            t = token(P_REC, index[t[1]], t[2])
                        if j == len(ands) - 1:
                            t |= END_AND
                            if i == len(clause) - 1:
                                t |= END_OR
                        preds.append(t)
            atom_rows.append([-1 if a.parent is None else a.parent, a.bond, pred_off, len(preds) - pred_off, len(closures),
                              len(a.closures)])
            closures.extend([j, m] for j, m in a.closures)

    def table(values, width):
        t = torch.tensor(values, dtype=torch.int32).reshape(-1, width) if values else torch.zeros((0, width), dtype=torch.int32)
        return t
    return Patterns(table(pat, PAT_FIELDS), table(atom_rows, ATOM_FIELDS), table(closures, 2),
                    torch.tensor(preds, dtype=torch.int32), len(ordered), len(tops), level_end, names, ordered,
                    [levels[b] for b in ordered])


def read_pattern_file(path):
    """The rows of a pattern file: CSV, the first column the SMARTS, an optional second column a name (the row number when
    there is none), lines that start with ``#`` and empty lines skipped."""
    rows = []
    with open(path, newline='') as f:
        for record in csv.reader(line for line in f if line.strip() and not line.lstrip().startswith('#')):
            if not record or not record[0].strip():
                continue
            name = record[1].strip() if len(record) > 1 and record[1].strip() else str(len(rows))
            rows.append((record[0].strip(), name))
    return rows


def basic_catalogue_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'filters_basic.csv')


def load_catalogue(spec):
    """``'basic'`` (the catalogue shipped with the package) or the path of a pattern file, compiled."""
    return compile_patterns(read_pattern_file(basic_catalogue_path() if spec == 'basic' else spec))
