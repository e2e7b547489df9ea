"""Hand-built molecules for the substructure search, and for each of them patterns with HAND-DERIVED root sets: the set of
atoms (by atom number) from which the pattern matches, worked out on paper from the rule of ``include/difflinker_hip.h`` -
not produced by ``tests/substructure_ref.py``, which is held against this table (``tests/test_substructure_host.py``) as the
kernel is (``tests/test_gpu_substructure.py``).

A molecule is ``(symbols, bonds, aromatic)``: element symbols by atom number, bonds ``(i, j, Kekule order)`` and the set of
bond positions flagged aromatic.  Heavy atoms only; the default valences are C 4, N 3, O 2, S 2, halogens 1."""
import random


def ring(n, first=0, orders=None):
    return [(first + k, first + (k + 1) % n, (orders or [1] * n)[k]) for k in range(n)]


KEKULE6 = [2, 1, 2, 1, 2, 1]
ALL6 = set(range(6))

MOLECULES = {
    'benzene': (['C'] * 6, ring(6, 0, KEKULE6), ALL6),
    'pyridine': (['N'] + ['C'] * 5, ring(6, 0, KEKULE6), ALL6),
    'pyrrole': (['N'] + ['C'] * 4, ring(5, 0, [1, 2, 1, 2, 1]), set(range(5))),
    'phenol': (['C'] * 6 + ['O'], ring(6, 0, KEKULE6) + [(0, 6, 1)], ALL6),
    'aniline': (['C'] * 6 + ['N'], ring(6, 0, KEKULE6) + [(0, 6, 1)], ALL6),
    'trimethylamine': (['N', 'C', 'C', 'C'], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], set()),
    'acetone': (['C', 'C', 'O', 'C'], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], set()),
    'ethanol': (['C', 'C', 'O'], [(0, 1, 1), (1, 2, 1)], set()),
    'acetamide': (['C', 'C', 'O', 'N'], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], set()),
    'acrylamide': (['C', 'C', 'C', 'O', 'N'], [(0, 1, 2), (1, 2, 1), (2, 3, 2), (2, 4, 1)], set()),
    'acetonitrile': (['C', 'C', 'N'], [(0, 1, 1), (1, 2, 3)], set()),
    # a rhodanine-like ring S0 - C1(=S5) - N2 - C3(=O6) - C4 - S0
    'rhodanine': (['S', 'C', 'N', 'C', 'C', 'S', 'O'], ring(5) + [(1, 5, 2), (3, 6, 2)], set()),
    'cyclopropane': (['C'] * 3, ring(3), set()),
    'cubane': (['C'] * 8, ring(4) + ring(4, 4) + [(k, k + 4, 1) for k in range(4)], set()),
    # two benzene rings (atoms 0-5 and 6-11) joined by the single bond 0 - 6
    'biphenyl': (['C'] * 12, ring(6, 0, KEKULE6) + ring(6, 6, KEKULE6) + [(0, 6, 1)], set(range(12))),
    'two_pieces': (['C', 'O', 'C', 'N'], [(0, 1, 1), (2, 3, 1)], set()),
}

EVERY = {name: set(range(len(m[0]))) for name, m in MOLECULES.items()}

# molecule -> [(pattern, the atoms that root a match)]
EXPECTED = {
    'benzene': [
        ('c', ALL6), ('C', set()), ('[#6]', ALL6), ('a', ALL6), ('A', set()), ('[!a]', set()), ('[!A]', ALL6), ('*', ALL6),
        ('c:c', ALL6), ('c-c', set()), ('cc', ALL6), ('c=c', set()), ('[#6]=[#6]', set()), ('[#6]-[#6]', set()),
        ('[#6]-,:[#6]', ALL6), ('[#6]=,:[#6]', ALL6), ('[#6]~[#6]', ALL6), ('[#6]@[#6]', ALL6), ('[#6]!@[#6]', set()),
        ('[#6]!:[#6]', set()), ('[#6]-;@[#6]', set()), ('c1ccccc1', ALL6), ('c:1:c:c:c:c:c:1', ALL6), ('c%11ccccc%11', ALL6),
        ('[cH]', ALL6), ('[cH0]', set()), ('[D2]', ALL6), ('[!D2]', set()), ('[D3]', set()), ('[X3]', ALL6), ('[!X3]', set()),
        ('[v4]', ALL6), ('[!v4]', set()), ('[R]', ALL6), ('[R0]', set()), ('[!R]', set()), ('[r6]', ALL6), ('[!r6]', set()),
        ('[r5]', set()), ('[r]', ALL6), ('[x2]', ALL6), ('[!x2]', set()), ('[x3]', set()), ('[+0]', ALL6), ('[+]', set()),
        ('[-]', set()), ('[!+]', ALL6), ('[-0]', ALL6), ('[#6;a;D2,D3;!$(*=O)]', ALL6), ('c1ccccc1c', set()),
    ],
    'pyridine': [
        ('n', {0}), ('[nH0]', {0}), ('[nH]', set()), ('[nX2]', {0}), ('c:n', {1, 5}), ('[#7;a]', {0}), ('[#7;A]', set()),
        ('N', set()), ('[n,o]', {0}), ('[c,n]', ALL6), ('[!c]', {0}), ('[!#6;!#7]', set()), ('[!#6,!#7]', ALL6),
        ('[!#1]', ALL6), ('[!C]', ALL6), ('n1ccccc1', {0}), ('c1ccncc1', {3}),
    ],
    'pyrrole': [
        ('[nH]', {0}), ('[nH1]', {0}), ('[nX3]', {0}), ('[r5]', set(range(5))), ('[r6]', set()), ('n1cccc1', {0}),
        ('c1cc[nH]c1', {2, 3}), ('[#7;H1;D2;a]', {0}), ('[h]', set(range(5))),
    ],
    'phenol': [
        ('[OH]', {6}), ('c[OH]', {0}), ('cO', {0}), ('c-O', {0}), ('c:O', set()), ('[OX2H]', {6}), ('[cD3]', {0}),
        ('[#8]!@[#6]', {6}), ('[#8]@[#6]', set()), ('[#8;R0]', {6}), ('[$(c[OH])]', {0}), ('[c;!$(c[OH])]', {1, 2, 3, 4, 5}),
        ('[$(c:[$(c[OH])])]', {1, 5}), ('[!$(*[OH])]', {1, 2, 3, 4, 5, 6}), ('[$(c[OH]),$([OH]c)]', {0, 6}),
        ('[x0]', {6}), ('[r]', ALL6), ('[!r]', {6}),
    ],
    'aniline': [
        ('[#7](-[#1])-[#1]', {6}), ('[NH2]', {6}), ('c[NH2]', {0}), ('[#7](-[#1])(-[#1])-c', {6}), ('[#1]-[#7]-c', {6}),
        ('[#1][#7]', {6}), ('c-[#7](-[#1])-[#1]', {0}), ('[N;!$(NC=O)]', {6}), ('c(:c-[#1]):c-[#1]', {0, 1, 2, 3, 4, 5} - {1, 5}),
    ],
    'trimethylamine': [
        ('[#7](-[#1])-[#1]', set()), ('[#7]-[#1]', set()), ('[NX3]([CH3])([CH3])[CH3]', {0}), ('[ND3]', {0}), ('[NH0]', {0}),
        ('[CH3]', {1, 2, 3}), ('[#6]-[#7]-[#6]', {1, 2, 3}), ('[#6](-[#1])(-[#1])(-[#1])-[#7]', {1, 2, 3}),
        ('[#6](-[#1])(-[#1])(-[#1])(-[#1])', set()), ('N(C)(C)(C)C', set()),
    ],
    'acetone': [
        ('C=O', {1}), ('[#6]=[#8]', {1}), ('O=C', {2}), ('C(=O)(C)C', {1}), ('[CX3]=O', {1}), ('[CH3]', {0, 3}),
        ('[CH3]C(=O)[CH3]', {0, 3}), ('C#O', set()), ('C-O', set()), ('C~O', {1}), ('[O;D1]', {2}), ('[v2]', {2}),
        ('[v4]', {0, 1, 3}), ('[X4]', {0, 3}), ('[X1]', {2}), ('[#6]!-[#8]', {1}), ('[#6]=,:[#8]', {1}), ('[R]', set()),
        ('[R0]', {0, 1, 2, 3}), ('[$(C=O)]', {1}), ('[C;!$(C=O)]', {0, 3}), ('[!C]', {2}), ('[!h]', {1, 2}),
    ],
    'ethanol': [
        ('[OH]', {2}), ('CO', {1}), ('[CH2][OH]', {1}), ('[CH3][CH2]', {0}), ('CCO', {0}), ('OCC', {2}), ('[H3]', {0}),
        ('[h]', {0, 1, 2}), ('[h2]', {1}), ('[!H0]', {0, 1, 2}), ('[H0]', set()), ('[#6]!-[#8]', set()), ('C=O', set()),
        ('CCCO', set()), ('C(C)(O)C', set()), ('[!h]', set()), ('C(CO3)3', set()),
    ],
    'acetamide': [
        ('C(=O)N', {1}), ('NC=O', {3}), ('[NH2]C(=O)C', {3}), ('[#7;H2]', {3}), ('O=C[NH2]', {2}), ('[$(C=O)]N', {1}),
        ('N[$(C=O)]', {3}), ('[N;!$(NC=O)]', set()), ('[#6](=[#8])-[#7](-[#1])-[#1]', {1}),
    ],
    'acrylamide': [
        ('C=CC=O', {0}), ('C=C-C(=O)N', {0}), ('[CH2]=[CH]', {0}), ('C=C', {0, 1}), ('[#6]=[#6]-[#6]=[#8]', {0}),
        ('O=CC=C', {3}), ('C=CC(=O)[NH2]', {0}), ('[#6]=,:[#6]', {0, 1}), ('C=CC=C', set()),
    ],
    'acetonitrile': [
        ('C#N', {1}), ('N#C', {2}), ('[CX2]#N', {1}), ('CC#N', {0}), ('C=N', set()), ('[#6]~[#7]', {1}), ('[ND1]', {2}),
        ('[v3]', {2}), ('C-N', set()), ('[#6]#,=[#7]', {1}),
    ],
    'rhodanine': [
        ('S=C', {5}), ('C=S', {1}), ('[#16]=[#6]', {5}), ('S=C1SCC(=O)N1', {5}), ('[#6]1(=[#16])[#16][#6][#6](=[#8])[#7]1', {1}),
        ('[r5]', {0, 1, 2, 3, 4}), ('[R0]', {5, 6}), ('[#16;R]', {0}), ('[#16;!R]', {5}), ('[#16]@[#6]', {0}),
        ('[#16]!@[#6]', {5}), ('[SX2]', {0}), ('[SX1]', {5}), ('[NH]', {2}), ('[x2]', {0, 1, 2, 3, 4}), ('[x0]', {5, 6}),
        ('[#6]=@[*]', set()), ('[#6]=!@[*]', {1, 3}), ('[$([#6]=[#16]),$([#6]=[#8])]', {1, 3}), ('[#7]([#6]=[#16])[#6]=[#8]', {2}),
    ],
    'cyclopropane': [
        ('C1CC1', {0, 1, 2}), ('C%10CC%10', {0, 1, 2}), ('[r3]', {0, 1, 2}), ('[r]', {0, 1, 2}), ('[r4]', set()),
        ('[R]', {0, 1, 2}), ('C@C', {0, 1, 2}), ('C!@C', set()), ('[CH2]', {0, 1, 2}), ('[x2]', {0, 1, 2}), ('[#6]-;@[#6]', {0, 1, 2}),
        ('C1CCC1', set()), ('C(CC3)3', {0, 1, 2}), ('C(C3)C3', {0, 1, 2}),
    ],
    'cubane': [
        ('[r4]', set(range(8))), ('[x3]', set(range(8))), ('[D3]', set(range(8))), ('[CH]', set(range(8))),
        ('C1CCC1', set(range(8))), ('[r5]', set()), ('C1CC1', set()), ('[r3]', set()),
    ],
    'biphenyl': [
        ('c-c', {0, 6}), ('c:c', set(range(12))), ('cc', set(range(12))), ('c!@c', {0, 6}), ('[cD3]', {0, 6}), ('c-!@c', {0, 6}),
        ('[#6]!:[#6]', {0, 6}), ('[#6]-;!@[#6]', {0, 6}), ('c1ccccc1-c1ccccc1', {1, 5, 7, 11}), ('[$(c-c)]', {0, 6}),
        ('[c;R;!$(c-c)]', set(range(12)) - {0, 6}), ('c=c', set()),
    ],
    'two_pieces': [
        ('CO', {0}), ('CN', {2}), ('OC', {1}), ('[OH]', {1}), ('[NH2]', {3}), ('C~*~C', set()), ('O~C~N', set()),
        ('[CH3]', {0, 2}), ('*', {0, 1, 2, 3}), ('C~*', {0, 2}),
    ],
}


def parse(text):
    """A molecule from a small notation of this file's own, for the alert table below: element symbols (``Cl`` and ``Br``
    too), ``=`` and ``#``, branches and one-digit ring closures; Kekule forms, nothing aromatic."""
    symbols, bonds, stack, rings, prev, order, at = [], [], [], {}, None, 1, 0
    while at < len(text):
        c = text[at]
        at += 1
        if c == '(':
            stack.append(prev)
        elif c == ')':
            prev = stack.pop()
        elif c in '=#':
            order = 2 if c == '=' else 3
        elif c.isdigit():
            if c in rings:
                other, opened = rings.pop(c)
                bonds.append((other, prev, max(opened, order)))
            else:
                rings[c] = (prev, order)
            order = 1
        else:
            if text[at - 1:at + 1] in ('Cl', 'Br'):
                c, at = text[at - 1:at + 1], at + 1
            symbols.append(c)
            if prev is not None:
                bonds.append((prev, len(symbols) - 1, order))
            prev, order = len(symbols) - 1, 1
    assert not stack and not rings
    return symbols, bonds, set()


# every alert of difflinker_amd/data/filters_basic.csv: a molecule that carries the group and a close one that does not
ALERTS = {
    'acyl_halide': ('CC(=O)Cl', 'CC(=O)OC'),                    # acetyl chloride / methyl acetate
    'aldehyde': ('CC=O', 'CC(=O)C'),                            # acetaldehyde / acetone
    'peroxide': ('COOC', 'COC'),                                # dimethyl peroxide / dimethyl ether
    'azide': ('CN=N#N', 'CN=NC'),                               # methyl azide, as N=N#N without charges / azomethane
    'epoxide': ('C1OC1C', 'C1OCC1'),                            # propylene oxide / oxetane
    'aziridine': ('C1NC1', 'C1NCC1'),                           # aziridine / azetidine
    'isocyanate': ('CN=C=O', 'CNC(=O)C'),                       # methyl isocyanate / N-methylacetamide
    'isothiocyanate': ('CN=C=S', 'CN=C=O'),
    'michael_acceptor': ('C=CC(=O)C', 'CCC(=O)C'),              # methyl vinyl ketone / butanone
    'thiol': ('CCS', 'CSC'),                                    # ethanethiol / dimethyl sulfide
    'disulfide': ('CSSC', 'CSCSC'),
    'sulfonyl_halide': ('CS(=O)(=O)Cl', 'CS(=O)(=O)N'),         # mesyl chloride / methanesulfonamide
    'nitroso': ('CN=O', 'CC=NO'),                               # nitrosomethane / acetaldoxime
    'hydrazine': ('CNNC', 'CC(=O)NNC(=O)C'),                    # 1,2-dimethylhydrazine / diacetylhydrazine
    'acid_anhydride': ('CC(=O)OC(=O)C', 'CC(=O)OCC'),           # acetic anhydride / ethyl acetate
    'primary_alkyl_halide': ('CCBr', 'CC(Br)C'),                # bromoethane / 2-bromopropane
    'thiocarbonyl': ('CC(=S)C', 'CC(=O)C'),
    'acyclic_imine': ('CC=NC', 'C1=NCCC1'),                     # N-methylethanimine / 1-pyrroline
    'azo': ('CN=NC', 'CNNC'),
    'acyl_cyanide': ('CC(=O)C#N', 'CC(O)C#N'),                  # pyruvonitrile / lactonitrile
    'vicinal_dicarbonyl': ('CC(=O)C(=O)C', 'CC(=O)CC(=O)C'),    # biacetyl / acetylacetone
    'ynone': ('C#CC(=O)C', 'C#CCC(=O)C'),
}


# ---- the seeded random batch ------------------------------------------------------------------------------------------------------
# Molecule-like graphs and patterns cut out of them, for the comparison of the kernel with the restatement
# (tests/test_gpu_substructure.py); tests/test_substructure_host.py checks that the batch can neither be vacuous (a quarter of the
# pairs hit, a quarter miss) nor hide behind the budget.  Nothing here says what a pattern matches.
VALENCE = {'C': 4, 'N': 3, 'O': 2, 'S': 2, 'F': 1, 'Cl': 1}
NUMBER = {'C': 6, 'N': 7, 'O': 8, 'S': 16, 'F': 9, 'Cl': 17}


def random_molecule(rng, n_max=24, n_min=1):
    """``(symbols, bonds, aromatic)`` of n_min..n_max atoms: a tree grown within the valences, benzene rings hung on it, a few
    five- and six-ring closures and a few double and triple bonds where both ends have room."""
    n = rng.randint(n_min, n_max)
    symbols, bonds, aromatic, free = [], [], set(), []

    def add(symbol):
        symbols.append(symbol)
        free.append(VALENCE[symbol])
        return len(symbols) - 1

    def join(i, j, order, flag=False):
        if flag:
            aromatic.add(len(bonds))
        bonds.append((i, j, order) if rng.random() < 0.5 else (j, i, order))
        free[i] -= order
        free[j] -= order
    add(rng.choice('CCCNO'))
    while len(symbols) < n:
        open_atoms = [k for k in range(len(symbols)) if free[k] > 0]
        if not open_atoms:
            break
        at = rng.choice(open_atoms)
        if n - len(symbols) >= 6 and rng.random() < 0.25:                  # a benzene ring on `at`
            first = len(symbols)
            for _ in range(6):
                add('C' if rng.random() < 0.85 else 'N')
            for k in range(6):
                join(first + k, first + (k + 1) % 6, KEKULE6[k], True)
            if free[first] > 0:
                join(at, first, 1)
            continue
        new = add(rng.choice(['C'] * 6 + ['N', 'N', 'O', 'O', 'S', 'F', 'Cl']))
        order = rng.choice([1, 1, 1, 1, 2, 2, 3])
        join(at, new, min(order, free[at], free[new]))
    pairs = {(min(i, j), max(i, j)) for i, j, _ in bonds}
    for _ in range(rng.randint(0, 2)):                                     # ring closures between atoms 4 or 5 bonds apart
        nbrs = [[] for _ in symbols]
        for i, j in pairs:
            nbrs[i].append(j)
            nbrs[j].append(i)
        start = rng.randrange(len(symbols))
        dist, order = {start: 0}, [start]
        for a in order:
            for w in nbrs[a]:
                if w not in dist:
                    dist[w] = dist[a] + 1
                    order.append(w)
        far = [w for w, d in dist.items() if d in (4, 5) and free[w] > 0 and free[start] > 0]
        if far:
            w = rng.choice(far)
            join(start, w, 1)
            pairs.add((min(start, w), max(start, w)))
    return symbols, bonds, aromatic


def _atom_text(rng, mol, u, loose):
    """A bracket atom that holds for kept atom ``u`` of the restatement's molecule ``mol``."""
    z = mol.z[u]
    roll = rng.random()
    if roll < loose:
        return rng.choice(['*', '[*]', f'[#{z},#{rng.choice([6, 7, 8])}]', 'a' if mol.arom[u] else 'A', f'[!#{9 if z != 9 else 6}]'])
    more = rng.choice(['', '', f';D{mol.d[u]}', f';H{mol.h[u]}', ';!H0' if mol.h[u] else ';H0', f';X{mol.x[u]}', f';v{mol.v[u]}',
                       ';R' if mol.xr[u] else ';R0', f';r{mol.rs[u]}' if mol.rs[u] else ';!r', f';x{mol.xr[u]}',
                       ';a' if mol.arom[u] else ';A', f'&!D{mol.d[u] + 1}', ';+0', f';D{mol.d[u]},D{mol.d[u] + 1}'])
    if z == 6 and not more and rng.random() < 0.5:
        return 'c' if mol.arom[u] else 'C'
    return f'[#{z}{more}]'


def _bond_text(rng, mol, u, v, loose):
    order, aromatic, ring = mol.bond(u, v)
    own = ':' if aromatic else '-=#'[order - 1]
    if rng.random() < loose:
        return rng.choice(['~', '@' if ring else '!@', f'{own},#', '-,:' if own in '-:' else f'{own},:'])
    if own in '-:' and rng.random() < 0.5:
        return ''
    return rng.choice([own, own, f'{own};@' if ring else f'{own};!@'])


def random_pattern(rng, mol, size, loose, recursive=0):
    """A SMARTS string cut out of ``mol`` (a ``substructure_ref.Molecule``): ``size`` connected atoms from a random start in
    depth-first order with branches, the other bonds among them as ring closures now and then; with ``recursive`` levels one
    atom carries a ``$(...)`` over its own surroundings, nested that deep."""
    start = rng.randrange(mol.n)
    chosen, tree, frontier = [start], {start: []}, [start]
    while len(chosen) < size and frontier:
        at = rng.choice(frontier)
        options = [w for w in mol.nbrs[at] if w not in tree]
        if not options:
            frontier.remove(at)
            continue
        w = rng.choice(options)
        tree[at].append(w)
        tree[w] = []
        chosen.append(w)
        frontier.append(w)
    closures, labels = {}, {}
    for u in chosen:
        for w in mol.nbrs[u]:
            if w in tree and u < w and w not in tree[u] and u not in tree[w] and rng.random() < 0.6 and len(labels) < 12:
                label = len(labels) + 1
                labels[u, w] = label
                digit = str(label) if label < 10 else f'%{label}'
                closures.setdefault(u, []).append((w, digit))
                closures.setdefault(w, []).append((u, digit))
    special = rng.choice(chosen) if recursive else None
    written = set()

    def body(u, depth):
        others = [w for w in mol.nbrs[u]]
        if not others:
            return _atom_text(rng, mol, u, 0.0)
        w = rng.choice(others)
        inner = f'[$({body(w, depth - 1)})]' if depth > 1 else _atom_text(rng, mol, w, loose)
        return f'{_atom_text(rng, mol, u, 0.0)}{_bond_text(rng, mol, u, w, loose)}{inner}'

    def write(u):
        written.add(u)
        text = _atom_text(rng, mol, u, loose)
        if u == special:
            text = f'[{text.strip("[]") if text.startswith("[") else "*"};$({body(u, recursive)})]' if rng.random() < 0.7 \
                else f'[$({body(u, recursive)}),$({body(u, 1)})]'
        for w, digit in closures.get(u, []):
            text += (_bond_text(rng, mol, u, w, loose) if w not in written else '') + digit
        children = tree[u]
        for k, w in enumerate(children):
            piece = _bond_text(rng, mol, u, w, loose) + write(w)
            text += piece if k == len(children) - 1 else f'({piece})'
        return text
    return write(start)


def random_batch(seed=7, n_molecules=64, n_patterns=60):
    """``(molecules, smarts)``: the seeded batch of the GPU comparison - 64 graphs of 1..24 atoms and about 60 patterns of
    1..12 atoms cut out of them (paths, branches, rings, loose and tight predicates, a fifth of them recursive, some nested),
    a few made to miss by a changed element."""
    import substructure_ref as sr
    rng = random.Random(seed)
    molecules = [random_molecule(rng) for _ in range(n_molecules)]
    restated = [sr.Molecule([NUMBER[s] for s in m[0]], [VALENCE[s] for s in m[0]], m[1], [k in m[2] for k in range(len(m[1]))])
                for m in molecules]
    smarts = []
    while len(smarts) < n_patterns:
        mol = rng.choice([m for m in restated if m.n >= 1])
        size = min(mol.n, rng.choice([1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 6, 7, 8, 10, 12]))
        recursive = rng.choice([0, 0, 0, 0, 0, 0, 0, 1, 1, 2])
        smarts.append(random_pattern(rng, mol, size, rng.choice([0.2, 0.5, 0.8]), recursive))
    return molecules, smarts


# ---- batches on the host ----------------------------------------------------------------------------------------------------------
# what tests/test_gpu_substructure.py and scripts/time_substructure.py hand to ``metrics.match_patterns``
FILLER = 0x7F7F7F7F


def molecule(symbols, entries, aromatic=(), keep=None, marked=None, status=0, n_bonds=None):
    return dict(symbols=list(symbols), entries=[tuple(e) for e in entries], aromatic=set(aromatic), keep=keep, marked=marked,
                status=status, n_bonds=n_bonds)


def rows_of(b, n, N, scatter):
    return sorted(random.Random(b).sample(range(N), n)) if scatter else list(range(n))


def batch_of(molecules, N, scatter=True, capacity=None):
    """Host tensors of a batch: the atoms of molecule ``b`` on ``len(symbols)`` of ``N`` rows (scattered in row order among
    padding rows unless ``scatter`` is off), the bond list and its aromatic flags as given, and a ``Bonds`` around the list."""
    import torch
    from difflinker_amd import const
    from difflinker_amd.molecule_builder import Bonds
    B = len(molecules)
    capacity = max([len(m['entries']) for m in molecules] + [1]) if capacity is None else capacity
    one_hot, mask = torch.zeros(B, N, const.GEOM_NUMBER_OF_ATOM_TYPES), torch.zeros(B, N)
    drop, mark = torch.zeros(B, N), torch.zeros(B, N)
    bonds = torch.full((B, capacity, 3), FILLER, dtype=torch.int32)
    flags = torch.full((B, capacity), 0, dtype=torch.int32)
    n_bonds, status = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, m in enumerate(molecules):
        for k, r in enumerate(rows_of(b, len(m['symbols']), N, scatter)):
            mask[b, r] = 1
            one_hot[b, r, const.GEOM_ATOM2IDX[m['symbols'][k]]] = 1
            drop[b, r] = float(m['keep'] is not None and not m['keep'][k])
            mark[b, r] = float(m['marked'] is not None and bool(m['marked'][k]))
        for e, row in enumerate(m['entries'][:capacity]):
            bonds[b, e] = torch.tensor(row, dtype=torch.int32)
            flags[b, e] = 7 if e in m['aromatic'] else 0                     # any value but 0 flags the entry
        n_bonds[b] = len(m['entries']) if m['n_bonds'] is None else m['n_bonds']
        status[b] = m['status']
    zeros = torch.zeros(B, N, dtype=torch.int32)
    found = Bonds(n_bonds, bonds, zeros, torch.ones(B, dtype=torch.int32), zeros.clone(), status)
    return one_hot, mask, drop, mark, found, flags


def on_device(found, place):
    return type(found)(*(place(t) for t in found))
