"""The molecules the canonical-labelling tests share (``test_canon_host.py``, ``test_gpu_canon.py``): named graphs whose
search trees are known, seeded random molecule-like graphs, renumbering, and a small SMILES checker.  Atoms carry element
indices of ``const.ATOM2IDX`` (C 0, O 1, N 2, F 3, S 4); bonds are ``(i, j, order)``."""
import random

C, O, N, F, S = 0, 1, 2, 3, 4


def ring(n, orders):
    return [(i, (i + 1) % n, orders[i % len(orders)]) for i in range(n)]


def chain(n):
    return [C] * n, [(i, i + 1, 1) for i in range(n - 1)]


CUBANE = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1), (4, 5, 1), (5, 6, 1), (6, 7, 1), (7, 4, 1), (0, 4, 1), (1, 5, 1), (2, 6, 1),
          (3, 7, 1)]
CUNEANE = [(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 2, 1), (1, 4, 1), (2, 5, 1), (3, 6, 1), (3, 7, 1), (4, 5, 1), (4, 6, 1), (5, 7, 1),
           (6, 7, 1)]

# name -> (types, bonds, leaves the search evaluates)
NAMED = {
    'benzene': ([C] * 6, ring(6, [2, 1]), 6),
    'six_ring': ([C] * 6, ring(6, [1]), 12),
    'neopentane': ([C] * 5, [(0, k, 1) for k in range(1, 5)], 1),
    'cf3_cyclohexane': ([C] * 7 + [F] * 3, ring(6, [1]) + [(0, 6, 1), (6, 7, 1), (6, 8, 1), (6, 9, 1)], 2),
    'cubane': ([C] * 8, CUBANE, 48),
    'cuneane': ([C] * 8, CUNEANE, 12),
    'two_ethanes': ([C] * 4, [(0, 1, 1), (2, 3, 1)], 8),
    'chain_40': chain(40) + (2,),
    'chain_256': chain(256) + (2,),
    'acetic_acid': ([C, C, O, O], [(0, 1, 1), (1, 2, 2), (1, 3, 1)], None),
    'nitromethane': ([C, N, O, O], [(0, 1, 1), (1, 2, 2), (1, 3, 2)], None),
    'sulfone': ([C, S, O, O, C], [(0, 1, 1), (1, 2, 2), (1, 3, 2), (1, 4, 1)], None),
    'water_oxygen': ([O], [], 1),
    'spiro': ([C] * 5, [(0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 3, 1), (3, 4, 1), (4, 0, 1)], None),
    'decalin': ([C] * 10, ring(6, [1]) + [(4, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 5, 1)], None),
}

STRINGS = {'benzene': 'C1=CC=CC=C1', 'neopentane': 'CC(C)(C)C', 'acetic_acid': 'CC(O)=O', 'nitromethane': 'C[N](=O)=O',
           'two_ethanes': 'CC.CC', 'water_oxygen': 'O'}


def random_graph(seed, least=2, most=24):
    """A molecule-like graph of ``least..most`` atoms (2..24): a random tree, up to three ring bonds, three element types,
    orders 1..2."""
    rng = random.Random(seed)
    n = rng.randint(least, most)
    types = [rng.choice((C, N, O)) for _ in range(n)]
    bonds, pairs = [], set()
    for i in range(1, n):
        j = rng.randrange(i)
        bonds.append((i, j, rng.randint(1, 2)))
        pairs.add((j, i))
    for _ in range(rng.randint(0, 3)):
        i, j = sorted(rng.sample(range(n), 2))
        if (i, j) not in pairs:
            pairs.add((i, j))
            bonds.append((i, j, rng.randint(1, 2)))
    return types, bonds


def renumber(types, bonds, rng):
    """The same molecule with its atoms renumbered at random and its bond list shuffled and randomly oriented."""
    new = list(range(len(types)))
    rng.shuffle(new)
    out = [None] * len(types)
    for i, k in enumerate(new):
        out[k] = types[i]
    rows = [(new[i], new[j], o) if rng.random() < 0.5 else (new[j], new[i], o) for i, j, o in bonds]
    rng.shuffle(rows)
    return out, rows


SYMBOLS = {'C': C, 'O': O, 'N': N, 'F': F, 'S': S}


def parse_smiles(text):
    """The graph a string of ``molecule_builder.smiles`` describes: ``(types, bonds, bracketed atoms, largest ring
    number)``.  Brackets, ring numbers (one digit or ``%nn``), ``=``/``#``, parentheses and ``.`` only."""
    types, bonds, bracketed, open_rings, largest = [], [], [], {}, 0
    previous, order, branch, at = None, 1, [], 0
    while at < len(text):
        ch = text[at]
        at += 1
        if ch == '.':
            assert not branch and order == 1
            previous = None
        elif ch == '(':
            branch.append(previous)
        elif ch == ')':
            previous = branch.pop()
        elif ch in '=#':
            order = 2 if ch == '=' else 3
        elif ch.isdigit() or ch == '%':
            k = int(ch) if ch != '%' else int(text[at:at + 2])
            at += 0 if ch != '%' else 2
            largest = max(largest, k)
            if k in open_rings:
                other, opened = open_rings.pop(k)
                assert order == 1, 'the closing end carries the bare number'
                bonds.append((other, previous, opened))
            else:
                open_rings[k] = (previous, order)
            order = 1
        else:
            inside = ch == '['
            if inside:
                ch, at = text[at], at + 2
                assert text[at - 1] == ']'
            types.append(SYMBOLS[ch])
            if inside:
                bracketed.append(len(types) - 1)
            if previous is not None:
                bonds.append((previous, len(types) - 1, order))
            previous, order = len(types) - 1, 1
    assert not open_rings and not branch
    return types, bonds, bracketed, largest
