"""Molecule scores without a GPU: the new C entry (exported, argument-checked, ABI unchanged), the valence table against
the reference's recorded ``ALLOWED_BONDS``, the restated key (``mol_keys_ref``) under renumbering and under single changes,
``same_molecule`` against a brute-force search, ``compute_metrics`` on hand-built cases, the drivers' new flags."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

import mol_keys_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_molecules(golden_dir):
    """(types, bonds) of the 96 molecules of bond_orders.npz, from the reference's recorded E matrices."""
    g = np.load(os.path.join(golden_dir, 'bond_orders.npz'))
    out = []
    for k in range(int(g['n_batches'])):
        one_hot, mask, E_all = g[f'b{k}_one_hot'], g[f'b{k}_mask'], g[f'b{k}_E']
        for m in range(len(mask)):
            rows = np.nonzero(mask[m])[0]
            types = one_hot[m][rows].argmax(1).tolist()
            E = E_all[m][:len(rows), :len(rows)]
            out.append((types, [(int(i), int(j), int(E[i, j])) for i, j in zip(*np.nonzero(E))]))
    assert len(out) == 96
    return out


def renumbered(types, bonds, perm):
    """Atom k becomes atom perm[k]."""
    new_types = [0] * len(types)
    for k, t in enumerate(types):
        new_types[perm[k]] = t
    return new_types, [(perm[i], perm[j], o) for i, j, o in bonds]


def graph(types, bonds, coloured=True):
    from difflinker_amd.metrics import Graph
    return Graph(list(types), list(bonds), ref.colours_and_key(types, bonds)[0] if coloured else None)


def molecule(types, bonds, max_valence=(4, 2, 3, 1, 4, 1, 1, 1, 5), status=0):
    """A ``Molecule`` record as ``to_host`` builds it, from the restatement."""
    from difflinker_amd.metrics import Graph, Molecule
    colours, key, _, _ = ref.colours_and_key(types, bonds)
    valence, pieces = ref.valences_and_pieces(types, bonds)
    n_over = sum(v > max_valence[t] for v, t in zip(valence, types))
    return Molecule(ref.signed(key), n_over, pieces, status, Graph(list(types), list(bonds), [ref.signed(c) for c in colours]))


def test_export_declared_checked_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    assert 'dl_molecule_keys' in _lib.EXPORTS and 'dl_molecule_keys(' in header and hasattr(lib, 'dl_molecule_keys')
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7 and '#define DL_ABI_VERSION 7' in header
    assert '#define DL_KEYS_TOO_LARGE 4' in header and '#define DL_KEYS_BAD_BOND 8' in header
    assert (_lib.DL_KEYS_TOO_LARGE, _lib.DL_KEYS_BAD_BOND) == (4, 8)
    # no GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1) before any device work
    assert lib.dl_molecule_keys(None, None) == -1
    one = ctypes.c_void_p(16)                    # never dereferenced
    names = ('one_hot', 'node_mask', 'n_bonds_in', 'bonds', 'valence_in', 'n_components_in', 'status_in', 'max_valence',
             'n_atoms', 'n_over', 'n_components', 'n_bonds', 'key', 'colour', 'status')
    ok = dict(B=2, N=10, nf=9, capacity=4, max_valence_len=9, drop_mask=None, **{k: one for k in names})
    bad_cases = [dict(N=0), dict(N=(1 << 20) + 1), dict(nf=0), dict(nf=17), dict(B=-1), dict(capacity=-1),
                 dict(max_valence_len=8)] + [{k: None} for k in names]
    for bad in bad_cases:
        assert lib.dl_molecule_keys(ctypes.byref(_lib.DLMolKeysArgs(**dict(ok, **bad))), None) == -1, bad
    empty = _lib.DLMolKeysArgs(B=0, N=10, nf=9, max_valence_len=9)
    assert lib.dl_molecule_keys(ctypes.byref(empty), None) == 0, 'an empty batch is DL_OK without a launch'
    empty.max_valence_len = 8
    assert lib.dl_molecule_keys(ctypes.byref(empty), None) == -1


def test_max_valence_table_equals_the_reference(golden_dir):
    from difflinker_amd import const
    g = np.load(os.path.join(golden_dir, 'valence_table.npz'))
    allowed = {str(el): [int(v) for v in row if v >= 0] for el, row in zip(g['elements'], g['allowed'])}
    assert allowed['P'] == [3, 5] and allowed['C'] == [4]
    for is_geom, symbols, idx2atom in ((False, g['zinc_symbols'], const.IDX2ATOM), (True, g['geom_symbols'], const.GEOM_IDX2ATOM)):
        table = const.max_valence_table(is_geom)
        assert table.dtype == torch.int32 and table.shape == (len(symbols),)
        assert [idx2atom[k] for k in range(len(idx2atom))] == [str(s) for s in symbols]
        for k, symbol in enumerate(symbols):
            assert int(table[k]) == max(allowed[str(symbol)]), symbol
            ours = const.ALLOWED_BONDS[str(symbol)]
            assert (ours if isinstance(ours, list) else [ours]) == allowed[str(symbol)], symbol


def test_key_is_unchanged_by_renumbering(golden_dir):
    rng = random.Random(7)
    for types, bonds in fixture_molecules(golden_dir):
        colours, key, n_atoms, n_bonds = ref.colours_and_key(types, bonds)
        assert n_atoms == len(types) and n_bonds == len(bonds) and 0 <= key < 1 << 64
        for _ in range(20):
            perm = list(range(len(types)))
            rng.shuffle(perm)
            t2, b2 = renumbered(types, bonds, perm)
            rng.shuffle(b2)                                           # the order of the list is free too
            b2 = [(j, i, o) if rng.random() < 0.5 else (i, j, o) for i, j, o in b2]
            c2, k2, _, _ = ref.colours_and_key(t2, b2)
            assert k2 == key
            assert all(c2[perm[k]] == colours[k] for k in range(len(types)))


def test_key_changes_with_one_bond_order_or_one_element(golden_dir):
    """A change is visible unless an automorphism maps the changed molecule onto the old one, which cannot happen here:
    changing one bond's order changes the multiset of bond orders, changing one element the multiset of elements."""
    rng = random.Random(8)
    for types, bonds in fixture_molecules(golden_dir):
        key = ref.colours_and_key(types, bonds)[1]
        if bonds:
            e = rng.randrange(len(bonds))
            i, j, o = bonds[e]
            changed = bonds[:e] + [(i, j, o % 3 + 1)] + bonds[e + 1:]
            assert ref.colours_and_key(types, changed)[1] != key
        a = rng.randrange(len(types))
        assert ref.colours_and_key(types[:a] + [(types[a] + 1) % 8] + types[a + 1:], bonds)[1] != key
    # a dropped atom takes its bonds with it: the key of the rest equals the key of the molecule built without it
    types, bonds = fixture_molecules(golden_dir)[0]
    keep = [k != 2 for k in range(len(types))]
    new = {k: (k if k < 2 else k - 1) for k in range(len(types)) if k != 2}
    rest = [(new[i], new[j], o) for i, j, o in bonds if i != 2 and j != 2]
    dropped = ref.colours_and_key(types, bonds, keep)
    alone = ref.colours_and_key(types[:2] + types[3:], rest)
    assert dropped[1:] == alone[1:] and dropped[0][2] == 0 and dropped[0][:2] + dropped[0][3:] == alone[0]


def brute_force_same(a, b):
    (ta, ba), (tb, bb) = a, b
    n = len(ta)
    if n != len(tb) or len(ba) != len(bb):
        return False
    want = {(min(i, j), max(i, j)): o for i, j, o in bb}
    for perm in itertools.permutations(range(n)):
        if all(ta[k] == tb[perm[k]] for k in range(n)) and \
                all(want.get((min(perm[i], perm[j]), max(perm[i], perm[j]))) == o for i, j, o in ba):
            return True
    return False


def random_graph(rng, n):
    types = [rng.choice([0, 0, 0, 1, 2]) for _ in range(n)]
    pairs = [(i, j) for i in range(n) for j in range(i)]
    bonds = [(i, j, rng.choice([1, 1, 2])) for i, j in pairs if rng.random() < 0.4]
    return types, bonds


@pytest.mark.parametrize('coloured', [True, False])
def test_same_molecule_agrees_with_brute_force(coloured):
    from difflinker_amd.metrics import same_molecule
    rng = random.Random(11)
    matches = 0
    for k in range(240):
        n = rng.randint(1, 7)
        a = random_graph(rng, n)
        if k % 2 == 0:                                                # a true match by construction
            perm = list(range(n))
            rng.shuffle(perm)
            b = renumbered(*a, perm)
            rng.shuffle(b[1])
        else:                                                         # the same atoms, bonds drawn again or one bond rewired
            b = (a[0], random_graph(rng, n)[1]) if rng.random() < 0.5 or not a[1] else \
                (a[0], a[1][:-1] + [(a[1][-1][0], a[1][-1][1], a[1][-1][2] % 2 + 1)])
        want = brute_force_same(a, b)
        assert same_molecule(graph(*a, coloured=coloured), graph(*b, coloured=coloured)) == want, (a, b)
        assert k % 2 or want
        matches += want
    assert 120 <= matches < 240


def ring(start, size):
    return [(start + k, start + (k + 1) % size, 1) for k in range(size)]


DECALIN = ([0] * 10, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 0, 1), (4, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1),
                      (9, 5, 1)])                                     # two six-rings sharing the bond 4-5
BICYCLOPENTYL = ([0] * 10, ring(0, 5) + ring(5, 5) + [(0, 5, 1)])     # two five-rings joined by a bond


def test_same_molecule_separates_what_refinement_cannot():
    from difflinker_amd.metrics import group, same_molecule
    key_a, key_b = ref.colours_and_key(*DECALIN)[1], ref.colours_and_key(*BICYCLOPENTYL)[1]
    assert key_a == key_b, '1-WL sees two atoms of degree 3 bonded to each other and eight of degree 2 in both'
    assert not same_molecule(graph(*DECALIN), graph(*BICYCLOPENTYL))
    assert not same_molecule(graph(*DECALIN, coloured=False), graph(*BICYCLOPENTYL, coloured=False))
    rng = random.Random(3)
    graphs = []
    for mol in (DECALIN, BICYCLOPENTYL):
        perm = list(range(10))
        rng.shuffle(perm)
        again = renumbered(*mol, perm)
        assert same_molecule(graph(*mol), graph(*again)) and same_molecule(graph(*again), graph(*mol))
        graphs += [graph(*mol), graph(*again)]
    assert group([key_a] * 4, graphs) == [[0, 1], [2, 3]]
    assert group([1, 2, 1], [graph(*DECALIN)] * 3) == [[0, 2], [1]], 'different keys are never compared'
    # a long chain is matched without recursion
    chain = ([0] * 1500, [(k + 1, k, 1) for k in range(1499)])
    back = renumbered(*chain, list(reversed(range(1500))))
    from difflinker_amd.metrics import Graph
    assert same_molecule(Graph(chain[0], chain[1], None), Graph(back[0], back[1], None))


ETHANOL = ([0, 0, 1], [(1, 0, 1), (2, 1, 1)])                         # C-C-O
ETHANOL_2 = ([1, 0, 0], [(1, 0, 1), (2, 1, 1)])                       # O-C-C: the same molecule
ETHER = ([0, 1, 0], [(1, 0, 1), (2, 1, 1)])                           # C-O-C
PROPANE = ([0, 0, 0], [(1, 0, 1), (2, 1, 1)])
OVER = ([1, 0, 0, 0], [(1, 0, 1), (2, 0, 1), (3, 0, 1)])              # an oxygen with three bonds
PIECES = ([0, 0, 0, 0], [(1, 0, 1), (3, 2, 1)])                       # two pieces


def test_compute_metrics_hand_built_cases():
    from difflinker_amd.metrics import METRIC_NAMES, compute_metrics
    m = {k: molecule(*v) for k, v in dict(ethanol=ETHANOL, ethanol2=ETHANOL_2, ether=ETHER, propane=PROPANE, over=OVER,
                                          pieces=PIECES).items()}
    assert m['over'].n_over == 1 and m['over'].n_components == 1
    assert m['pieces'].n_over == 0 and m['pieces'].n_components == 2
    assert m['ethanol'].key == m['ethanol2'].key != m['ether'].key

    empty = compute_metrics([], [], [])
    assert empty == {k: 0.0 for k in METRIC_NAMES} and all(type(v) is float for v in empty.values())
    assert compute_metrics([]) == {k: 0.0 for k in METRIC_NAMES[:4]}

    # two inputs, three samples each.  input 0 (true: ethanol): ethanol2 (recovered), ether, an over-valent sample.
    # input 1 (true: propane): ether again (a duplicate), two pieces, ethanol (known from the true set, not its own input).
    pred = [m['ethanol2'], m['ether'], m['over'], m['ether'], m['pieces'], m['ethanol']]
    true = [m['ethanol']] * 3 + [m['propane']] * 3
    got = compute_metrics(pred, true, [0, 0, 0, 1, 1, 1])
    assert set(got) == set(METRIC_NAMES) and all(type(v) is float for v in got.values())
    assert got['valence_validity'] == 5 / 6 and got['connectivity'] == 5 / 6 and got['validity_and_connectivity'] == 4 / 6
    assert got['uniqueness'] == 2 / 4, 'ethanol twice and ether twice among four valid and connected samples'
    assert got['novelty'] == 1 / 2, 'ether is in no true molecule, ethanol is'
    assert got['recovery'] == 1 / 2, 'input 0 is recovered, input 1 never samples propane'

    # a true molecule that is itself invalid drops its predictions: input 1 disappears altogether
    for broken in (m['over'], m['pieces'], molecule(*PROPANE, status=2)):
        got = compute_metrics(pred, [m['ethanol']] * 3 + [broken] * 3, [0, 0, 0, 1, 1, 1])
        assert got['valence_validity'] == 2 / 3 and got['connectivity'] == 1.0 and got['validity_and_connectivity'] == 2 / 3
        assert got['uniqueness'] == 1.0 and got['novelty'] == 1 / 2 and got['recovery'] == 1.0
    assert compute_metrics(pred, [m['over']] * 6, [0] * 6) == {k: 0.0 for k in METRIC_NAMES}

    # without true molecules (generation from a fragment file): four scores, nothing dropped
    got = compute_metrics(pred)
    assert set(got) == set(METRIC_NAMES[:4]) and got['validity_and_connectivity'] == 4 / 6 and got['uniqueness'] == 2 / 4
    # a flagged molecule (non-finite coordinate) is not valid
    assert compute_metrics([molecule(*PROPANE, status=2)])['valence_validity'] == 0.0
    with pytest.raises(ValueError):
        compute_metrics(pred, true, [0])
    assert 'not RDKit' in compute_metrics.__doc__ or 'NOT RDKit' in compute_metrics.__doc__


def test_equal_keys_of_different_molecules_do_not_merge():
    """Uniqueness, novelty and recovery go through ``same_molecule``, not through the keys alone."""
    from difflinker_amd.metrics import compute_metrics
    a, b = molecule(*DECALIN), molecule(*BICYCLOPENTYL)
    assert a.key == b.key
    got = compute_metrics([a, b], [a, a], [0, 1])
    assert got['uniqueness'] == 1.0 and got['novelty'] == 1 / 2 and got['recovery'] == 1 / 2


def test_drivers_parse_the_new_flags_and_cpu_tensors_raise(monkeypatch, capsys):
    from difflinker_amd import _lib, generate, sample, train
    from difflinker_amd.metrics import analyze
    seen = {}
    monkeypatch.setattr(sample, 'sample', lambda *a: seen.setdefault('sample', a))
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--metrics'])
    assert seen['sample'][-1] is True
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p'])
    monkeypatch.setattr(generate, 'generate', lambda *a, **kw: seen.setdefault('generate', kw) and [])
    generate.main(['--fragments', 'f.sdf', '--model', 'm.ckpt', '--linker_size', '3', '--metrics'])
    assert seen['generate']['metrics'] is True and seen['generate']['output_format'] == 'xyz'
    with pytest.raises(SystemExit):
        train.main(['--sample_every_epochs'])                          # needs a number
    with pytest.raises(SystemExit):
        train.main(['--help'])
    assert '--sample_every_epochs' in capsys.readouterr().out
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze(torch.zeros(1, 4, 8), torch.zeros(1, 4, 3), torch.ones(1, 4, 1), False)
