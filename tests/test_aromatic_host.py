"""Aromatic-ring perception without a GPU: the plain-Python rule of ``tests/aromatic_ref.py`` on molecules whose answer is known
by hand and on the committed case-study ligands, its invariance under the order of the list and the numbering of the atoms,
``compute_aromatic`` on made-up records, and the argument checks of ``dl_aromatic_rings``, which come before any device work."""
import ctypes
import glob
import math
import os
import random

import numpy as np
import pytest
import torch

import aromatic_ref as ar
from difflinker_amd import _lib, const
from difflinker_amd.io import read_sdf_molecules
from difflinker_amd.metrics import AROMATIC_NAMES, AromaticRecord, analyze_aromatic, compute_aromatic
from difflinker_amd.molecule_builder import Aromatic, Bonds, refine_bond_orders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h
CLASSES = ar.ring_class_table(const.ATOM2IDX)
CASE_STUDIES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', '**', '*.sdf'), recursive=True))


def run(types, points, entries, detail=None, **kwargs):
    return ar.molecule(np.asarray(points, dtype=np.float32), list(types), [1.0] * len(types), list(entries), len(entries),
                       CLASSES, detail=detail, **kwargs)


def doubles(entries, got):
    return sorted((min(i, j), max(i, j)) for (i, j, _), order in zip(entries, got['order_out']) if order == 2)


@pytest.mark.parametrize('name', sorted(ar.HAND))
def test_hand_molecules(name):
    types, points, entries, want = ar.HAND[name]
    detail = {}
    got = run(types, points, entries, detail)
    assert got['status'] == 0
    assert (got['n_planar_rings'], got['n_aromatic_rings']) == (want['planar'], want['aromatic'])
    assert doubles(entries, got) == want['doubles']
    if not want['planar']:
        assert got['order_out'] == [o for _, _, o in entries], 'nothing planar: every order as it came'
    assert got['n_aromatic_marked'] == 0, 'nothing is marked'
    valence = [0] * len(types)
    for (i, j, _), order in zip(entries, got['order_out']):
        valence[i] += order
        valence[j] += order
    assert got['valence_out'] == valence
    ring_atoms = {a for c in detail.get('planar', []) for a in c} if want['aromatic'] == want['planar'] else None
    if ring_atoms is not None:
        assert got['atom_aromatic'] == [int(k in ring_atoms) for k in range(len(types))]


def test_hand_details():
    detail = {}
    got = run(*ar.hand_molecule('cyclopentadiene'), detail=detail)
    assert sorted(detail['role'].values()) == ['P'] * 5 and len(detail['covered']) == 4, 'one P is left uncovered'
    assert got['bond_aromatic'] == [0] * 5 and got['atom_aromatic'] == [0] * 5
    run(*ar.hand_molecule('pyridone'), detail=detail)
    assert detail['role'][0] == 'D' and detail['role'][1] == 'X' and [detail['role'][k] for k in range(2, 6)] == ['P'] * 4
    types, points, entries = ar.hand_molecule('biphenyl')
    got = run(types, points, entries)
    assert got['order_out'][-1] == 1 and got['bond_aromatic'] == [1] * 12 + [0], 'the link bond is untouched'
    got = run(*ar.hand_molecule('dioxin'), detail=detail)
    assert sorted(detail['role'].values()) == ['D', 'D', 'P', 'P', 'P', 'P'], 'two donors and four carbons: eight electrons'
    # the ring that is 0.11 A off its own plane: planar once the tolerance allows 0.12 A
    types, points, entries = ar.hand_molecule('ring_off_plane')
    c, q, m, mm = ar.ring_plane([tuple(float(np.float32(v)) for v in p) for p in points])
    off = [abs(ar.dot(v, m)) / math.sqrt(mm) for v in q]
    assert 0.105 < max(off) < 0.115 and sorted(off)[-2] > 0.105
    assert run(types, points, entries, tol2_ring=0.12 ** 2)['n_aromatic_rings'] == 1
    # the chair: its atoms are 0.25 A off the plane
    c, q, m, mm = ar.ring_plane(ar.HAND['cyclohexane_chair'][1])
    assert all(abs(abs(ar.dot(v, m)) / math.sqrt(mm) - 0.25) < 1e-9 for v in q)


def test_marks_drops_and_bad_entries():
    types, points, entries = ar.hand_molecule('biphenyl')
    x = np.asarray(points, dtype=np.float32)
    mark = [1.0] * 6 + [0.0] * 6
    got = ar.molecule(x, types, [1.0] * 12, entries, len(entries), CLASSES, mark=mark)
    assert (got['n_aromatic_rings'], got['n_aromatic_marked']) == (2, 1)
    drop = [0.0] * 12
    drop[7] = 1.0                                # opens the second ring
    got = ar.molecule(x, types, [1.0] * 12, entries, len(entries), CLASSES, drop=drop)
    assert got['n_planar_rings'] == 1 and got['atom_aromatic'] == [1] * 6 + [0] * 6 and got['valence_out'][7] == 0
    assert got['order_out'][6:12] == [1] * 6 and got['status'] == 0, 'a bond with a dropped end keeps its order; no error'
    bad = entries + [(0, 0, 1), (0, 1, 0), (0, 1, 4), (1, 0, 3), (0, 12, 1)]
    got = ar.molecule(x, types, [1.0] * 12, bad, len(bad), CLASSES)
    assert got['status'] == ar.BAD_BOND and got['order_out'][-5:] == [0, 0, 0, 2, 0], 'the repeated pair gets the pair\'s order'
    assert got['valence_out'] == run(types, points, entries)['valence_out'], 'and counts once'
    got = ar.molecule(x, types, [1.0] * 12, entries, len(entries) + 1, CLASSES, status_in=2)
    assert got['status'] == 2 | ar.BONDS_OVERFLOW


def test_limits():
    types, points, entries = ar.strip(8)         # 34 atoms in one system
    got = run(types, points, entries)
    assert got['status'] == ar.BIG_SYSTEM and (got['n_planar_rings'], got['n_aromatic_rings']) == (8, 0)
    assert got['order_out'] == [1] * len(entries) and got['bond_aromatic'] == [0] * len(entries)
    types, points, entries = ar.strip(7)         # 30 atoms
    got = run(types, points, entries)
    assert got['status'] == 0 and (got['n_planar_rings'], got['n_aromatic_rings']) == (7, 7)
    assert got['valence_out'] == [4 if v == 3 else 3 for v in np.bincount([a for e in entries for a in e[:2]]).tolist()]


def case_study_molecules():
    out = []
    for path in CASE_STUDIES:
        for mol in read_sdf_molecules(path)[0]:
            if all(s in const.ATOM2IDX for s in mol.symbols):
                out.append((os.path.relpath(path, ROOT), mol))
    return out


def test_case_studies_are_aromatic_and_within_valence():
    """Every chordless 5- or 6-cycle of the eight case-study files is an aromatic ring of a crystal ligand: planar and aromatic
    under the rule, and with the new orders no atom exceeds its valence.  Hydrogens are removed by the reader and the files'
    aromatic order 4 is replaced by 1."""
    assert len(CASE_STUDIES) == 8
    rings = 0
    for path, mol in case_study_molecules():
        types = [const.ATOM2IDX[s] for s in mol.symbols]
        entries = [(i, j, 1 if order == 4 else order) for i, j, order in mol.bonds]
        detail = {}
        got = run(types, mol.positions, entries, detail)
        adj = {k: set() for k in range(len(types))}
        for i, j, _ in entries:
            adj[i].add(j)
            adj[j].add(i)
        cycles = ar.candidate_rings(adj, {k: True for k in adj})
        assert got['status'] == 0 and got['n_planar_rings'] == got['n_aromatic_rings'] == len(cycles), path
        rings += len(cycles)
        for k, s in enumerate(mol.symbols):
            assert got['valence_out'][k] <= const.ALLOWED_BONDS[s], (path, k, s)
    assert rings == 29


def test_benzene_of_5ou2_and_3fi3():
    """The rings the distance table gets wrong: six doubles in the 5OU2 fragment, two in 3FI3; three after the rule."""
    for path in ('impdh/5ou2_fragments_input.sdf', 'jnk/3fi3_ligand.sdf'):
        mol = read_sdf_molecules(os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', path))[0][0]
        types = [const.ATOM2IDX[s] for s in mol.symbols]
        entries = [(i, j, 1 if order == 4 else order) for i, j, order in mol.bonds]
        detail = {}
        got = run(types, mol.positions, entries, detail)
        benzenes = [c for c in detail['planar'] if len(c) == 6 and all(mol.symbols[a] == 'C' for a in c)]
        assert benzenes
        for c in benzenes:
            for a in c:
                mine = [o for (i, j, _), o in zip(entries, got['order_out']) if a in (i, j) and (i in c and j in c)]
                assert sorted(mine) == [1, 2], 'each benzene carbon carries exactly one double bond'


def renumbered(types, points, entries, rng):
    n = len(types)
    new = list(range(n))
    rng.shuffle(new)                             # old atom k becomes new[k]
    back = sorted(range(n), key=lambda k: new[k])
    listed = [(new[i], new[j], o) if rng.random() < 0.5 else (new[j], new[i], o) for i, j, o in entries]
    return [types[k] for k in back], [points[k] for k in back], listed, new


def test_invariance_under_list_order_and_numbering():
    rng = random.Random(11)
    nprng = np.random.default_rng(3)
    molecules = [ar.hand_molecule(name) for name in sorted(ar.HAND)] + [ar.random_fused(nprng) for _ in range(12)]
    for known, (types, points, entries) in enumerate(molecules):
        base = run(types, points, entries)
        order = list(range(len(entries)))
        rng.shuffle(order)
        shuffled = run(types, points, [entries[e] for e in order])
        assert shuffled['order_out'] == [base['order_out'][e] for e in order]
        assert shuffled['bond_aromatic'] == [base['bond_aromatic'][e] for e in order]
        assert all(shuffled[key] == base[key] for key in ar.PER_MOLECULE)
        # another numbering: the planar rings and the weight of the matching hold.  Its third criterion looks at the atom
        # numbers, so the double bonds may sit elsewhere - compared by their number, the valences by their sum - and where
        # a two-bonded N may or may not be covered the electron count of a ring can change with it: the aromatic rings are
        # compared for the hand molecules only, whose answer does not hang on that
        t2, p2, e2, new = renumbered(types, points, entries, rng)
        other = run(t2, p2, e2)
        assert other['n_planar_rings'] == base['n_planar_rings'] and other['status'] == base['status']
        assert sorted(other['order_out']) == sorted(base['order_out']) and sum(other['valence_out']) == sum(base['valence_out'])
        if known < len(ar.HAND):
            assert other['n_aromatic_rings'] == base['n_aromatic_rings']
            assert [other['atom_aromatic'][new[k]] for k in range(len(types))] == base['atom_aromatic']
            assert other['bond_aromatic'] == base['bond_aromatic'], 'the list kept its order'


def test_kekule_against_listing_every_matching():
    rng = random.Random(5)
    for _ in range(300):
        n = rng.randint(2, 9)
        degree, edges = [0] * n, set()
        for _ in range(rng.randint(1, 11)):
            u, v = rng.sample(range(n), 2)
            if degree[u] < 3 and degree[v] < 3 and len(edges) < 11 and (min(u, v), max(u, v)) not in edges:
                edges.add((min(u, v), max(u, v)))
                degree[u] += 1
                degree[v] += 1
        adj = {k: set() for k in range(n)}
        for u, v in edges:
            adj[u].add(v)
            adj[v].add(u)
        role = {k: rng.choice('PPPFFDX') for k in range(n)}
        assert ar.kekule(range(n), adj, role) == ar.kekule_brute(range(n), adj, role)


def test_ring_class_tables():
    assert const.ring_class_table(False).tolist() == [1, 3, 2, 0, 3, 0, 0, 0] == ar.ring_class_table(const.ATOM2IDX).tolist()
    assert const.ring_class_table(True).tolist() == [1, 3, 2, 0, 3, 0, 0, 0, 0] == ar.ring_class_table(const.GEOM_ATOM2IDX).tolist()
    assert const.ring_class_table(True).dtype == torch.int32
    for table, idx in ((const.ring_class_table(False), const.ATOM2IDX), (const.ring_class_table(True), const.GEOM_ATOM2IDX)):
        assert {name: int(table[k]) for name, k in idx.items() if table[k]} == {'C': 1, 'N': 2, 'O': 3, 'S': 3}


def record(n_linker, n_aromatic, n_planar, filtered, over, status=0):
    return AromaticRecord(n_linker, n_aromatic, n_planar, filtered, over, status)


def test_compute_aromatic():
    pred = [record(1, 2, 2, 0, 0), record(0, 1, 2, 2, 0), record(0, 0, 0, 0, 1, status=_lib.DL_BONDS_NONFINITE),
            record(3, 3, 3, 0, 0, status=_lib.DL_AROM_BIG_SYSTEM), record(1, 1, 1, 0, 0)]
    got = compute_aromatic(pred)
    assert list(got) == list(AROMATIC_NAMES)
    assert (got['aromatic_molecules'], got['aromatic_flagged']) == (4, 1) and type(got['aromatic_molecules']) is int
    assert got['aromatic_rings_n'] == 0.5 and got['ring_filter'] == 0.75 and got['valence_validity_geometric'] == 0.75
    true = [record(1, 1, 1, 0, 0), record(1, 1, 1, 0, 0), record(0, 0, 0, 0, 0, status=_lib.DL_AROM_TOO_LARGE),
            record(0, 0, 0, 0, 0), record(0, 0, 0, 1, 1)]
    both = compute_aromatic(pred, true)
    assert list(both) == list(AROMATIC_NAMES) + ['true_aromatic_rings_n', 'true_ring_filter', 'true_valence_validity_geometric']
    assert {k: both[k] for k in AROMATIC_NAMES} == got
    assert both['true_aromatic_rings_n'] == 2 / 3 and both['true_ring_filter'] == 2 / 3, 'positions 0, 1 and 4: both scored'
    for status in (_lib.DL_BONDS_OVERFLOW, _lib.DL_AROM_TOO_LARGE, _lib.DL_AROM_BAD_BOND, _lib.DL_AROM_MANY_RINGS):
        assert compute_aromatic([record(1, 1, 1, 0, 0, status=status)])['aromatic_flagged'] == 1
    nothing = compute_aromatic([], [])
    assert nothing['aromatic_molecules'] == 0 and all(nothing[k] is None for k in AROMATIC_NAMES[2:])
    with pytest.raises(ValueError, match='2 predictions, 1 true'):
        compute_aromatic(pred[:2], true[:1])


def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_fragment_multicuts')
    assert _lib.EXPORTS[at + 1] == 'dl_aromatic_rings' and _lib.EXPORTS[-1] == 'dl_best_rmsd', 'right after dl_fragment_multicuts'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_aromatic_rings(const dl_aromatic_args* args, void* stream);' in header and '#define DL_ABI_VERSION 7' in header
    for name, value in (('DL_AROM_MAX_ATOMS', 256), ('DL_AROM_MAX_RINGS', 64), ('DL_AROM_MAX_SYSTEM', 32), ('DL_AROM_TOO_LARGE', 4),
                        ('DL_AROM_BAD_BOND', 8), ('DL_AROM_MANY_RINGS', 16), ('DL_AROM_BIG_SYSTEM', 32)):
        assert f'#define {name} {value} ' in header and getattr(_lib, name) == value
    assert (ar.MAX_ATOMS, ar.MAX_RINGS, ar.MAX_SYSTEM, ar.TOO_LARGE, ar.BAD_BOND, ar.MANY_RINGS, ar.BIG_SYSTEM, ar.BONDS_OVERFLOW) == \
        (_lib.DL_AROM_MAX_ATOMS, _lib.DL_AROM_MAX_RINGS, _lib.DL_AROM_MAX_SYSTEM, _lib.DL_AROM_TOO_LARGE, _lib.DL_AROM_BAD_BOND,
         _lib.DL_AROM_MANY_RINGS, _lib.DL_AROM_BIG_SYSTEM, _lib.DL_BONDS_OVERFLOW)
    assert _lib.DL_AROM_TOO_LARGE == _lib.DL_KEYS_TOO_LARGE and _lib.DL_AROM_BAD_BOND == _lib.DL_KEYS_BAD_BOND
    for words in ('NOT RDKit', "NOT OpenBabel's", 'lexicographically smallest', 'chordless', 'contraction off', 'no formal charges'):
        assert words in header, words
    lib = _lib.load()
    assert lib.dl_abi_version() == 7 and hasattr(lib, 'dl_aromatic_rings')
    assert [name for name, _ in _lib.DLAromaticArgs._fields_] == [
        'B', 'N', 'nf', 'x', 'one_hot', 'node_mask', 'drop_mask', 'mark_mask', 'ring_class', 'capacity', 'n_bonds_in', 'bonds',
        'status_in', 'tol2_ring', 'tol2_sub', 'order_out', 'bond_aromatic', 'atom_aromatic', 'valence_out', 'n_planar_rings',
        'n_aromatic_rings', 'n_aromatic_marked', 'status']
    assert Aromatic._fields == ('bond_aromatic', 'atom_aromatic', 'n_planar_rings', 'n_aromatic_rings', 'n_aromatic_marked',
                                'status')


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    call = lambda a: int(lib.dl_aromatic_rings(ctypes.byref(a), None))   # noqa: E731
    ok = dict(B=2, N=40, nf=8, capacity=8, tol2_ring=0.01, tol2_sub=0.25)
    assert int(lib.dl_aromatic_rings(None, None)) == BAD_ARG
    assert call(_lib.DLAromaticArgs(**ok)) == BAD_ARG                    # null pointers
    assert call(_lib.DLAromaticArgs(**dict(ok, capacity=0))) == BAD_ARG  # also when the list may be null
    for wrong in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict(tol2_ring=-1.0),
                  dict(tol2_sub=float('nan'))):
        assert call(_lib.DLAromaticArgs(**{**ok, 'B': 0, **wrong})) == BAD_ARG, wrong
    # an empty batch is looked at no further than its sizes
    assert call(_lib.DLAromaticArgs(**dict(ok, B=0))) == _lib.DL_OK
    assert call(_lib.DLAromaticArgs(**dict(ok, B=0, N=1024, capacity=0))) == _lib.DL_OK


def test_python_callers_refuse_the_cpu():
    found = Bonds(*(torch.zeros(s, dtype=torch.int32) for s in ((1,), (1, 4, 3), (1, 6), (1,), (1, 6), (1,))))
    one_hot, x, mask = torch.zeros(1, 6, 8), torch.zeros(1, 6, 3), torch.ones(1, 6, 1)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        refine_bond_orders(found, one_hot, x, mask, False)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_aromatic(one_hot, x, mask, False, mask)


def test_command_lines_keep_their_defaults(monkeypatch):
    """Without the new switches ``generate`` and ``sample`` are called exactly as before; with them the new keywords appear."""
    from difflinker_amd import generate as gen, sample as smp
    seen = {}
    monkeypatch.setattr(gen, 'generate', lambda *a, **k: seen.update(k) or [])
    gen.main(['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3'])
    assert 'bond_orders' not in seen and 'aromatic' not in seen
    gen.main(['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3', '--bond_orders', 'geometric', '--aromatic'])
    assert seen['bond_orders'] == 'geometric' and seen['aromatic'] is True
    seen.clear()
    monkeypatch.setattr(smp, 'sample', lambda *a, **k: seen.update(k) or 'out')
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p'])
    assert 'bond_orders' not in seen and 'aromatic' not in seen
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p', '--bond_orders', 'geometric', '--aromatic'])
    assert seen['bond_orders'] == 'geometric' and seen['aromatic'] is True
    with pytest.raises(ValueError, match='bond_orders must be one of'):
        gen._sample_and_save(None, [], None, None, 1, '.', 'n', 'k', False, bond_orders='obabel')
