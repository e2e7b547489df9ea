"""Double cuts without a GPU: the plain-Python rule of ``tests/fragment_ref.py`` on molecules whose answer is known by hand,
``fragment.examples`` on a made-up result, ``io.read_sdf_molecules``, and the argument checks of ``dl_fragment_cuts``, which
come before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fragment_ref
from difflinker_amd import _lib, const
from difflinker_amd.datasets import collate
from difflinker_amd.fragment import CUT_FIELDS, Cuts, examples, fragment_all, fragment_cuts
from difflinker_amd.io import read_molecule, read_sdf_molecules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


def cuts_of(got):
    return [dict(zip(CUT_FIELDS, row)) for row in got['cuts'][:got['n_cuts']]]


def pieces(got):
    return [(c['n_frag_1'], c['n_linker'], c['n_frag_2']) for c in cuts_of(got)]


@pytest.mark.parametrize('n, kept', [(12, []), (13, [(5, 3, 5)]), (14, [(5, 3, 6), (5, 4, 5), (6, 3, 5)])])
def test_linear_chains(n, kept):
    """a + m + c = n with a, c >= 5 and 3 <= m <= min(a, c)."""
    got = fragment_ref.hand(f'chain{n}')
    assert got['n_cuttable'] == n - 1 and got['n_cuts'] == len(kept) and pieces(got) == kept and got['status'] == 0
    assert got['bond_side'] == list(range(1, n)), 'bond k is (k, k + 1): k + 1 atoms on the side of its atom i'
    for c in cuts_of(got):
        assert c['path_atoms'] == c['n_linker'] and c['e1'] < c['e2']
        assert (c['anchor_1'], c['exit_1'], c['exit_2'], c['anchor_2']) == (c['e1'], c['e1'] + 1, c['e2'], c['e2'] + 1)
    for r, c in enumerate(cuts_of(got)):
        want = [0] * c['n_frag_1'] + [2] * c['n_linker'] + [1] * c['n_frag_2']
        assert got['labels'][r] == want
    assert got['labels'][got['n_cuts']:] == [[255] * n] * (64 - got['n_cuts']) and got['cuts'][got['n_cuts']] == [0] * 10


def test_orientation_and_order_of_the_list_do_not_change_the_pieces():
    mask, one_hot, entries, n_in, charge = fragment_ref.hand_molecule('chain14')
    flipped = [(j, i, order) for i, j, order in entries][::-1]
    got = fragment_ref.molecule(mask, one_hot, flipped, n_in, 8, charge)
    assert got['bond_side'] == list(range(1, 14)), 'entry k is now the bond (13 - k, 12 - k): 14 - (12 - k + 1) atoms beyond'
    assert sorted(pieces(got)) == [(5, 3, 6), (5, 4, 5), (6, 3, 5)]
    first = cuts_of(got)[0]
    assert (first['e1'], first['e2']) == (4, 7) and (first['anchor_1'], first['exit_1']) == (9, 8), 'fragment 1 is beyond e1'
    assert (first['anchor_2'], first['exit_2'], first['n_frag_1'], first['n_frag_2']) == (5, 6, 5, 6)


def test_amide_and_ester():
    for name in ('amide', 'ester'):
        got = fragment_ref.hand(name)
        types, entries, _ = fragment_ref.HAND[name]
        side = dict(zip([tuple(e[:2]) for e in entries], got['bond_side']))
        assert side[(5, 7)] == 0, 'C(=O)-N / C(=O)-O is not cuttable: the carbonyl carbon does not qualify, the other end is no carbon'
        assert side[(5, 6)] == 0, 'a double bond'
        assert side[(4, 5)] == 5, 'C(=O)-C is cuttable through its other end'
        assert side[(7, 8)] == 8, 'N-C / O-C is cuttable through the carbon'
        assert got['n_cuttable'] == 10 and pieces(got) == [(5, 3, 5)]
        cut = cuts_of(got)[0]
        assert (cut['anchor_1'], cut['exit_1'], cut['exit_2'], cut['anchor_2'], cut['path_atoms']) == (4, 5, 7, 8, 2)
        assert got['labels'][0] == [0] * 5 + [2] * 3 + [1] * 5


def test_n_o_charges_and_orders():
    got = fragment_ref.hand('n_o')
    assert got['bond_side'] == [1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 11], 'the N-O bond 5-6 is never cuttable; C-N and O-C are'
    got = fragment_ref.hand('charged')
    assert got['bond_side'][5] == 0 and got['bond_side'][4] == 5 and got['bond_side'][6] == 7 and got['n_cuttable'] == 10
    mask, one_hot, entries, n_in, _ = fragment_ref.hand_molecule('charged')
    assert fragment_ref.molecule(mask, one_hot, entries, n_in, 4)['n_cuttable'] == 11, 'charge=None is 0 everywhere'
    got = fragment_ref.hand('orders')
    assert [got['bond_side'][e] for e in (5, 6, 7)] == [0, 0, 0], 'double, triple and aromatic bonds are never cut'
    assert got['n_cuttable'] == 10 and pieces(got) == [(5, 4, 5)] and cuts_of(got)[0]['path_atoms'] == 4
    # a carbon with a double bond to a hetero atom can still be the OTHER end; two of them make no cuttable bond
    types = [fragment_ref.C, fragment_ref.C, fragment_ref.O, fragment_ref.O]
    one_hot = [[float(t == k) for k in range(3)] for t in types]
    got = fragment_ref.molecule([1.0] * 4, one_hot, [(0, 1, 1), (0, 2, 2), (1, 3, 2)], 3, 2)
    assert got['bond_side'] == [0, 0, 0] and got['n_cuttable'] == 0 and got['status'] == 0
    one_hot[3] = [1.0, 0.0, 0.0]                                        # C=C in place of C=O on atom 1
    assert fragment_ref.molecule([1.0] * 4, one_hot, [(0, 1, 1), (0, 2, 2), (1, 3, 2)], 3, 2)['bond_side'] == [2, 0, 0]


def test_rings_are_never_cut():
    got = fragment_ref.hand('biphenyl_tails')
    _, entries, _ = fragment_ref.HAND['biphenyl_tails']
    assert all(side == 0 for side in got['bond_side'][:6] + got['bond_side'][7:13]), 'the twelve ring bonds'
    assert got['bond_side'][6] == 11 and got['n_cuttable'] == 11 and got['n_cuts'] == 0, 'every linker is larger than a tail'
    got = fragment_ref.hand('biphenyl_tails', linker_leq_frags=0)
    assert pieces(got) == [(11, 6, 5), (11, 6, 5), (5, 12, 5)]
    assert [c['path_atoms'] for c in cuts_of(got)] == [4, 4, 8], 'half round a ring; both rings and the bond between them'
    assert [(c['anchor_1'], c['exit_1'], c['anchor_2'], c['exit_2']) for c in cuts_of(got)] == \
        [(6, 5, 12, 2), (5, 6, 17, 9), (12, 2, 17, 9)]
    assert got['labels'][0] == [2] * 6 + [0] * 6 + [1] * 5 + [0] * 5


def test_branched_linker_with_a_ring_and_star():
    assert fragment_ref.hand('ring_linker')['n_cuts'] == 0
    got = fragment_ref.hand('ring_linker', linker_leq_frags=0)
    assert pieces(got) == [(5, 6, 5)] and cuts_of(got)[0]['path_atoms'] == 3, 'the path 5-6-7 is shorter than the linker'
    assert got['labels'][0] == [0] * 5 + [2] * 6 + [1] * 5
    assert fragment_ref.hand('star', linker_leq_frags=0)['n_cuts'] == 0, 'both exits are the core atom: one atom on the path'
    got = fragment_ref.hand('star', linker_leq_frags=0, min_path_atoms=1)
    assert pieces(got) == [(5, 6, 5)] * 3 and all(c['path_atoms'] == 1 and c['exit_1'] == c['exit_2'] == 0 for c in cuts_of(got))
    assert got['labels'][1] == [2] + [0] * 5 + [2] * 5 + [1] * 5, 'the linker is the core and the third arm'


def test_bad_entries_pieces_and_limits():
    mask, one_hot, entries, n_in, charge = fragment_ref.hand_molecule('chain13')
    clean = fragment_ref.molecule(mask, one_hot, entries, n_in, 4, charge)
    for entry in ((2, 2, 1), (0, 13, 1), (-1, 2, 1), (0, 2, 0), (0, 2, 5)):
        got = fragment_ref.molecule(mask, one_hot, entries + [entry], n_in + 1, 4, charge)
        assert got['status'] == fragment_ref.BAD_BOND and got['cuts'] == clean['cuts'] and got['bond_side'] == clean['bond_side'] + [0]
    # a repeated pair: the first entry is the bond, with its order
    again = fragment_ref.molecule(mask, one_hot, entries + [(5, 4, 2)], n_in + 1, 4, charge)
    assert again['status'] == fragment_ref.BAD_BOND and again['n_bonds'] == 12 and again['cuts'] == clean['cuts']
    first = fragment_ref.molecule(mask, one_hot, [(5, 4, 2)] + entries, n_in + 1, 4, charge)
    assert first['n_cuts'] == 0 and first['bond_side'][0] == 0 and first['bond_side'][5] == 0, 'now the bond 4-5 is double'
    # two pieces: cuttable bonds are still counted, nothing is cut
    two = fragment_ref.molecule(mask, one_hot, entries[:6] + entries[7:], n_in - 1, 4, charge)
    assert two['status'] == fragment_ref.DISCONNECTED and two['n_cuts'] == 0 and two['n_cuttable'] == 11
    assert two['bond_side'][6] == 1, 'the bond 7-8: atom 7 alone on its side'
    # records: truncation keeps the count whole
    mask, one_hot, entries, n_in, charge = fragment_ref.hand_molecule('chain14')
    short = fragment_ref.molecule(mask, one_hot, entries, n_in, 2, charge, status_in=2)
    assert short['n_cuts'] == 3 and short['status'] == 2 | fragment_ref.TRUNCATED and len(short['cuts']) == 2
    none = fragment_ref.molecule(mask, one_hot, entries, n_in, 0, charge)
    assert none['n_cuts'] == 3 and none['cuts'] == [] and none['labels'] == []
    over = fragment_ref.molecule(mask, one_hot, entries, n_in + 5, 4, charge)
    assert over['status'] == fragment_ref.BONDS_OVERFLOW and over['n_cuts'] == 3
    lone = fragment_ref.molecule([0.0, 1.0, 0.0], [[1.0, 0.0]] * 3, [(0, 0, 0)], 0, 1)
    assert (lone['n_atoms'], lone['n_cuttable'], lone['n_cuts'], lone['status']) == (1, 0, 0, 0) and lone['labels'] == [[255] * 3]
    empty = fragment_ref.molecule([0.0, 0.0], [[1.0, 0.0]] * 2, [], 0, 1)
    assert (empty['n_atoms'], empty['n_cuts'], empty['status']) == (0, 0, 0)
    big = fragment_ref.molecule([1.0] * 257, [[1.0]] * 257, [(k, k + 1, 1) for k in range(256)], 256, 1, status_in=2)
    assert big['n_atoms'] == 257 and big['status'] == 2 | fragment_ref.TOO_LARGE
    assert (big['n_bonds'], big['n_cuttable'], big['n_cuts']) == (0, 0, 0) and big['bond_side'] == [0] * 256
    # the type is the FIRST largest entry of the row
    tie = fragment_ref.molecule([1.0] * 2, [[0.5, 0.5, 0.1], [0.0, 0.7, 0.7]], [(0, 1, 1)], 1, 1)
    assert tie['n_cuttable'] == 1, 'atom 0 is type 0: carbon'
    assert fragment_ref.molecule([1.0] * 2, [[0.4, 0.5, 0.1], [0.0, 0.7, 0.7]], [(0, 1, 1)], 1, 1)['n_cuttable'] == 0


def test_batch_helper_shapes():
    one_hot = np.zeros((2, 14, 3), np.float32)
    one_hot[:, :, 0] = 1
    mask = np.ones((2, 14), np.float32)
    mask[1, 13] = 0
    bonds = np.array([fragment_ref.chain(14), fragment_ref.chain(14)])
    got = fragment_ref.fragment_cuts(mask, one_hot, bonds, [13, 12], 4)
    assert got['n_cuts'].tolist() == [3, 1] and got['cuts'].shape == (2, 4, 10) and got['labels'].shape == (2, 4, 14)
    assert got['labels'].dtype == np.uint8 and all(got[k].dtype == np.int32 for k in fragment_ref.FIELDS if k != 'labels')
    assert got['labels'][1, 0].tolist() == [0] * 5 + [2] * 3 + [1] * 5 + [255] and got['bond_side'][1, 12] == 0


def made_up_result():
    """Two molecules: a chain of 13 by the reference rule, and one without cuts."""
    got = fragment_ref.fragment_cuts(np.ones((2, 13), np.float32), np.tile([1.0, 0, 0, 0, 0, 0, 0, 0], (2, 13, 1)),
                                     np.array([fragment_ref.chain(13)[::-1], fragment_ref.chain(13)]), [12, 3], 2)
    return Cuts(*(torch.as_tensor(got[name]) for name in fragment_ref.FIELDS))


def test_examples():
    result = made_up_result()
    assert result.n_cuts.tolist() == [1, 0]
    symbols = [['C'] * 4 + ['N'] + ['C'] * 3 + ['O'] + ['C'] * 4, ['C'] * 13]
    positions = [np.arange(39, dtype=np.float64).reshape(13, 3) / 7, np.zeros((13, 3))]
    data, rows = examples(result, symbols, positions, ['first', 'second'], False, with_rows=True)
    assert examples(result, symbols, positions, ['first', 'second'], False)[0].keys() == data[0].keys()
    assert len(data) == 1 and rows == [(0, 0, 9, 5, 5, 3)]
    item = data[0]
    assert list(item) == ['uuid', 'name', 'positions', 'one_hot', 'charges', 'anchors', 'fragment_mask', 'linker_mask', 'num_atoms']
    assert (item['uuid'], item['name'], item['num_atoms']) == (0, 'first', 13)
    # the list was reversed: e1 is the bond (8, 7), fragment 1 the atoms 8..12, fragment 2 the atoms 0..4, the linker 5, 6, 7
    order = [8, 9, 10, 11, 12, 0, 1, 2, 3, 4, 5, 6, 7]
    assert torch.equal(item['positions'], torch.tensor(positions[0][order], dtype=torch.float32))
    assert item['charges'].tolist() == [{'C': 6.0, 'N': 7.0, 'O': 8.0}[symbols[0][k]] for k in order]
    assert item['one_hot'].argmax(1).tolist() == [const.ATOM2IDX[symbols[0][k]] for k in order]
    assert item['one_hot'].shape == (13, const.NUMBER_OF_ATOM_TYPES) and item['one_hot'].sum(1).tolist() == [1.0] * 13
    assert item['anchors'].tolist() == [1.0] + [0.0] * 4 + [0.0] * 4 + [1.0] + [0.0] * 3, 'atom 8 and atom 4'
    assert item['fragment_mask'].tolist() == [1.0] * 10 + [0.0] * 3 and item['linker_mask'].tolist() == [0.0] * 10 + [1.0] * 3
    assert all(item[k].dtype == torch.float32 for k in list(item)[2:8])
    geom = examples(result, symbols, positions, ['first', 'second'], True)
    assert geom[0]['one_hot'].shape == (13, const.GEOM_NUMBER_OF_ATOM_TYPES)
    batch = collate([item, dict(item, uuid=1)])
    assert batch['positions'].shape == (2, 13, 3) and batch['anchors'].shape == (2, 13, 1) and batch['uuid'] == [0, 1]
    assert batch['edge_mask'].shape == (2 * 13 * 13, 1) and int(batch['atom_mask'].sum()) == 26
    truncated = result._replace(n_cuts=torch.tensor([3, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match='fragment_all'):
        examples(truncated, symbols, positions, ['first', 'second'], False)


V2000 = '''ethanolamine
  made by hand            3D

  7  6  0  0  0  0  0  0  0  0999 V2000
    0.0000    0.0000    0.1000 C   0  0  0  0  0  0  0  0  0  0  0  0
    1.5000    0.0000    0.2000 H   0  0  0  0  0  0  0  0  0  0  0  0
    1.5000    1.4000    0.3000 C   0  0  0  0  0  0  0  0  0  0  0  0
    2.5000    1.4000    0.4000 N   0  3  0  0  0  0  0  0  0  0  0  0
    3.5000    1.4000    0.5000 H   0  0  0  0  0  0  0  0  0  0  0  0
    2.5000    2.4000    0.6000 O   0  0  0  0  0  0  0  0  0  0  0  0
    2.5000    3.4000    0.7000 Cl  0  0  0  0  0  0  0  0  0  0  0  0
  1  2  1  0  0  0  0
  1  3  1  0  0  0  0
  4  3  2  0  0  0  0
  4  5  1  0  0  0  0
  4  6  4  0  0  0  0
  7  6  1  0  0  0  0
M  CHG  2   4   1   6  -1
M  END
> <note>
kept out of the way

$$$$
'''
BROKEN = '''broken
  made by hand            3D

  3  2  0  0  0  0  0  0  0  0999 V2000
    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0
    oops
M  END
$$$$
'''
V3000 = '''
  made by hand            3D

  0  0  0     0  0            999 V3000
M  V30 BEGIN CTAB
M  V30 COUNTS 4 3 0 0 0
M  V30 BEGIN ATOM
M  V30 10 C 0.5 0.25 1.5 0
M  V30 20 H 0.5 0.25 2.5 0
M  V30 30 S 1.5 0.25 1.5 0 CHG=-1
M  V30 40 Br 2.5 0.25 1.5 0
M  V30 END ATOM
M  V30 BEGIN BOND
M  V30 1 1 10 20
M  V30 2 3 30 10
M  V30 3 1 30 40
M  V30 END BOND
M  V30 END CTAB
M  END
$$$$
'''
FLAT = '''flat
  made by hand            2D

  2  1  0  0  0  0  0  0  0  0999 V2000
    0.0000    0.0000    0.0000 C   0  5  0  0  0  0  0  0  0  0  0  0
    1.5000    0.0000    0.0000 O   0  0  0  0  0  0  0  0  0  0  0  0
  1  2  1  0  0  0  0
M  END
'''


def test_read_sdf_molecules(tmp_path):
    path = os.path.join(tmp_path, 'mols.sdf')
    with open(path, 'w') as f:
        f.write(V2000 + BROKEN + V3000 + FLAT)
    molecules, malformed = read_sdf_molecules(path)
    assert malformed == 1 and [m.name for m in molecules] == ['ethanolamine', 'record_2', 'flat']
    first, second, flat = molecules
    assert first.symbols == ['C', 'C', 'N', 'O', 'Cl'] and len(first) == 5
    assert first.bonds == [(0, 1, 1), (2, 1, 2), (2, 3, 4), (4, 3, 1)], 'the hydrogens went with their bonds; the rest is renumbered'
    assert first.charges == [0, 0, 1, -1, 0], 'M  CHG replaces the charge column'
    assert first.positions.shape == (5, 3) and first.positions[2].tolist() == [2.5, 1.4, 0.4] and first.is_3d
    assert second.symbols == ['C', 'S', 'Br'] and second.bonds == [(1, 0, 3), (1, 2, 1)] and second.charges == [0, -1, 0]
    assert second.positions[1].tolist() == [1.5, 0.25, 1.5] and second.is_3d
    assert flat.symbols == ['C', 'O'] and flat.charges == [-1, 0] and not flat.is_3d, 'the charge column: 5 is -1'
    alone = read_molecule(path)
    assert alone.symbols == first.symbols and np.array_equal(alone.positions, first.positions), 'read_molecule is what it was'


def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_ring_scores')
    assert _lib.EXPORTS[at + 1] == 'dl_fragment_cuts' and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_fragment_cuts(const dl_fragment_args* args, void* stream);' in header
    for name, value in (('DL_FRAG_MAX_ATOMS', 256), ('DL_FRAG_CUT_FIELDS', 10), ('DL_FRAG_TOO_LARGE', 4), ('DL_FRAG_BAD_BOND', 8),
                        ('DL_FRAG_DISCONNECTED', 16), ('DL_FRAG_TRUNCATED', 32)):
        assert f'#define {name} {value} ' in header and getattr(_lib, name) == value
    assert (fragment_ref.MAX_ATOMS, fragment_ref.CUT_FIELDS, fragment_ref.TOO_LARGE, fragment_ref.BAD_BOND,
            fragment_ref.DISCONNECTED, fragment_ref.TRUNCATED, fragment_ref.BONDS_OVERFLOW) == \
        (_lib.DL_FRAG_MAX_ATOMS, _lib.DL_FRAG_CUT_FIELDS, _lib.DL_FRAG_TOO_LARGE, _lib.DL_FRAG_BAD_BOND,
         _lib.DL_FRAG_DISCONNECTED, _lib.DL_FRAG_TRUNCATED, _lib.DL_BONDS_OVERFLOW)
    assert _lib.DL_FRAG_TOO_LARGE == _lib.DL_KEYS_TOO_LARGE and _lib.DL_FRAG_BAD_BOND == _lib.DL_KEYS_BAD_BOND
    assert '[#6+0;!$(*=,#[!#6])]!@!=!#[*]' in header and 'n_linker <= min(n_frag_1, n_frag_2)' in header
    lib = _lib.load()
    assert lib.dl_abi_version() == 7 and hasattr(lib, 'dl_fragment_cuts')
    assert [name for name, _ in _lib.DLFragmentArgs._fields_] == [
        'B', 'N', 'nf', 'one_hot', 'node_mask', 'charge', 'carbon_type', 'capacity', 'n_bonds_in', 'bonds', 'status_in',
        'min_linker', 'min_fragment', 'min_path_atoms', 'linker_leq_frags', 'R', 'n_atoms', 'n_bonds', 'n_cuttable', 'n_cuts',
        'status', 'bond_side', 'cuts', 'labels']
    assert Cuts._fields == fragment_ref.FIELDS and len(CUT_FIELDS) == _lib.DL_FRAG_CUT_FIELDS


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    call = lambda **kw: int(lib.dl_fragment_cuts(ctypes.byref(_lib.DLFragmentArgs(**kw)), None))      # noqa: E731
    assert int(lib.dl_fragment_cuts(None, None)) == BAD_ARG
    assert call(B=2, N=40, nf=8, capacity=8, R=4) == BAD_ARG            # null pointers
    assert call(B=2, N=40, nf=8, capacity=0, R=0) == BAD_ARG            # also when the lists may be null
    assert call(B=-1, N=40, nf=8, capacity=8, R=4) == BAD_ARG
    # an empty batch is looked at no further than its sizes
    assert call(B=0, N=40, nf=8, capacity=8, R=4) == _lib.DL_OK
    assert call(B=0, N=1, nf=1, capacity=0, R=0) == _lib.DL_OK and call(B=0, N=1024, nf=9, carbon_type=8, capacity=0, R=0) == _lib.DL_OK
    assert call(B=0, N=0, nf=8, capacity=8, R=4) == BAD_ARG
    assert call(B=0, N=1025, nf=8, capacity=8, R=4) == BAD_ARG
    assert call(B=0, N=40, nf=0, capacity=8, R=4) == BAD_ARG
    assert call(B=0, N=40, nf=8, carbon_type=8, capacity=8, R=4) == BAD_ARG
    assert call(B=0, N=40, nf=8, carbon_type=-1, capacity=8, R=4) == BAD_ARG
    assert call(B=0, N=40, nf=8, capacity=-1, R=4) == BAD_ARG
    assert call(B=0, N=40, nf=8, capacity=8, R=-1) == BAD_ARG


def test_cpu_tensors_raise():
    B, N = 2, 6
    args = (torch.zeros(B, N, 8), torch.ones(B, N), torch.zeros(B, 5, 3, dtype=torch.int32), torch.zeros(B, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        fragment_cuts(*args, is_geom=False, capacity=4)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        fragment_all(*args, is_geom=False)


def test_prepare_command_line_has_the_rule_options():
    from difflinker_amd import prepare
    with pytest.raises(SystemExit) as done:
        prepare.main(['--help'])
    assert done.value.code == 0
    with pytest.raises(SystemExit):
        prepare.main(['--out', 'x', '--prefix', 'y'])                  # no --sdf
    assert prepare.TABLE_COLUMNS == ('uuid', 'molecule', 'anchor_1', 'anchor_2', 'n_frag_1', 'n_frag_2', 'n_linker')
