"""Ring perception without a GPU: the plain-Python rule of ``tests/rings_ref.py`` on molecules whose answer is known by hand,
``compute_rings`` on made-up records, and the argument checks of ``dl_ring_scores``, which come before any device work."""
import ctypes
import os

import pytest
import torch

import rings_ref
from difflinker_amd import _lib
from difflinker_amd.metrics import RING_NAMES, RingRecord, Rings, analyze_rings, compute_rings, ring_scores
from difflinker_amd.molecule_builder import Bonds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


@pytest.mark.parametrize('name', sorted(rings_ref.HAND))
def test_hand_molecules(name):
    bond_ring, n_rings = rings_ref.HAND_ANSWERS[name]
    atoms, pairs = rings_ref.HAND[name]
    got = rings_ref.molecule(*rings_ref.hand_molecule(name))
    assert sorted(got['bond_ring']) == bond_ring and got['n_rings'] == n_rings
    assert (got['n_atoms'], got['n_bonds'], got['n_components'], got['status']) == (atoms, len(pairs), 1, 0)
    assert sum(got['ring_hist'][0]) == len(pairs) and got['ring_hist'][1] == [0] * 7, 'nothing is marked'
    for k in range(atoms):                                              # the smallest non-zero value over the atom's bonds
        mine = [r for r, (i, j) in zip(got['bond_ring'], pairs) if k in (i, j) and r]
        assert got['atom_ring'][k] == (min(mine) if mine else 0)
    # the other orientation, another order, a higher bond order: the same answer
    mask, entries, n = rings_ref.hand_molecule(name, order=3)
    flipped = rings_ref.molecule(mask, [(j, i, o) for i, j, o in entries][::-1], n)
    assert flipped['bond_ring'] == got['bond_ring'][::-1]
    assert all(flipped[key] == got[key] for key in rings_ref.PER_MOLECULE)


def test_cyclopropylbenzene_in_detail():
    got = rings_ref.molecule(*rings_ref.hand_molecule('cyclopropylbenzene'))
    assert got['bond_ring'] == [6] * 6 + [0] + [3] * 3
    assert got['atom_ring'] == [6] * 6 + [3] * 3, 'atom 5 carries the bridge and lies in the six-ring; atom 6 in the three-ring'
    assert got['ring_hist'][0] == [1, 3, 0, 0, 6, 0, 0]
    tail = rings_ref.molecule(*rings_ref.hand_molecule('macrocycle_tail'))
    assert tail['ring_hist'][0] == [1, 0, 0, 0, 0, 0, 12] and tail['atom_ring'] == [12] * 12 + [0]


def test_drop_mask_opens_a_ring_and_rows_are_renumbered():
    """Benzene in rows 1, 2, 4, 5, 7, 8 of ten; dropping one atom leaves a chain of five."""
    mask = [0, 1, 1, 0, 1, 1, 0, 1, 1, 0]
    entries = [(i, j, 1) for i, j in rings_ref.ring(6)] + [(7, 7, 7)] * 2          # room beyond n_bonds_in is not read
    whole = rings_ref.molecule(mask, entries, 6)
    assert whole['bond_ring'] == [6] * 6 + [0, 0] and whole['n_rings'] == 1 and whole['status'] == 0
    assert whole['atom_ring'] == [6] * 6 + [0] * 4, 'by atom number, zero from the atom count on'
    drop = [0] * 10
    drop[4] = 1                                                         # row 4 is atom 2
    cut = rings_ref.molecule(mask, entries, 6, drop=drop)
    assert cut['bond_ring'] == [0] * 8 and cut['atom_ring'] == [0] * 10
    assert (cut['n_atoms'], cut['n_bonds'], cut['n_components'], cut['n_rings'], cut['status']) == (5, 4, 1, 0, 0)
    assert cut['ring_hist'][0] == [4, 0, 0, 0, 0, 0, 0], 'the two bonds of the dropped atom are not counted'
    drop[8] = 1                                                         # atom 5 as well: two pieces
    two = rings_ref.molecule(mask, entries, 6, drop=drop)
    assert (two['n_atoms'], two['n_bonds'], two['n_components'], two['n_rings']) == (4, 2, 2, 0)


def test_a_ring_closed_through_a_fragment_atom_is_absent_from_the_linker_view():
    """Fragment atoms 0-2, linker atoms 3-9: the linker is a chain whose two ends sit on fragment atom 1, an eight-ring."""
    n = 10
    pairs = [(0, 1), (1, 2), (1, 3)] + [(k, k + 1) for k in range(3, 9)] + [(9, 1)]
    entries = [(i, j, 1) for i, j in pairs]
    linker = [0.0] * 3 + [1.0] * 7
    ligand = rings_ref.molecule([1.0] * n, entries, len(pairs), mark=linker)
    assert ligand['n_rings'] == 1 and ligand['bond_ring'] == [0, 0] + [8] * 8
    assert ligand['ring_hist'] == [[2, 0, 0, 0, 0, 0, 8], [0, 0, 0, 0, 0, 0, 8]], 'the fragment bonds are not marked'
    alone = rings_ref.molecule([1.0] * n, entries, len(pairs), drop=[1.0 - v for v in linker])
    assert (alone['n_atoms'], alone['n_bonds'], alone['n_components'], alone['n_rings']) == (7, 6, 1, 0)
    assert alone['bond_ring'] == [0] * len(pairs) and alone['ring_hist'][0] == [6, 0, 0, 0, 0, 0, 0]


def test_bad_entries_counts_and_size_limit():
    mask = [1.0] * 5
    square = [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 0, 1)]
    for entry in ((2, 2, 1), (0, 5, 1), (-1, 2, 1), (0, 2, 0), (0, 2, 4)):
        got = rings_ref.molecule(mask, square + [entry], 5)
        assert got['bond_ring'] == [4, 4, 4, 4, 0] and got['status'] == rings_ref.BAD_BOND and got['n_bonds'] == 4, entry
    again = rings_ref.molecule(mask, square + [(2, 1, 1)], 5)            # the pair (1, 2) once more, the other way round
    assert again['bond_ring'] == [4] * 5 and again['status'] == rings_ref.BAD_BOND
    assert (again['n_bonds'], again['n_rings']) == (4, 1) and again['ring_hist'][0][2] == 5, 'entries are counted, pairs make rings'
    lone = rings_ref.molecule(mask, [(1, 0, 1), (2, 1, 1), (3, 2, 1), (0, 3, 1)], 4)
    assert lone['status'] == 0 and lone['bond_ring'] == [4] * 4, 'i < j is as good as j < i'
    over = rings_ref.molecule(mask, square, 9, status_in=2)
    assert over['status'] == 2 | rings_ref.BONDS_OVERFLOW and over['bond_ring'] == [4] * 4
    cut = rings_ref.molecule(mask, square, 3)
    assert cut['bond_ring'] == [0, 0, 0, 0] and cut['n_bonds'] == 3 and cut['status'] == 0
    none = rings_ref.molecule(mask, square, -3)
    assert (none['n_bonds'], none['n_components'], none['n_rings'], none['status']) == (0, 5, 0, 0)
    big = rings_ref.molecule([1.0] * 257, [(0, 1, 1), (9, 9, 9)], 2, status_in=2)
    assert big['n_atoms'] == 257 and big['status'] == 2 | rings_ref.TOO_LARGE, 'the list of a molecule too large is not looked at'
    assert (big['n_bonds'], big['n_components'], big['n_rings']) == (0, 0, 0) and big['bond_ring'] == [0, 0]
    fits = rings_ref.molecule([1.0] * 257, [(0, 1, 1)], 1, drop=[0.0] * 256 + [1.0])
    assert (fits['n_atoms'], fits['n_components'], fits['status']) == (256, 255, 0)


def test_batch_helper_shapes():
    got = rings_ref.ring_scores([[1, 1, 1, 0], [1, 1, 1, 1]], [[(0, 1, 1), (1, 2, 1), (2, 0, 1)], [(0, 1, 1), (0, 0, 0), (0, 0, 0)]],
                                [3, 1])
    assert got['bond_ring'].tolist() == [[3, 3, 3], [0, 0, 0]] and got['n_rings'].tolist() == [1, 0]
    assert got['ring_hist'].shape == (2, 2, 7) and got['atom_ring'].tolist() == [[3, 3, 3, 0], [0, 0, 0, 0]]
    assert got['n_components'].tolist() == [1, 3] and all(got[name].dtype == 'int32' for name in rings_ref.FIELDS)


def record(n_rings, n_rings_ligand, marked, status=0):
    hist = [0] * 7
    for size, count in marked.items():
        hist[rings_ref.ring_bin(size)] += count
    return RingRecord(n_rings, n_rings_ligand, hist, status)


def test_compute_rings():
    pred = [record(1, 3, {0: 2, 6: 6}),                                 # a six-ring in the linker
            record(0, 3, {0: 3, 9: 4}),                                 # a macrocycle closed through the fragments
            record(1, 1, {3: 3, 0: 1}, status=_lib.DL_BONDS_NONFINITE),  # a three-ring; a non-finite coordinate is no flag here
            record(2, 2, {4: 4, 5: 5}, status=_lib.DL_RINGS_BAD_BOND),   # left out
            record(0, 2, {0: 5})]
    got = compute_rings(pred)
    assert list(got) == list(RING_NAMES)
    assert (got['ring_molecules'], got['ring_flagged']) == (4, 1) and type(got['ring_molecules']) is int
    assert got['rings_n'] == 0.5 and got['rings_n_ligand'] == 2.25 and got['ring_free'] == 0.5
    assert got['small_ring'] == 0.25 and got['macrocycle'] == 0.25
    assert [got[name] for name in RING_NAMES[7:]] == [3 / 13, 0.0, 0.0, 6 / 13, 0.0, 4 / 13]
    true = [record(1, 3, {6: 6}), record(1, 3, {6: 6}), record(0, 0, {}, status=_lib.DL_RINGS_TOO_LARGE),
            record(2, 2, {}), record(0, 2, {})]
    both = compute_rings(pred, true)
    assert list(both) == list(RING_NAMES) + ['true_rings_n', 'rings_n_match']
    assert {k: both[k] for k in RING_NAMES} == got
    assert both['true_rings_n'] == 2 / 3 and both['rings_n_match'] == 2 / 3, 'positions 0, 1 and 4: both scored'
    for status in (_lib.DL_BONDS_OVERFLOW, _lib.DL_RINGS_TOO_LARGE, _lib.DL_RINGS_BAD_BOND | _lib.DL_BONDS_NONFINITE):
        assert compute_rings([record(1, 1, {5: 5}, status=status)])['ring_flagged'] == 1
    with pytest.raises(ValueError, match='2 predictions, 1 true'):
        compute_rings(pred[:2], true[:1])


def test_compute_rings_with_nothing_scored():
    for records in ([], [record(1, 1, {5: 5}, status=_lib.DL_RINGS_TOO_LARGE)]):
        got = compute_rings(records, records)
        assert (got['ring_molecules'], got['ring_flagged']) == (0, len(records))
        assert all(got[name] is None for name in RING_NAMES[2:] + ('true_rings_n', 'rings_n_match'))
    no_rings = compute_rings([record(0, 0, {0: 4})])
    assert no_rings['ring_free'] == 1.0 and no_rings['small_ring'] == 0.0 and no_rings['ring_bonds_6'] is None


def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_shape_scores')
    assert _lib.EXPORTS[at + 1] == 'dl_ring_scores', 'right after dl_shape_scores'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_ring_scores(const dl_rings_args* args, void* stream);' in header
    for name, value in (('DL_RINGS_MAX_ATOMS', 256), ('DL_RING_BINS', 7), ('DL_RINGS_TOO_LARGE', 4), ('DL_RINGS_BAD_BOND', 8)):
        assert f'#define {name} {value} ' in header and getattr(_lib, name) == value
    assert (rings_ref.MAX_ATOMS, rings_ref.BINS, rings_ref.TOO_LARGE, rings_ref.BAD_BOND, rings_ref.BONDS_OVERFLOW) == \
        (_lib.DL_RINGS_MAX_ATOMS, _lib.DL_RING_BINS, _lib.DL_RINGS_TOO_LARGE, _lib.DL_RINGS_BAD_BOND, _lib.DL_BONDS_OVERFLOW)
    assert _lib.DL_RINGS_TOO_LARGE == _lib.DL_KEYS_TOO_LARGE and _lib.DL_RINGS_BAD_BOND == _lib.DL_KEYS_BAD_BOND
    assert 'cyclomatic' in header and 'cubane' in header
    lib = _lib.load()
    assert lib.dl_abi_version() == 7 and hasattr(lib, 'dl_ring_scores')
    assert [name for name, _ in _lib.DLRingsArgs._fields_] == [
        'B', 'N', 'node_mask', 'drop_mask', 'mark_mask', 'capacity', 'n_bonds_in', 'bonds', 'status_in', 'n_atoms', 'n_bonds',
        'n_components', 'n_rings', 'bond_ring', 'atom_ring', 'ring_hist', 'status']
    assert Rings._fields == ('n_atoms', 'n_bonds', 'n_components', 'n_rings', 'bond_ring', 'atom_ring', 'ring_hist', 'status',
                             'bonds')


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    call = lambda a: int(lib.dl_ring_scores(ctypes.byref(a), None))      # noqa: E731
    assert int(lib.dl_ring_scores(None, None)) == BAD_ARG
    assert call(_lib.DLRingsArgs(B=2, N=40, capacity=8)) == BAD_ARG      # null pointers
    assert call(_lib.DLRingsArgs(B=2, N=40, capacity=0)) == BAD_ARG      # also when the list may be null
    assert call(_lib.DLRingsArgs(B=-1, N=40, capacity=8)) == BAD_ARG
    # an empty batch is looked at no further than its sizes
    assert call(_lib.DLRingsArgs(B=0, N=40, capacity=8)) == _lib.DL_OK
    assert call(_lib.DLRingsArgs(B=0, N=1, capacity=0)) == _lib.DL_OK and call(_lib.DLRingsArgs(B=0, N=1024, capacity=0)) == _lib.DL_OK
    assert call(_lib.DLRingsArgs(B=0, N=0, capacity=8)) == BAD_ARG
    assert call(_lib.DLRingsArgs(B=0, N=1025, capacity=8)) == BAD_ARG
    assert call(_lib.DLRingsArgs(B=0, N=40, capacity=-1)) == BAD_ARG


def test_cpu_tensors_raise():
    B, N = 2, 6
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)          # noqa: E731
    found = Bonds(i32(B), i32(B, 4 * N, 3), i32(B, N), i32(B), i32(B, N), i32(B))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        ring_scores(torch.ones(B, N, 1), found)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_rings(torch.zeros(B, N, 8), torch.zeros(B, N, 3), torch.ones(B, N, 1), False, torch.zeros(B, N, 1))
