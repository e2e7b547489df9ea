"""The symmetry-aware RMSD without a GPU: ``metrics.isomorphisms`` against hand counts and against the recursion of
``rmsd_ref``, its agreement with ``same_molecule``, the map table's layout, the new C entry (exported, argument-checked, ABI
unchanged), the drivers' flag and ``compute_geometry`` on an empty list."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import rmsd_ref
from test_metrics_host import BICYCLOPENTYL, DECALIN, graph, random_graph, renumbered, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CNO = ([0, 1, 2], [(0, 1, 1), (1, 2, 1)])                             # C-N-O: no symmetry
SIX_RING = ([0] * 6, ring(0, 6))                                      # 6 rotations x 2 directions
CF3_LIKE = ([0, 3, 3, 3, 1], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)])          # a centre, three equal leaves, one other
TWO_CF3 = ([0, 3, 3, 3, 0, 0, 3, 3, 3], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (4, 5, 1), (5, 6, 1), (5, 7, 1), (5, 8, 1)])
TWO_UNLIKE = ([0, 3, 3, 3, 0, 4, 3, 3, 3], TWO_CF3[1])                # the second centre is another element: no end-to-end swap


@pytest.mark.parametrize('mol, count', [(CNO, 1), (SIX_RING, 12), (CF3_LIKE, 6), (TWO_UNLIKE, 36)],
                         ids=['chain', 'six_ring', 'three_equal_leaves', 'two_groups'])
@pytest.mark.parametrize('coloured', [True, False])
def test_isomorphism_counts_by_hand_and_against_the_helper(mol, count, coloured):
    from difflinker_amd.metrics import isomorphisms, same_molecule
    rng = random.Random(count)
    perm = list(range(len(mol[0])))
    rng.shuffle(perm)
    other = renumbered(*mol, perm)
    for a, b in ((mol, mol), (mol, other), (other, mol)):
        maps, truncated = isomorphisms(graph(*a, coloured=coloured), graph(*b, coloured=coloured), 1000)
        want = rmsd_ref.isomorphisms(*a, *b)
        assert len(maps) == count == len(want) and not truncated
        assert sorted(maps) == sorted(want), 'the same set of maps as the plain recursion finds'
        assert all(rmsd_ref.is_isomorphism(m, *a, *b) for m in maps)
        assert same_molecule(graph(*a, coloured=coloured), graph(*b, coloured=coloured))


def test_two_groups_with_an_end_to_end_swap():
    """Two such groups on a carbon chain that reads the same from both ends: 6 x 6 leaf orders times the swap of the ends."""
    from difflinker_amd.metrics import isomorphisms
    maps, truncated = isomorphisms(graph(*TWO_CF3), graph(*TWO_CF3), None)
    assert len(maps) == 72 == len(rmsd_ref.isomorphisms(*TWO_CF3, *TWO_CF3)) and not truncated


def test_limit_cuts_the_enumeration():
    from difflinker_amd.metrics import isomorphisms
    g = graph(*SIX_RING)
    full, _ = isomorphisms(g, g, None)
    maps, truncated = isomorphisms(g, g, 5)
    assert len(maps) == 5 and truncated is True and maps == full[:5]
    maps, truncated = isomorphisms(g, g, 12)
    assert len(maps) == 12 and truncated is False, 'exactly as many as there are: nothing was cut'
    maps, truncated = isomorphisms(g, g, 11)
    assert len(maps) == 11 and truncated is True
    assert isomorphisms(g, g, 0) == ([], False)


@pytest.mark.parametrize('coloured', [True, False])
def test_maps_exist_exactly_when_same_molecule(coloured):
    """Over the graphs ``test_metrics_host`` builds, equal and unequal pairs alike; the first map is what ``same_molecule``
    stops at, so it must be an isomorphism."""
    from difflinker_amd.metrics import Graph, isomorphisms, same_molecule
    rng = random.Random(11)
    pairs = []
    for k in range(240):
        n = rng.randint(1, 7)
        a = random_graph(rng, n)
        if k % 2 == 0:
            perm = list(range(n))
            rng.shuffle(perm)
            b = renumbered(*a, perm)
            rng.shuffle(b[1])
        else:
            b = (a[0], random_graph(rng, n)[1]) if rng.random() < 0.5 or not a[1] else \
                (a[0], a[1][:-1] + [(a[1][-1][0], a[1][-1][1], a[1][-1][2] % 2 + 1)])
        pairs.append((a, b))
    pairs += [(DECALIN, BICYCLOPENTYL), (DECALIN, DECALIN), (BICYCLOPENTYL, BICYCLOPENTYL), (CNO, SIX_RING)]
    equal = 0
    for a, b in pairs:
        ga, gb = graph(*a, coloured=coloured), graph(*b, coloured=coloured)
        maps, truncated = isomorphisms(ga, gb, 100000)
        assert bool(maps) == same_molecule(ga, gb) and not truncated, (a, b)
        want = rmsd_ref.isomorphisms(*a, *b)
        assert sorted(maps) == sorted(want), (a, b)
        if maps:
            assert rmsd_ref.is_isomorphism(maps[0], *a, *b)
            assert isomorphisms(ga, gb, 1)[0] == [maps[0]]
        equal += bool(maps)
    assert 120 <= equal < len(pairs)
    assert len(isomorphisms(graph(*DECALIN), graph(*DECALIN))[0]) == 4
    with pytest.raises(ValueError):
        isomorphisms(Graph([0, 0], [(0, 1, 1), (1, 0, 1)], None), Graph([0, 0], [(0, 1, 1), (1, 0, 1)], None))


def test_map_table_layout_is_atom_major_per_pair():
    from difflinker_amd.metrics import pack_maps
    maps = [[[0, 1, 2], [2, 1, 0]], [], [[1, 0]]]                      # pairs of 3, (none) and 2 atoms; n_max 4
    table, offsets = pack_maps(maps, 4)
    assert table.dtype == torch.int16 and offsets.dtype == torch.int32
    assert offsets.tolist() == [0, 2, 2, 3] and table.numel() == 3 * 4
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'maps[map_offsets[p] * n_max + k * m_p + j]' in header, 'the layout the header states'
    for p, rows in enumerate(maps):
        m = len(rows)
        for j, image in enumerate(rows):
            for k, v in enumerate(image):
                assert int(table[int(offsets[p]) * 4 + k * m + j]) == v
    assert table.tolist() == [0, 2, 1, 1, 2, 0, 0, 0, 1, 0, 0, 0]
    empty, off = pack_maps([], 4)
    assert empty.numel() == 0 and off.tolist() == [0]


def test_export_declared_checked_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    assert 'dl_best_rmsd' in _lib.EXPORTS and 'int32_t dl_best_rmsd(const dl_rmsd_args* args, void* stream);' in header
    assert hasattr(lib, 'dl_best_rmsd') and 'compute_metrics.py:366-402' in header
    assert _lib.EXPORTS[-1] == 'dl_best_rmsd', 'one export, added at the end'
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7 and '#define DL_ABI_VERSION 7' in header
    for name, bit in (('DL_RMSD_NONFINITE', 1), ('DL_RMSD_NO_MAP', 2), ('DL_RMSD_TOO_LARGE', 4)):
        assert f'#define {name} {bit} ' in header and getattr(_lib, name) == bit
    # no GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1) before any device work
    assert lib.dl_best_rmsd(None, None) == -1
    one = ctypes.c_void_p(16)                    # never dereferenced
    names = ('xa', 'xb', 'n_atoms', 'map_offsets', 'maps', 'rmsd', 'best', 'status')
    ok = dict(P=2, n_max=8, maps_capacity=3, **{k: one for k in names})
    for bad in [dict(P=-1), dict(n_max=0), dict(n_max=65537), dict(maps_capacity=-1)] + [{k: None} for k in names]:
        assert lib.dl_best_rmsd(ctypes.byref(_lib.DLRmsdArgs(**dict(ok, **bad))), None) == -1, bad
    empty = _lib.DLRmsdArgs(P=0, n_max=8)
    assert lib.dl_best_rmsd(ctypes.byref(empty), None) == _lib.DL_OK, 'an empty list is DL_OK without a launch'
    empty.n_max = 0
    assert lib.dl_best_rmsd(ctypes.byref(empty), None) == -1


def test_compute_geometry_of_nothing_and_cpu_tensors_raise():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import GEOMETRY_NAMES, best_rmsd, compute_geometry, kept_positions, pack_maps
    from test_metrics_host import ETHANOL, ETHER, molecule
    nothing = {'rmsd': None, 'rmsd_molecules': 0, 'rmsd_truncated': 0}
    assert compute_geometry([], [], [], [], []) == nothing and tuple(nothing) == GEOMETRY_NAMES
    # nothing recovered, or a linker of no atoms: no launch either, so this runs without a GPU
    x = torch.zeros(3, 3)
    assert compute_geometry([molecule(*ETHER)], [molecule(*ETHANOL)], [x], [x], [1]) == nothing
    assert compute_geometry([molecule(*ETHANOL)], [molecule(*ETHANOL)], [x], [x], [0]) == nothing
    with pytest.raises(ValueError):
        compute_geometry([molecule(*ETHANOL)], [], [], [], [])
    table, offsets = pack_maps([[[0, 1, 2]]], 3)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        best_rmsd(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3), torch.tensor([3], dtype=torch.int32), table, offsets)
    # kept_positions is plain tensor code: the numbering of to_host (real rows in order, dropped ones left out)
    pos = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
    mask = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 0, 0, 1]], dtype=torch.float32)[:, :, None]
    drop = torch.tensor([[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], dtype=torch.float32)[:, :, None]
    got, counts = kept_positions(pos, mask)
    assert counts.tolist() == [3, 1] and counts.dtype == torch.int32 and got.shape == (2, 5, 3)
    assert torch.equal(got[0, :3], pos[0, [0, 2, 3]]) and torch.equal(got[1, :1], pos[1, [4]])
    assert float(got[0, 3:].abs().sum()) == 0 and float(got[1, 1:].abs().sum()) == 0
    got, counts = kept_positions(pos, mask, drop)
    assert counts.tolist() == [2, 1] and torch.equal(got[0, :2], pos[0, [0, 3]])


def test_drivers_parse_the_geometry_flag(monkeypatch, capsys):
    from difflinker_amd import sample, train
    seen = []
    monkeypatch.setattr(sample, 'sample', lambda *a, **kw: seen.append((a, kw)))
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--metrics', '--geometry'])
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--metrics'])
    assert seen[0][0][-1] is True and seen[0][1] == {'geometry': True}
    assert seen[1][0][-1] is True and seen[1][1] == {}, 'without the flag the call is what it was'
    with pytest.raises(SystemExit):
        train.main(['--help'])
    assert '--geometry' in capsys.readouterr().out


def test_helper_agrees_with_itself():
    """The pin's own sanity: a rotated copy scores 0, a mirror image of a chiral set does not, maps are searched."""
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(5, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    assert rmsd_ref.kabsch_rmsd(pts, pts @ q.T + 3.0) < 1e-12
    assert rmsd_ref.kabsch_rmsd(pts, pts * [1, 1, -1]) > 0.1
    perm = [3, 0, 4, 1, 2]
    moved = np.empty_like(pts)
    moved[perm] = pts                                                  # atom k of pts is atom perm[k] of moved
    value, index = rmsd_ref.best_rmsd(pts, moved, [[0, 1, 2, 3, 4], perm, perm])
    assert value < 1e-12 and index == 1
