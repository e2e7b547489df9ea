"""Bond perception without a GPU: the restated threshold table against the reference's recorded decisions, the new C
entries (exported, argument-checked, ABI unchanged), the V2000 writer, CPU tensors raise, the drivers' new flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dl_perceive_bonds', 'dl_bonds_workspace_bytes')


def rule(table, a, b, dist):
    """get_bond_order restated over the numeric table: fp32 distance in pm, nested strict comparisons."""
    d = np.float32(100) * np.float32(dist)
    t = table[a][b]
    order = 0
    if d < t[0]:
        order = 1
        if d < t[1]:
            order = 2
            if d < t[2]:
                order = 3
    return order


def test_table_reproduces_every_recorded_decision(golden_dir):
    from difflinker_amd import const
    g = np.load(os.path.join(golden_dir, 'bond_orders.npz'))
    tables = {flag: const.bond_threshold_table(bool(flag)).numpy() for flag in (0, 1)}
    assert tables[0].shape == (8, 8, 3) and tables[1].shape == (9, 9, 3) and tables[1].dtype == np.float32
    seen = set()
    for flag, a, b, dist, want in zip(g['sweep_is_geom'], g['sweep_a'], g['sweep_b'], g['sweep_dist'], g['sweep_order']):
        assert rule(tables[int(flag)], int(a), int(b), dist) == int(want), (flag, a, b, dist, want)
        seen.add((int(flag), int(a), int(b)))
    assert len(seen) == 8 * 8 + 9 * 9, 'every ordered pair of both vocabularies is in the sweep'
    assert set(g['sweep_order'].tolist()) == {0, 1, 2, 3}
    # both sides of every threshold the table has are in the sweep, so no entry is left unpinned
    for flag, table in tables.items():
        for a in range(table.shape[0]):
            for b in range(table.shape[1]):
                sel = (g['sweep_is_geom'] == flag) & (g['sweep_a'] == a) & (g['sweep_b'] == b)
                d = np.float32(100) * g['sweep_dist'][sel]
                for t in table[a, b]:
                    if t > 0:
                        assert (np.abs(d / t - 1) < 2e-4).sum() >= 2 and (d < t).any() and (d > t).any(), (flag, a, b, t)
    assert np.array_equal(tables[0], tables[1][:8, :8])
    assert np.array_equal(tables[1], tables[1].transpose(1, 0, 2))
    wide = const.bond_threshold_table(True, margins=(20, 5, 2)).numpy()
    assert wide[0, 0, 0] == tables[1][0, 0, 0] + 10 and wide[0, 0, 1] == tables[1][0, 0, 1]


def test_new_exports_declared_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and f'{name}(' in header
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7
    assert '#define DL_BONDS_OVERFLOW 1' in header and '#define DL_BONDS_NONFINITE 2' in header
    assert (_lib.DL_BONDS_OVERFLOW, _lib.DL_BONDS_NONFINITE) == (1, 2)


def test_arguments_are_checked_before_device_work():
    """No GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1), never as a HIP error."""
    from difflinker_amd import _lib
    lib = _lib.load()
    assert lib.dl_perceive_bonds(None, None) == -1
    assert lib.dl_bonds_workspace_bytes(256, 50) == 0
    one = ctypes.c_void_p(16)                    # never dereferenced: every call below is refused before any device work
    ok = dict(B=2, N=10, nf=9, one_hot=one, x=one, node_mask=one, table=one, table_len=9 * 9 * 3, capacity=4, n_bonds=one,
              bonds=one, valence=one, n_components=one, component=one, status=one)
    for bad in (dict(N=0), dict(N=1025), dict(nf=0), dict(nf=17), dict(table_len=8 * 8 * 3), dict(B=-1), dict(capacity=-1),
                dict(one_hot=None), dict(x=None), dict(node_mask=None), dict(table=None), dict(n_bonds=None),
                dict(bonds=None), dict(valence=None), dict(n_components=None), dict(component=None), dict(status=None)):
        a = _lib.DLBondsArgs(**dict(ok, **bad))
        assert lib.dl_perceive_bonds(ctypes.byref(a), None) == -1, bad
    empty = _lib.DLBondsArgs(B=0, N=10, nf=9, table_len=9 * 9 * 3)
    assert lib.dl_perceive_bonds(ctypes.byref(empty), None) == 0, 'an empty batch is DL_OK without a launch'
    empty.N = 2000
    assert lib.dl_perceive_bonds(ctypes.byref(empty), None) == -1


def test_cpu_tensors_raise():
    from difflinker_amd import _lib
    from difflinker_amd.molecule_builder import build_xae_molecules, is_connected, perceive_bonds
    h, x, m = torch.zeros(1, 4, 8), torch.zeros(1, 4, 3), torch.ones(1, 4, 1)
    for fn in (perceive_bonds, build_xae_molecules, is_connected):
        with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
            fn(h, x, m, False)


def _toy():
    one_hot = torch.zeros(2, 5, 8)
    types = torch.tensor([[0, 1, 2, 5, 0], [6, 0, 0, 0, 0]])            # C O N Cl (masked) / Br C (rest masked)
    one_hot.scatter_(2, types[:, :, None], 1.0)
    pos = torch.tensor([[[0.0, 0, 0], [1.25, -0.5, 0.123456], [-12.5, 100.25, 3], [9, 9, 9], [7, 7, 7]],
                        [[1.0, 2, 3], [2.5, 2, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0]]])
    mask = torch.tensor([[1.0, 1, 1, 1, 0], [1, 1, 0, 0, 0]])[:, :, None]
    bonds = torch.tensor([[[1, 0, 2], [2, 1, 1], [3, 0, 3], [0, 0, 0]], [[1, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]]])
    return one_hot, pos, mask, bonds, torch.tensor([3, 1])


def test_save_sdf_file_is_fixed_width_v2000_and_reads_back(tmp_path):
    from difflinker_amd import io
    one_hot, pos, mask, bonds, n_bonds = _toy()
    io.save_sdf_file(str(tmp_path), one_hot, pos, mask, bonds, n_bonds, names=['a', 'b'],
                     is_geom=False, suffix='s')
    lines = open(tmp_path / 'a_s.sdf').read().split('\n')
    assert lines[0] == 'a_s' and lines[2] == ''
    assert lines[3] == '  4  3  0  0  0  0  0  0  0  0999 V2000'
    assert lines[4] == '    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0'
    assert lines[5].startswith('    1.2500   -0.5000    0.1235 O   0')
    assert lines[6].startswith('  -12.5000  100.2500    3.0000 N   0')
    assert lines[7].startswith('    9.0000    9.0000    9.0000 Cl  0')
    assert all(len(ln) == 69 for ln in lines[4:8])
    assert lines[8:11] == ['  2  1  2  0  0  0  0', '  3  2  1  0  0  0  0', '  4  1  3  0  0  0  0']
    assert lines[11:] == ['M  END', '$$$$', '']
    mol = io.read_molecule(str(tmp_path / 'a_s.sdf'))
    assert mol.symbols == ['C', 'O', 'N', 'Cl'] and mol.name == 'a_s'
    assert np.abs(mol.positions - pos[0, :4].numpy()).max() <= 5e-5
    second = open(tmp_path / 'b_s.sdf').read().split('\n')
    assert second[3].startswith('  2  1') and second[6] == '  2  1  1  0  0  0  0'
    assert io.read_molecule(str(tmp_path / 'b_s.sdf')).symbols == ['Br', 'C']


def test_save_sdf_file_refuses_what_v2000_cannot_hold(tmp_path):
    from difflinker_amd import io
    one_hot, pos, mask, bonds, n_bonds = _toy()
    with pytest.raises(ValueError, match='its list holds'):                  # a list cut short by its capacity
        io.save_sdf_file(str(tmp_path), one_hot, pos, mask, bonds, torch.tensor([5, 1]), ['a', 'b'], False)
    with pytest.raises(ValueError, match='j < i'):                           # an atom number beyond the molecule
        io.save_sdf_file(str(tmp_path), one_hot, pos, mask, torch.tensor([[[4, 0, 1]], [[1, 0, 1]]]), torch.tensor([1, 1]),
                         ['a', 'b'], False)
    big = 1000
    h = torch.zeros(1, big, 8); h[:, :, 0] = 1
    with pytest.raises(ValueError, match='999'):
        io.save_sdf_file(str(tmp_path), h, torch.zeros(1, big, 3), torch.ones(1, big, 1), torch.zeros(1, 0, 3, dtype=torch.int32),
                         torch.tensor([0]), ['c'], False)
    many = torch.tensor([[[i + 1, 0, 1] for i in range(big)]])
    h = torch.zeros(1, 999, 8); h[:, :, 0] = 1
    with pytest.raises(ValueError, match='999'):
        io.save_sdf_file(str(tmp_path), h, torch.zeros(1, 999, 3), torch.ones(1, 999, 1), many, torch.tensor([big]), ['d'], False)


def test_unknown_output_format_raises(tmp_path):
    from difflinker_amd.generate import _sample_and_save
    with pytest.raises(ValueError, match='output_format'):
        _sample_and_save(None, [], None, None, 1, str(tmp_path), 'x', 'fragment_mask', False, output_format='mol2')


@pytest.mark.parametrize('module', ['difflinker_amd.generate', 'difflinker_amd.sample'])
def test_help_shows_output_format(module):
    out = subprocess.run([sys.executable, '-m', module, '--help'], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert '--output_format {xyz,sdf,both}' in out
