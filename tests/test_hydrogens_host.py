"""Host side of the explicit hydrogens (``dl_add_hydrogens``): the plain-Python rule of ``tests/hydrogens_ref.py`` on textbook
molecules, the export and its declaration, the SDF writer with and without a ``Hydrogens``, and the ``generate`` switch.  No
GPU: the kernel is compared with the same reference in ``tests/test_gpu_hydrogens.py``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hydrogens_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETRAHEDRAL = 109.4712206


def run(name, planar=True):
    """``(heavy positions, {parent: [hydrogen positions]}, h_count)`` of a hand-made molecule by the reference."""
    m = hr.hand_molecule(name)
    n = len(m['types'])
    flags = np.zeros(n)
    if planar:
        flags[m['planar']] = 1
    valence, length = hr.tables()
    x = np.asarray(m['points'], dtype=np.float32)
    n_h, h_count, parents, points, status, _ = hr.molecule(x, m['types'], np.ones(n), m['entries'], len(m['entries']), valence,
                                                           length, planar=flags)
    assert status == 0 and n_h == len(parents) == sum(h_count)
    by_parent = {}
    for parent, point in zip(parents, points):
        by_parent.setdefault(parent, []).append(np.asarray(point))
    assert parents == sorted(parents), 'listed by parent atom number'
    return x.astype(np.float64), by_parent, h_count


@pytest.mark.parametrize('name', sorted(hr.HAND) + sorted(hr.DEGENERATE))
def test_counts_and_lengths_of_every_hand_made_molecule(name):
    heavy, hs, h_count = run(name)
    assert h_count == (hr.HAND.get(name) or hr.DEGENERATE[name])[3]
    _, length = hr.tables()
    types = hr.hand_molecule(name)['types']
    for parent, points in hs.items():
        for p in points:
            want = length[types[parent]]
            assert abs(np.linalg.norm(p - heavy[parent]) - want) <= 1e-12 * want, 'exactly the table length'
        for a in range(len(points)):
            for b in range(a):
                assert np.linalg.norm(points[a] - points[b]) > 1.0, 'no two hydrogens of an atom in one place'


def test_methane_is_a_regular_tetrahedron():
    heavy, hs, _ = run('lone_C')
    pts = hs[0]
    assert len(pts) == 4
    for a in range(4):
        for b in range(a):
            assert abs(hr.angle(pts[a], heavy[0], pts[b]) - TETRAHEDRAL) < 1e-6


def test_ethane_is_staggered():
    heavy, hs, _ = run('ethane')
    for c, other in ((0, 1), (1, 0)):
        for a in range(3):
            assert abs(hr.angle(hs[c][a], heavy[c], heavy[other]) - TETRAHEDRAL) < 1e-6
            for b in range(a):
                assert abs(hr.angle(hs[c][a], heavy[c], hs[c][b]) - TETRAHEDRAL) < 1e-6
    torsions = sorted(abs(hr.torsion(p, heavy[0], heavy[1], q)) for p in hs[0] for q in hs[1])
    assert np.allclose(torsions, [60] * 6 + [180] * 3, atol=1e-6)


def test_a_methyl_group_is_staggered_to_the_chain():
    heavy, hs, _ = run('propane')
    for methyl, far in ((0, 2), (2, 0)):
        torsions = [hr.torsion(p, heavy[methyl], heavy[1], heavy[far]) for p in hs[methyl]]
        assert abs(abs(torsions[0]) - 180) < 1e-6, 'the first hydrogen is anti to r'
        assert np.allclose(sorted(torsions[1:]), [-60, 60], atol=1e-6)
    a, b = hs[1]
    assert abs(hr.angle(a, heavy[1], b) - TETRAHEDRAL) < 1e-6
    assert abs((a + b)[2] / 2) < 1e-12 and abs(a[2] + b[2]) < 1e-12, 'one above and one below the plane of the chain'


def test_ethene_is_planar_with_120_degrees():
    heavy, hs, _ = run('ethene')
    for c, other in ((0, 1), (1, 0)):
        a, b = hs[c]
        assert abs(hr.angle(a, heavy[c], heavy[other]) - 120) < 1e-6 and abs(hr.angle(b, heavy[c], heavy[other]) - 120) < 1e-6
        assert abs(hr.angle(a, heavy[c], b) - 120) < 1e-6
    torsions = sorted(abs(hr.torsion(p, heavy[0], heavy[1], q)) for p in hs[0] for q in hs[1])
    assert np.allclose(torsions, [0, 0, 180, 180], atol=1e-6)
    heavy, hs, _ = run('propene')
    assert np.allclose(sorted(abs(hr.torsion(p, heavy[0], heavy[1], heavy[2])) for p in hs[0]), [0, 180], atol=1e-6)
    assert abs(abs(hr.torsion(hs[0][0], heavy[0], heavy[1], heavy[2])) - 180) < 1e-6, 'the first is trans to r'
    assert abs(hr.angle(hs[1][0], heavy[1], heavy[0]) - 120) < 1e-4 and abs(hs[1][0][2]) < 1e-12


def test_ethyne_is_linear():
    heavy, hs, _ = run('propyne')
    assert len(hs[0]) == 1 and abs(hr.angle(hs[0][0], heavy[0], heavy[1]) - 180) < 1e-6
    assert 1 not in hs and len(hs[2]) == 3


def test_ring_hydrogens_lie_in_the_plane_and_point_outwards():
    heavy, hs, _ = run('benzene')
    for k in range(6):
        (p,) = hs[k]
        assert abs(p[2]) < 1e-12 and np.linalg.norm(p) > np.linalg.norm(heavy[k]) + 1.0
    heavy, hs, _ = run('pyrrole')
    assert abs(hs[0][0][2]) < 1e-12, 'the flag puts the N-H in plane'
    heavy, hs, _ = run('pyrrole', planar=False)
    assert abs(hs[0][0][2]) > 0.5, 'without it the nitrogen is tetrahedral'


def test_the_random_builder_keeps_nine_draws_in_ten():
    molecules, draws = hr.random_molecules(np.random.default_rng(3), 64)
    assert len(molecules) == 64 and 64 / draws >= 0.9, draws
    sizes = [len(m['types']) for m in molecules]
    assert min(sizes) >= 1 and max(sizes) <= 40 and any(m['dropped'] for m in molecules)


def test_export_declaration_and_tables():
    import __graft_entry__ as g
    from difflinker_amd import _lib, const
    at = _lib.EXPORTS.index('dl_interaction_scores')
    assert _lib.EXPORTS[at + 1:at + 3] == ('dl_add_hydrogens', 'dl_molecule_keys') and _lib.ABI_VERSION == 7
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_add_hydrogens(const dl_hydrogens_args* args);' in header
    assert 'NOT RDKit' in header[header.index('hydrogens.hip'):] and '#define DL_ABI_VERSION 7' in header
    for name, value in (('MAX_ATOMS', 256), ('TOO_LARGE', 4), ('BAD_BOND', 8), ('OVERFLOW', 32), ('NONFINITE', 64)):
        assert re.search(rf'#define DL_HYDRO_{name} {value}\b', header) and getattr(_lib, f'DL_HYDRO_{name}') == value
        assert getattr(hr, name) == value
    assert (_lib.DL_HYDRO_TOO_LARGE, _lib.DL_HYDRO_BAD_BOND, _lib.DL_HYDRO_OVERFLOW, _lib.DL_HYDRO_NONFINITE) == (
        _lib.DL_PHARM_TOO_LARGE, _lib.DL_PHARM_BAD_BOND, _lib.DL_PHARM_OVERFLOW, _lib.DL_PHARM_NONFINITE)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'hydrogens.hip') in g.HIP_SOURCES
    fields = [f[0] for f in _lib.DLHydrogensArgs._fields_]
    struct = header[header.index('typedef struct dl_hydrogens_args {'):header.index('} dl_hydrogens_args;')]
    declared = re.findall(r'(\w+)\s*(?:,|;)', re.sub(r'/\*.*?\*/', '', struct))
    assert declared == fields, 'the ctypes structure lists the header\'s members in order'
    assert fields[-1] == 'stream', 'the entry point takes the structure alone, the stream as its last field'
    assert ctypes.sizeof(_lib.DLHydrogensArgs) == 160   # LP64: 16 + 7 * 8 + 8 + 3 * 8 + 8 + 6 * 8 (an int32 before a pointer is padded)
    for is_geom in (False, True):
        idx2atom = const.GEOM_IDX2ATOM if is_geom else const.IDX2ATOM
        table = const.xh_length_table(is_geom)
        assert table.dtype == torch.float64 and table.tolist() == [hr.XH_LENGTH[idx2atom[k]] for k in range(len(idx2atom))]
        assert const.default_valence_table(is_geom).tolist() == [hr.DEFAULT_VALENCE[idx2atom[k]] for k in range(len(idx2atom))]
    assert const.ATOM2IDX == hr.ATOM2IDX
    g.build()
    assert hasattr(_lib.load(), 'dl_add_hydrogens')


# ---- the SDF writer ----------------------------------------------------------------------------------------------------------
def heavy_batch():
    """Two molecules on the host: propane and, scattered over the rows, methanol."""
    one_hot, x, mask = torch.zeros(2, 5, 8), torch.zeros(2, 5, 3), torch.zeros(2, 5, 1)
    for b, name, rows in ((0, 'propane', [0, 1, 2]), (1, 'methanol', [1, 4])):
        m = hr.hand_molecule(name)
        x[b, rows] = torch.tensor(m['points'], dtype=torch.float32)
        one_hot[b, rows, m['types']] = 1
        mask[b, rows] = 1
    bonds = torch.tensor([[[1, 0, 1], [2, 1, 1], [7, 7, 7]], [[1, 0, 1], [7, 7, 7], [7, 7, 7]]], dtype=torch.int32)
    return one_hot, x, mask, bonds, torch.tensor([2, 1], dtype=torch.int32)


def hand_made_hydrogens():
    from difflinker_amd.molecule_builder import Hydrogens
    parent = torch.tensor([[0, 0, 2, 1], [1, 0, 9, 9]], dtype=torch.int32)
    x = torch.arange(2 * 4 * 3, dtype=torch.float64).reshape(2, 4, 3) / 8 - 1
    return Hydrogens(torch.tensor([4, 2], dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), parent, x,
                     torch.zeros(2, dtype=torch.int32))


def test_sdf_without_hydrogens_is_byte_identical(tmp_path):
    from difflinker_amd.io import save_sdf_file
    one_hot, x, mask, bonds, n_bonds = heavy_batch()
    for name, more in (('old', {}), ('none', {'hydrogens': None})):
        os.makedirs(tmp_path / name)
        save_sdf_file(str(tmp_path / name), one_hot, x, mask, bonds, n_bonds, ['a', 'b'], False, **more)
    for f in ('a_.sdf', 'b_.sdf'):
        assert open(tmp_path / 'old' / f, 'rb').read() == open(tmp_path / 'none' / f, 'rb').read()
    lines = open(tmp_path / 'old' / 'a_.sdf').read().splitlines()
    assert lines[3] == '  3  2  0  0  0  0  0  0  0  0999 V2000' and len(lines) == 4 + 3 + 2 + 2


def test_sdf_with_hydrogens(tmp_path):
    from difflinker_amd.io import read_sdf_molecules, save_sdf_file
    one_hot, x, mask, bonds, n_bonds = heavy_batch()
    hydrogens = hand_made_hydrogens()
    for name, more in (('heavy', {}), ('all', {'hydrogens': hydrogens})):
        os.makedirs(tmp_path / name)
        save_sdf_file(str(tmp_path / name), one_hot, x, mask, bonds, n_bonds, ['a', 'b'], False, **more)
    for f, n, nb, nh in (('a_.sdf', 3, 2, 4), ('b_.sdf', 2, 1, 2)):
        b = 0 if f[0] == 'a' else 1
        heavy, full = (open(tmp_path / d / f).read().splitlines() for d in ('heavy', 'all'))
        assert full[3] == '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (n + nh, nb + nh), 'the counts line holds the totals'
        assert full[:3] == heavy[:3] and full[4:4 + n] == heavy[4:4 + n] and full[-2:] == ['M  END', '$$$$']
        for t in range(nh):
            px, py, pz = hydrogens.x[b, t].tolist()
            assert full[4 + n + t] == '%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (px, py, pz, 'H')
            assert full[4 + n + nh + nb + t] == '%3d%3d%3d  0  0  0  0' % (n + t + 1, int(hydrogens.parent[b, t]) + 1, 1)
        assert full[4 + n + nh:4 + n + nh + nb] == heavy[4 + n:4 + n + nb], 'the heavy bonds come first'
        assert len(full) == 4 + n + nh + nb + nh + 2
        (before,), bad = read_sdf_molecules(str(tmp_path / 'heavy' / f))
        (after,), bad_too = read_sdf_molecules(str(tmp_path / 'all' / f))
        assert bad == bad_too == 0 and after.symbols == before.symbols and after.bonds == before.bonds
        assert np.array_equal(after.positions, before.positions) and after.charges == before.charges


def test_sdf_limits_hold_for_the_totals(tmp_path):
    from difflinker_amd.io import save_sdf_file
    from difflinker_amd.molecule_builder import Hydrogens
    n = 600
    one_hot, x, mask = torch.zeros(1, n, 8), torch.zeros(1, n, 3), torch.ones(1, n, 1)
    one_hot[:, :, 0] = 1
    bonds = torch.tensor([[[k + 1, k, 1] for k in range(n - 1)]], dtype=torch.int32)
    args = (str(tmp_path), one_hot, x, mask, bonds, torch.tensor([n - 1]), ['big'], False)
    save_sdf_file(*args)

    def some(count, status=0, capacity=400):
        return Hydrogens(torch.tensor([count]), torch.zeros(1, n, dtype=torch.int32), torch.zeros(1, capacity, dtype=torch.int32),
                         torch.zeros(1, capacity, 3, dtype=torch.float64), torch.tensor([status]))
    save_sdf_file(*args, hydrogens=some(399))
    assert open(tmp_path / 'big_.sdf').read().splitlines()[3].startswith('999998')
    with pytest.raises(ValueError, match='999'):
        save_sdf_file(*args, hydrogens=some(400))
    with pytest.raises(ValueError, match='hydrogens'):
        save_sdf_file(*args, hydrogens=some(10, status=hr.OVERFLOW))
    with pytest.raises(ValueError, match='hydrogens'):
        save_sdf_file(*args, hydrogens=some(401, capacity=400))


def test_xyz_output_cannot_carry_hydrogens(tmp_path):
    from difflinker_amd import generate as gen
    from difflinker_amd import sample as smp
    calls = ((gen.generate, ('frag.sdf', 'no-such-model.ckpt', str(tmp_path / 'a'), 1, 5, '3')),
             (gen.generate_with_pocket, ('frag.sdf', 'pocket.pdb', False, 'no-such-model.ckpt', str(tmp_path / 'b'), 1, 5, '3')),
             (gen.generate_with_protein, ('frag.sdf', 'protein.pdb', False, 'no-such-model.ckpt', str(tmp_path / 'c'), 1, 5, '3')))
    for function, args in calls:
        with pytest.raises(ValueError, match='hydrogens'):
            function(*args, output_format='xyz', hydrogens=True)
    with pytest.raises(ValueError, match='hydrogens'):
        smp.sample('no-such-model.ckpt', str(tmp_path / 'd'), 'prefix', 1, 'cuda:0', hydrogens=True)
    assert not os.listdir(tmp_path), 'raised before anything was made'


def test_host_tensors_raise():
    from difflinker_amd import _lib
    from difflinker_amd.molecule_builder import Bonds, add_hydrogens
    one_hot, x, mask, bonds, n_bonds = heavy_batch()
    found = Bonds(n_bonds, bonds, None, None, None, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        add_hydrogens(found, one_hot, x, mask, False)
