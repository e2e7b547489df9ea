"""The relaxation rule on the host: the declarations of ``dl_relax_molecules``, the reference ``tests/relax_ref.py`` against
its own stated energy (the force is its gradient), the properties of the rule with the default constants - which the kernel
inherits through bit equality (``tests/test_gpu_relax.py``) - its identities, and the host plumbing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_checks_ref as pr
import relax_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def alone(m, **kwargs):
    """The reference on one unscattered molecule: ``(batch, outputs)``."""
    batch = rr.batch_of([m], len(m['types']), scatter=False)
    return batch, rr.reference(batch, **kwargs)


# ---- declarations --------------------------------------------------------------------------------------------------------------
def test_export_declaration_and_constants():
    import __graft_entry__ as g
    from difflinker_amd import _lib
    at = _lib.EXPORTS.index('dl_interaction_types')
    assert _lib.EXPORTS[at + 1:at + 3] == ('dl_relax_molecules', 'dl_interaction_scores') and _lib.ABI_VERSION == 7
    assert _lib.RELAX_ENTRY_POINTS == {'dl_relax_molecules': _lib.DLRelaxArgs}
    assert 'dl_relax_molecules' not in _lib.STRUCT_ENTRY_POINTS and 'dl_relax_molecules' not in _lib.SELECT_ENTRY_POINTS
    assert _lib.entry_struct('dl_relax_molecules') is _lib.DLRelaxArgs and _lib.entry_struct('dl_pose_checks') is _lib.DLPoseArgs
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_relax_molecules(const dl_relax_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert ' *   dl_relax_molecules ' in header[:header.index('#ifndef DIFFLINKER_HIP_H')], 'listed in the opening comment'
    section = header[header.index('(relax.hip)'):]
    for words in ('NOT UFF', 'NOT MMFF', 'units of its own', 'contraction off', 'five-ring', 'p mod 64', "T'[i] = T[2i] + T[2i+1]",
                  'tests/relax_ref.py', 'plain stores only', 'PRL 97, 170201', 'no hydrogens in the energy', 'frozen'):
        assert words in section, words
    for name, value in (('MAX_ATOMS', 256), ('MAX_STEPS', 1000), ('DIVERGED', 128), ('TERMS', 5)):
        assert re.search(rf'#define DL_RELAX_{name} {value}\b', header) and getattr(_lib, f'DL_RELAX_{name}') == value
    assert (rr.MAX_ATOMS, rr.MAX_STEPS, rr.DIVERGED, rr.TOO_LARGE, rr.BAD_BOND, rr.NONFINITE) == (
        _lib.DL_RELAX_MAX_ATOMS, _lib.DL_RELAX_MAX_STEPS, _lib.DL_RELAX_DIVERGED, _lib.DL_POSE_TOO_LARGE, _lib.DL_POSE_BAD_BOND,
        _lib.DL_POSE_NONFINITE)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'relax.hip') in g.HIP_SOURCES
    struct = header[header.index('typedef struct dl_relax_args {'):header.index('} dl_relax_args;')]
    body = re.sub(r'/\*.*?\*/', '', struct[struct.index('{') + 1:])
    declared, kinds = [], []
    for statement in body.split(';'):
        if not statement.strip():
            continue
        kind = 'pointer' if '*' in statement else statement.split()[0]
        names = re.findall(r'(\w+)\s*(?:,|$)', statement.strip())
        declared += names
        kinds += [kind] * len(names)
    fields = _lib.DLRelaxArgs._fields_
    assert declared == [f[0] for f in fields], 'the ctypes structure lists the header\'s members in order'
    ctype = {'pointer': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    assert [ctype[k] for k in kinds] == [f[1] for f in fields], 'and with the header\'s types'
    assert declared[-1] == 'stream', 'the entry point takes the structure alone, the stream as its last field'
    assert tuple(n for n, k in zip(declared, kinds) if k == 'double') == _lib.RELAX_CONSTANTS
    g.build()
    assert hasattr(_lib.load(), 'dl_relax_molecules') and _lib.load().dl_abi_version() == 7


def test_argument_checks_come_before_device_work():
    from difflinker_amd import _lib
    lib = _lib.load()
    call = lambda a: int(lib.dl_relax_molecules(ctypes.byref(a)))      # noqa: E731
    ok = dict(B=2, N=40, nf=8, capacity=8, steps=10)
    assert int(lib.dl_relax_molecules(None)) == BAD_ARG
    assert call(_lib.DLRelaxArgs(**ok)) == BAD_ARG                   # null pointers
    assert call(_lib.DLRelaxArgs(**dict(ok, capacity=0))) == BAD_ARG  # also when the list may be null
    for wrong in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict(steps=-1), dict(steps=1001)):
        assert call(_lib.DLRelaxArgs(**{**ok, 'B': 0, **wrong})) == BAD_ARG, wrong
    assert call(_lib.DLRelaxArgs(**dict(ok, B=0))) == _lib.DL_OK, 'an empty batch is looked at no further than its sizes'
    assert call(_lib.DLRelaxArgs(**dict(ok, B=0, N=1024, capacity=0, steps=1000))) == _lib.DL_OK


def test_the_tables_against_the_reference_and_hand_values():
    from difflinker_amd import const
    for is_geom, nf in ((False, 8), (True, 9)):
        want = rr.length0(nf), rr.aromatic_length0(nf), list(rr.IDEAL_COS), rr.reach2(nf)
        got = (const.length0_table(is_geom), const.aromatic_length0_table(is_geom), const.ideal_cos_table(),
               const.relax_reach_table(is_geom))
        for g, w, shape in zip(got, want, ((nf, nf, 3), (nf, nf), (3,), (nf, nf))):
            assert g.dtype == torch.float64 and tuple(g.shape) == shape
            assert g.numpy().tobytes() == np.asarray(w, dtype=np.float64).tobytes()
    C, O, N_, S, F = pr.C, pr.O, pr.N_, pr.S, pr.F
    l0, arom = const.length0_table(False), const.aromatic_length0_table(False)
    assert l0[C, C].tolist() == [1.54, 1.34, 1.20] and l0[C, F].tolist() == [1.35, 0.0, 0.0]
    assert [float(arom[a, b]) for a, b in ((C, C), (C, N_), (N_, C), (C, O), (S, C), (N_, N_))] == [1.39, 1.34, 1.34, 1.36, 1.71, 1.35]
    assert float(arom[O, O]) == (1.48 + 1.21) / 2.0, 'no ring value: the mean of single and double'
    assert float(arom[C, F]) == 1.35, 'no double length: the single length'
    assert const.ideal_cos_table().tolist() == [-1.0, -0.5, -1.0 / 3.0]
    assert float(const.relax_reach_table(False)[C, O]) == (0.8 * (1.70 + 1.52)) ** 2
    assert const.RELAX_DEFAULTS == rr.DEFAULTS and const.RELAX_STEPS == 200 and const.AROMATIC_LENGTHS == rr.AROMATIC_LENGTHS
    assert set(const.RELAX_DEFAULTS) == set(__import__('difflinker_amd')._lib.RELAX_CONSTANTS) | {'n_min'}


# ---- the force is the gradient of the stated energy ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['walled', 'kekule_benzene', 'folded_linker'])
def test_the_force_is_the_gradient_of_the_energy(name):
    """Central differences at h = 1e-5 against the reference forces, to 1e-6 * (1 + |F|): two orders above the truncation
    (h^2 k, about 1e-8) and the round-off (eps E / h, about 2e-9), so only a wrong sign, factor or missing term shows."""
    mol = rr.engine(getattr(rr, name)())
    x = mol.x0 + np.random.default_rng(3).normal(0.0, 0.05, mol.x0.shape) * mol.mov[:, None]      # off the restraint's minimum
    F, h = mol.forces(x), 1e-5
    if name == 'walled':
        terms = mol.energies(x)
        assert all(terms[t] > 0.0 for t in (rr.BOND, rr.ANGLE, rr.WALL, rr.RESTRAINT)), 'every term but the repulsion is live'
        assert any(mol.adj[a] and len(mol.adj[a]) == 2 for a in range(mol.K))
    if name == 'folded_linker':
        assert mol.energies(x)[rr.REPULSION] > 0.0
    assert not F[~mol.mov].any() and np.abs(F).max() > 1.0
    for u in mol.M:
        for d in range(3):
            up, down = x.copy(), x.copy()
            up[u, d] += h
            down[u, d] -= h
            slope = -(sum(mol.energies(up)) - sum(mol.energies(down))) / (2 * h)
            assert abs(slope - F[u, d]) <= 1e-6 * (1 + abs(F[u, d])), (u, d, slope, F[u, d])


# ---- properties with the default constants -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['perturbed_chain', 'folded_linker'])
def test_a_bad_linker_comes_back_clean(name):
    m = getattr(rr, name)()
    batch, out = alone(m)
    before, _ = rr.pose_of(m, batch['x'][0])
    after, flags = rr.pose_of(m, out['x_out'][0])
    bad = lambda counts: sum(counts[1][k] for k in (pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES))      # noqa: E731
    assert bad(before) > 0 and bad(after) == 0 and not any(flags[k] for k in m['marked']) and out['status'][0] == 0
    assert out['energy'][0, 1].sum() < out['energy'][0, 0].sum()
    assert 0.0 < out['moved2'][0] <= (200 * rr.DEFAULTS['max_step']) ** 2
    if name == 'perturbed_chain':
        x = out['x_out'][0].astype(np.float64)
        lengths = [np.linalg.norm(x[k + 1] - x[k]) for k in range(2, 9)]
        assert max(abs(v - 1.54) for v in lengths) < 0.02, lengths


def test_a_linker_atom_inside_the_wall_is_pushed_out():
    from difflinker_amd.const import VDW_RADII
    m = rr.walled()
    batch, out = alone(m)
    _, free = alone(m, use_wall=False)
    assert out['energy'][0, 0, rr.WALL] > 0.0 and not free['energy'][0, :, rr.WALL].any()

    def closest(x):                                  # the smallest distance over 0.75 x the radii sum, linker against pocket
        return min(np.linalg.norm(x[a].astype(np.float64) - x[w]) / (0.75 * (VDW_RADII[m['types'][a]] + VDW_RADII[m['types'][w]]))
                   for a in m['marked'] for w in m['dropped'])
    assert closest(batch['x'][0]) < 1.0 < closest(out['x_out'][0])
    assert np.array_equal(out['x_out'][0, m['dropped']], batch['x'][0, m['dropped']]), 'the wall itself stays'


def test_a_kekule_benzene_keeps_six_equal_bonds():
    m = rr.kekule_benzene()
    batch, out = alone(m)
    ring = lambda x: [float(np.linalg.norm(x[(k + 1) % 6].astype(np.float64) - x[k])) for k in range(6)]      # noqa: E731
    assert max(ring(batch['x'][0])) - min(ring(batch['x'][0])) > 0.1
    assert max(ring(out['x_out'][0])) - min(ring(out['x_out'][0])) < 0.03
    unflagged = dict(m, aromatic=[], planar=[])
    _, pulled = alone(unflagged)
    assert max(ring(pulled['x_out'][0])) - min(ring(pulled['x_out'][0])) > 0.1, 'without the flags the orders pull it apart'
    assert out['steps_done'][0] < 200 and out['f_max'][0] < rr.DEFAULTS['f_tol'], 'stopped on f_tol'


# ---- identities ------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return all(a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes() for name in rr.FIELDS)


def test_nothing_movable_or_no_steps_gives_x_back():
    rng = np.random.default_rng(11)
    molecules = [rr.random_molecule(rng, max_atoms=25, min_atoms=4) for _ in range(6)]
    batch = rr.batch_of(molecules, 32, seed=2, aromatic='random')
    out = rr.reference(batch, steps=0)
    assert out['x_out'].tobytes() == batch['x'].tobytes() and not out['steps_done'].any() and not out['f_max'].any()
    assert np.array_equal(out['energy'][:, 0], out['energy'][:, 1]) and out['energy'].any()
    nothing = dict(batch, mark_mask=np.zeros_like(batch['mark_mask']))
    out = rr.reference(nothing, steps=20)
    assert out['x_out'].tobytes() == batch['x'].tobytes() and not out['steps_done'].any() and not out['energy'].any()


def test_fixed_dropped_and_padding_rows_stay_bit_for_bit():
    rng = np.random.default_rng(12)
    molecules = [rr.random_molecule(rng, max_atoms=25, min_atoms=4) for _ in range(8)]
    batch = rr.batch_of(molecules, 32, seed=3, aromatic='random')
    out = rr.reference(batch, steps=10)
    movable = (batch['node_mask'] != 0) & (batch['drop_mask'] == 0) & (batch['mark_mask'] != 0)
    bits = lambda a: a.view(np.uint32)                                # noqa: E731
    assert np.array_equal(bits(out['x_out'])[~movable], bits(batch['x'])[~movable])
    assert (bits(out['x_out'])[movable] != bits(batch['x'])[movable]).any() and out['steps_done'].max() == 10


def test_invariance_under_list_order_and_orientation():
    rng = np.random.default_rng(13)
    molecules = [rr.random_molecule(rng, max_atoms=25, min_atoms=6) for _ in range(6)]
    for m in molecules:
        m['aromatic'] = [e for e in range(len(m['entries'])) if rng.random() < 0.3]
    base = rr.reference(rr.batch_of(molecules, 32, seed=4), steps=8)
    shuffled = []
    for m in molecules:
        order = rng.permutation(len(m['entries']))
        entries = [m['entries'][e] if rng.random() < 0.5 else (m['entries'][e][1], m['entries'][e][0], m['entries'][e][2]) for e in order]
        shuffled.append(dict(m, entries=entries, aromatic=[k for k, e in enumerate(order) if e in m['aromatic']]))
    assert same_bits(base, rr.reference(rr.batch_of(shuffled, 32, seed=4), steps=8))


def test_coincident_atoms_and_zero_length_arms_give_no_nan():
    points = [(0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (1.5, 0.0, 0.0), (3.0, 0.2, 0.0), (1.5, 0.0, 0.0)]
    m = rr.molecule_of([pr.C] * 5, points, [(1, 0, 1), (2, 1, 1), (3, 2, 1)], [1, 2, 3, 4])
    mol = rr.engine(m)
    assert np.isfinite(mol.forces(mol.x0)).all() and np.isfinite(mol.energies(mol.x0)).all()
    _, out = alone(m, steps=5)
    assert out['status'][0] == 0 and np.isfinite(out['x_out']).all() and np.isfinite(out['energy']).all()


def test_limits_and_bad_inputs():
    m = rr.perturbed_chain()
    batch = rr.batch_of([m, m, m, m], 16, seed=5, status=[0, 16, 0, 2])
    batch['x'][1, np.flatnonzero(batch['node_mask'][1])[4], 1] = np.inf
    batch['bonds'][2, 3] = (5, 5, 1)
    batch['n_bonds_in'][3] = 99
    out = rr.reference(batch, steps=6)
    assert out['status'].tolist() == [0, 16 | rr.NONFINITE, rr.BAD_BOND, 2 | rr.BONDS_OVERFLOW]
    assert out['x_out'][1].tobytes() == batch['x'][1].tobytes() and not out['energy'][1].any() and out['steps_done'][1] == 0
    assert out['steps_done'][[0, 2, 3]].tolist() == [6, 6, 6]
    big = rr.molecule_of([pr.C] * 257, [(1.3 * k, 0.0, 0.0) for k in range(257)], pr.chain_bonds(257), range(257))
    out = rr.reference(rr.batch_of([big], 257, scatter=False), steps=2)
    assert out['status'][0] == rr.TOO_LARGE and not out['energy'].any()
    out = rr.reference(rr.batch_of([m], 12, scatter=False), steps=30, dt0=1e200, dt_max=1e300, max_step=1e300)
    assert out['status'][0] == rr.DIVERGED and out['energy'][0, 0].any() and not out['energy'][0, 1].any()
    assert out['x_out'].tobytes() == rr.batch_of([m], 12, scatter=False)['x'].tobytes()


# ---- host plumbing ---------------------------------------------------------------------------------------------------------------
def test_compute_relaxation_on_hand_records():
    from difflinker_amd.metrics import RelaxRecord, compute_relaxation
    records = [RelaxRecord((4.0, 2.0, 1.0, 1.0, 0.0), (1.0, 0.5, 0.25, 0.25, 3.0), 50, 5e-4, 0.5, 0, False, True),
               RelaxRecord((8.0, 0.0, 0.0, 0.0, 0.0), (2.0, 0.0, 0.0, 0.0, 1.0), 200, 0.5, 1.0, 0, True, False),
               RelaxRecord((0.0,) * 5, (0.0,) * 5, 0, 0.0, 0.0, 64, False, False)]
    out = compute_relaxation(records)
    assert out == {'relax_molecules': 2, 'relax_energy_before': 8.0, 'relax_energy_after': 2.0, 'relax_displacement_mean': 0.75,
                   'relax_displacement_max': 1.0, 'relax_converged': 0.5, 'relax_bonds_changed': 0.5}
    empty = compute_relaxation([])
    assert empty['relax_molecules'] == 0 and empty['relax_energy_before'] is None and empty['relax_bonds_changed'] is None


def test_python_callers_refuse_the_cpu_and_bad_arguments():
    from difflinker_amd import _lib, molecule_builder as mb
    one_hot, x, mask = torch.zeros(1, 4, 8), torch.zeros(1, 4, 3), torch.ones(1, 4)
    found = mb.Bonds(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 3, dtype=torch.int32), None, None, None, None)
    with pytest.raises(_lib.HipLibraryError, match='HIP device only'):
        mb.relax(found, one_hot, x, mask, False, mask)
    with pytest.raises(_lib.HipLibraryError, match='HIP device only'):
        mb.relax_samples(one_hot, x, mask, False, mask)
    with pytest.raises(TypeError, match='unknown constants'):
        mb.relax(found, one_hot, x, mask, False, mask, k_torsion=1.0)
    for steps in (-1, 1001):
        with pytest.raises(ValueError, match='steps must be'):
            mb.relax(found, one_hot, x, mask, False, mask, steps=steps)


def test_command_lines_keep_their_defaults(monkeypatch):
    """Without ``--relax`` the drivers are called exactly as before; with it the keyword carries the step count."""
    import inspect
    from difflinker_amd import generate as gen, sample as smp, train
    for function in (gen.generate, gen.generate_with_pocket, gen.generate_with_protein, gen._sample_and_save, smp.sample):
        assert inspect.signature(function).parameters['relax'].default is None
    seen = {}
    for name in ('generate', 'generate_with_pocket', 'generate_with_protein'):
        monkeypatch.setattr(gen, name, lambda *a, **k: seen.update(k) or [])
    base = ['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3']
    for more in ([], ['--pocket', 'p.pdb'], ['--protein', 'p.pdb']):
        seen.clear()
        gen.main(base + more)
        assert 'relax' not in seen
        gen.main(base + more + ['--relax'])
        assert seen['relax'] == 200
        gen.main(base + more + ['--relax', '50'])
        assert seen['relax'] == 50
    seen.clear()
    monkeypatch.setattr(smp, 'sample', lambda *a, **k: seen.update(k) or 'out')
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p'])
    assert 'relax' not in seen
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p', '--relax', '7'])
    assert seen['relax'] == 7
    assert '--relax' not in inspect.getsource(train.main), 'not in train'
