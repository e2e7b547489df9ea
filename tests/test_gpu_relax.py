"""The relaxation on the GPU (``dl_relax_molecules``, ``csrc/relax.hip``) against the numpy rule of ``tests/relax_ref.py``.  The C
entry point is called on outputs pre-filled with 0x5a bytes, so an element it should write and does not shows, and EVERY output
byte is compared with the reference: both sides round every fp64 operation once and sum in the order the header states, so there
is no tolerance anywhere in this file.  The public path (``relax``, ``relax_samples``, ``relax_to_host``, the drivers) comes
last; the launch on a side stream is in ``tests/test_gpu_streams_relax.py``, collected after the stream harness it uses."""
import ctypes

import numpy as np
import pytest
import torch

import input_forms as IF
import pose_checks_ref as pr
import relax_ref as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'x_out': torch.float32, 'energy': torch.float64, 'steps_done': torch.int32, 'f_max': torch.float64,
          'moved2': torch.float64, 'status': torch.int32}
ALL, NONE = dict(zip(rr.OPTIONAL, (True,) * 5)), dict(zip(rr.OPTIONAL, (False,) * 5))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def launch(batch, tables=None, steps=200, use_wall=True, drop=True, mark=True, planar=True, status=True, aromatic=True, stream=None,
           **constants):
    """The C entry point on outputs full of 0x5a bytes: a dict of numpy arrays by the names of ``relax_ref.FIELDS``."""
    from difflinker_amd import _lib
    B, N = batch['node_mask'].shape
    nf, capacity = batch['one_hot'].shape[2], batch['bonds'].shape[1]
    tables = tables or rr.default_tables(nf)
    held = [dev(batch['x']), dev(batch['one_hot']), dev(batch['node_mask']), dev(batch['drop_mask']), dev(batch['mark_mask']),
            dev(batch['atom_planar'], torch.int32), dev(batch['n_bonds_in'], torch.int32), dev(batch['bonds'], torch.int32),
            dev(batch['bond_aromatic'], torch.int32), dev(batch['status_in'], torch.int32)] + [dev(t, torch.float64) for t in tables]
    x, one_hot, mask, drop_t, mark_t, planar_t, n_in, bonds, flags, status_in, l0, arom0, ideal, reach, wall_reach = held
    assert l0.shape == (nf, nf, 3) and arom0.shape == reach.shape == wall_reach.shape == (nf, nf) and ideal.shape == (3,)
    shapes = {'x_out': (B, N, 3), 'energy': (B, 2, 5)}
    out = {name: torch.empty(shapes.get(name, (B,)), dtype=DTYPES[name], device=DEV) for name in rr.FIELDS}
    for t in out.values():
        t.view(torch.uint8).fill_(0x5a)
    values = dict(rr.DEFAULTS, **constants)
    args = _lib.DLRelaxArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
        drop_mask=drop_t.data_ptr() if drop else None, mark_mask=mark_t.data_ptr() if mark else None,
        atom_planar=planar_t.data_ptr() if planar else None, length0=l0.data_ptr(), aromatic_length0=arom0.data_ptr(),
        ideal_cos=ideal.data_ptr(), reach2=reach.data_ptr(), wall_reach2=wall_reach.data_ptr(), capacity=capacity,
        n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr() if bonds.numel() else None,
        bond_aromatic=flags.data_ptr() if aromatic and flags.numel() else None, status_in=status_in.data_ptr() if status else None,
        use_wall=int(use_wall), steps=steps, n_min=values['n_min'], x_out=out['x_out'].data_ptr(), energy=out['energy'].data_ptr(),
        steps_done=out['steps_done'].data_ptr(), f_max=out['f_max'].data_ptr(), moved2=out['moved2'].data_ptr(),
        status=out['status'].data_ptr(), **{name: float(values[name]) for name in _lib.RELAX_CONSTANTS})
    args.stream = (torch.cuda.current_stream(torch.device(DEV)) if stream is None else stream).cuda_stream
    _lib.check(_lib.load().dl_relax_molecules(ctypes.byref(args)), 'dl_relax_molecules')
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def same_bits(a, b):
    return all(a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes() for name in rr.FIELDS)


def compare(got, want):
    for name in rr.FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        if got[name].tobytes() != want[name].tobytes():
            g, w = (a.view(np.uint32 if a.itemsize == 4 else np.uint64) for a in (got[name], want[name]))
            where = np.argwhere(g != w)
            raise AssertionError((name, len(where), where[:5].tolist(), got[name][g != w][:5], want[name][g != w][:5]))
    return got


def check(batch, tables=None, **kwargs):
    return compare(launch(batch, tables, **kwargs), rr.reference(batch, tables, **kwargs))


def row(batch, b):
    return {key: value[b:b + 1] for key, value in batch.items()}


EMPTY = rr.molecule_of([], [], [], [])
OWN = ('perturbed_chain', 'folded_linker', 'kekule_benzene', 'walled')


def hand_molecules():
    return [dict(pr.hand_molecule(name), marked=list(range(1, len(pr.HAND[name][0])))) for name in sorted(pr.HAND)] + \
        [getattr(rr, name)() for name in OWN] + [EMPTY]


@pytest.fixture(scope='module')
def random_batch():
    rng = np.random.default_rng(31)
    molecules = [rr.random_molecule(rng) for _ in range(200)]
    return rr.batch_of(molecules, 64, seed=32, status=rng.choice([0, 0, 2, 16], 200), aromatic='random')


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [0, 1, 2, 7, 40])
def test_hand_molecules(steps):
    """7 steps cross n_min; 40 see dt grow, a P <= 0 reset and, for the benzene, the f_tol exit."""
    batch = rr.batch_of(hand_molecules(), 12, seed=1)
    got = check(batch, steps=steps)
    assert got['steps_done'].max() == steps and not got['status'].any()
    assert got['steps_done'][-1] == 0 and not got['energy'][-1].any(), 'the molecule with no real row'
    if steps == 40:
        butane = sorted(pr.HAND).index('butane')
        assert got['steps_done'][butane] < 40 and got['f_max'][butane] < rr.DEFAULTS['f_tol'], 'an ideal chain stops on f_tol'
        assert (got['energy'][-5:-1, 1].sum(1) < got['energy'][-5:-1, 0].sum(1)).all()
    if steps == 0:
        assert got['x_out'].tobytes() == batch['x'].tobytes()


@pytest.mark.parametrize('use_wall', [True, False])
@pytest.mark.parametrize('options', [ALL, NONE], ids=['all', 'null'])
def test_random_molecules(random_batch, options, use_wall):
    got = check(random_batch, steps=25, use_wall=use_wall, **options)
    assert got['steps_done'].max() == 25 and (got['status'] & rr.BAD_BOND).sum() == 0
    if options is ALL:
        assert got['energy'][:, 0, :4].any(axis=0).tolist() == [True, True, True, use_wall]
        movable = (random_batch['node_mask'] != 0) & (random_batch['drop_mask'] == 0) & (random_batch['mark_mask'] != 0)
        assert np.array_equal(got['x_out'].view(np.uint32)[~movable], random_batch['x'].view(np.uint32)[~movable])


# ---- the edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_movable', [0, 1, 4, 5])
def test_movable_atoms_on_both_sides_of_the_four_waves(n_movable):
    m = dict(rr.perturbed_chain(), marked=list(range(3, 3 + n_movable)))
    got = check(rr.batch_of([m, rr.folded_linker()], 14, seed=n_movable), steps=12)
    assert got['steps_done'][0] == (12 if n_movable else 0)


@pytest.mark.parametrize('n_wall', [0, 1, 63, 64, 65, 130])
def test_wall_atoms_on_both_sides_of_the_64_partials(n_wall):
    rng = np.random.default_rng(n_wall)
    chain = rr.perturbed_chain(8)
    wall = rng.normal(0.0, 1.0, (n_wall, 3)) * (4.0, 2.0, 2.0) + (4.0, 0.5, 0.0)
    m = rr.molecule_of([pr.C] * 8 + [int(t) for t in rng.choice([pr.C, pr.N_, pr.O, pr.S], n_wall)], list(chain['points']) + wall.tolist(),
                       chain['entries'], range(1, 7), dropped=range(8, 8 + n_wall))
    got = check(rr.batch_of([m], 160, seed=n_wall), steps=6)
    assert got['energy'][0, 0, rr.WALL] > 0.0 if n_wall >= 63 else n_wall == 1 or got['energy'][0, 0, rr.WALL] == 0.0


def folded(n):
    m = pr.chain(n)
    return rr.molecule_of(m['types'], m['points'], m['entries'], range(n))


def test_256_atoms_all_movable_and_257():
    got = check(rr.batch_of([folded(256), folded(257), folded(255)], 257, scatter=False), steps=3)
    assert got['status'].tolist() == [0, rr.TOO_LARGE, 0] and got['steps_done'].tolist() == [3, 0, 3]
    assert got['energy'][0, 0, rr.REPULSION] > 0.0 and not got['energy'][1].any()


def test_1024_rows_with_700_wall_rows():
    rng = np.random.default_rng(9)
    m = pr.chain(200)
    wall = np.asarray(m['points'])[rng.integers(0, 200, 700)] + rng.normal(0.0, 1.0, (700, 3)) * (0.5, 0.5, 2.5)
    m = rr.molecule_of(m['types'] + [pr.C, pr.O] * 350, list(m['points']) + wall.tolist(), m['entries'], range(60, 110),
                       dropped=range(200, 900))
    got = check(rr.batch_of([m, rr.walled()], 1024, seed=10), steps=3)
    assert got['energy'][0, 0, rr.WALL] > 0.0 and got['status'].tolist() == [0, 0]


def test_coincident_atoms_the_clamp_and_a_diverging_start():
    points = [(0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (1.5, 0.0, 0.0), (3.0, 0.2, 0.0), (1.5, 0.0, 0.0)]
    twin = rr.molecule_of([pr.C] * 5, points, [(1, 0, 1), (2, 1, 1), (3, 2, 1)], [1, 2, 3, 4])
    close = rr.molecule_of([pr.C, pr.C, pr.O], [(0.0, 0.0, 0.0), (0.01, 0.0, 0.0), (1.2, 0.9, 0.0)], [(1, 0, 1), (2, 1, 1)], [1, 2])
    got = check(rr.batch_of([twin, close], 6, seed=2), steps=1, k_bond=5000.0)
    assert abs(float(np.sqrt(got['moved2'][1])) - rr.DEFAULTS['max_step']) < 1e-12, 'the first step hit the clamp'
    assert not got['status'].any() and np.isfinite(got['energy']).all()
    got = check(rr.batch_of([twin, close, rr.perturbed_chain()], 12, seed=3), steps=30, dt0=1e200, dt_max=1e300, max_step=1e300)
    assert got['status'].tolist() == [rr.DIVERGED] * 3 and got['energy'][:, 0].any() and not got['energy'][:, 1].any()


def test_geom_vocabulary_and_an_empty_batch():
    rng = np.random.default_rng(14)
    molecules = [rr.random_molecule(rng, max_atoms=20, min_atoms=3) for _ in range(10)]
    for m in molecules:
        m['types'] = [int(t) for t in rng.integers(0, 9, len(m['types']))]
    got = check(rr.batch_of(molecules, 24, seed=15, nf=9, aromatic='random'), steps=5)
    assert got['steps_done'].max() == 5
    empty = rr.batch_of([], 8)
    empty['node_mask'] = empty['node_mask'].reshape(0, 8)
    got = launch(empty)
    assert all(got[name].shape[0] == 0 for name in rr.FIELDS)


def test_bad_arguments():
    from difflinker_amd import _lib
    lib = _lib.load()
    ok = dict(B=0, N=40, nf=8, capacity=8, steps=10)
    for wrong in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict(steps=-1), dict(steps=1001), dict(B=1)):
        assert int(lib.dl_relax_molecules(ctypes.byref(_lib.DLRelaxArgs(**{**ok, **wrong})))) == -1, wrong
    assert int(lib.dl_relax_molecules(None)) == -1 and int(lib.dl_relax_molecules(ctypes.byref(_lib.DLRelaxArgs(**ok)))) == 0


# ---- reproducibility and independence ------------------------------------------------------------------------------------------------
def test_the_same_launch_twice_and_every_molecule_alone(random_batch):
    some = {key: value[:24] for key, value in random_batch.items()}
    first = launch(some, steps=10)
    assert same_bits(first, launch(some, steps=10))
    for b in range(24):
        single = launch(row(some, b), steps=10)
        assert all(single[name].tobytes() == first[name][b:b + 1].tobytes() for name in rr.FIELDS), b


# ---- the public path -----------------------------------------------------------------------------------------------------------------
def public(batch, place=dev, **kwargs):
    from difflinker_amd.molecule_builder import Bonds, relax
    found = Bonds(place(batch['n_bonds_in'], torch.int32), place(batch['bonds'], torch.int32), None, None, None,
                  place(batch['status_in'], torch.int32))
    return relax(found, place(batch['one_hot']), place(batch['x']), place(batch['node_mask']), False, place(batch['mark_mask']),
                 drop_mask=place(batch['drop_mask']), atom_planar=place(batch['atom_planar'], torch.int32),
                 bond_aromatic=place(batch['bond_aromatic'], torch.int32), **kwargs)


def test_relax_and_its_records(random_batch):
    from difflinker_amd import metrics
    from difflinker_amd.molecule_builder import perceive_bonds
    some = {key: value[:40] for key, value in random_batch.items()}
    result = public(some, steps=25)
    want = rr.reference(some, steps=25)
    got = dict(zip(rr.FIELDS, (t.cpu().numpy() for t in result)))
    compare(got, want)
    result = public(some, steps=9, k_bond=80.0, f_tol=1e-2, use_wall=False)
    compare(dict(zip(rr.FIELDS, (t.cpu().numpy() for t in result))), rr.reference(some, steps=9, k_bond=80.0, f_tol=1e-2, use_wall=False))
    one_hot, mask = dev(some['one_hot']), dev(some['node_mask'])
    raw, relaxed = perceive_bonds(one_hot, dev(some['x']), mask, False), perceive_bonds(one_hot, result.x, mask, False)
    records = metrics.relax_to_host(result, raw, relaxed)
    assert [r.status for r in records] == want['status'].tolist()
    changed = [r.bonds_changed for r in records]
    assert all(isinstance(c, bool) for c in changed) and any(changed)
    same = metrics.relax_to_host(result, raw, raw)
    assert not any(r.bonds_changed for r in same)
    scores = metrics.compute_relaxation(records)
    assert set(scores) == set(metrics.RELAX_NAMES) and scores['relax_molecules'] == sum(r.status == 0 for r in records)
    assert scores['relax_energy_after'] < scores['relax_energy_before'] and 0.0 < scores['relax_bonds_changed'] <= 1.0


def samples_batch():
    """Linkers in need of a clean-up between fragments, as the sampler leaves them: plain tensors on the host."""
    molecules = [rr.perturbed_chain(12, seed=s) for s in range(6)] + [rr.kekule_benzene(), rr.folded_linker(), rr.walled()]
    batch = rr.batch_of(molecules, 14, seed=7)
    return {k: torch.as_tensor(batch[k]) for k in ('one_hot', 'x', 'node_mask', 'mark_mask', 'drop_mask')}


def run_samples(place):
    from difflinker_amd.molecule_builder import relax_samples
    h = samples_batch()
    return relax_samples(place(h['one_hot']), place(h['x']), place(h['node_mask']), False, place(h['mark_mask']),
                         drop_mask=place(h['drop_mask']), steps=60)


def test_relax_samples_cleans_linkers_up():
    from difflinker_amd import metrics
    h = samples_batch()
    result = run_samples(lambda t: t.to(DEV))
    linker = h['mark_mask'].to(DEV)
    before = metrics.analyze_pose_checks(h['one_hot'].to(DEV), h['x'].to(DEV), h['node_mask'].to(DEV), False, linker, h['drop_mask'].to(DEV))
    after = metrics.analyze_pose_checks(h['one_hot'].to(DEV), result.x, h['node_mask'].to(DEV), False, linker, h['drop_mask'].to(DEV))
    bad = lambda counts: int(counts[:, 1, [pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES]].sum())      # noqa: E731
    assert bad(before.counts) > 5 and bad(after.counts) < bad(before.counts) and not result.status.any()
    fixed = (h['mark_mask'] == 0) | (h['node_mask'] == 0) | (h['drop_mask'] != 0)
    assert torch.equal(result.x.cpu().view(torch.int32)[fixed], h['x'].view(torch.int32)[fixed])
    energy = result.energy.cpu()
    assert (energy[:, 1, :4].sum(1) < energy[:, 0, :4].sum(1)).all()


@pytest.mark.parametrize('form', ['strided', 'sliced', 'wide'])
def test_input_forms_of_relax_samples(form):
    """The result is a function of the values alone - not of strides, storage offsets or (exact) dtypes - and no input is
    written to, in the manner of ``tests/test_gpu_input_forms.py``."""
    base = run_samples(lambda t: IF.canonical(t, DEV))
    placed = []

    def place(t):
        out = IF.BY_NAME[form](t, DEV)
        placed.append((IF.buffer_of(out), IF.as_bytes(IF.buffer_of(out)).clone()))
        return out
    got = run_samples(place)
    for name in base._fields:
        a, b = getattr(base, name), getattr(got, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(IF.as_bytes(a.contiguous()), IF.as_bytes(b.contiguous())), name
    for buf, copy in placed:
        assert torch.equal(IF.as_bytes(buf), copy), 'an input was written to'


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def crowded_schedule():
    """A noise schedule that ends at alpha_T^2 = 0.4 (the polynomial schedule needs less than 0.5): the untrained denoiser of
    the driver tests then leaves the linker atoms within an Angstrom or two of the fragments' centre, crowded together - a
    linker in need of a clean-up (with the schedules the other driver tests use the linker atoms end tens of Angstrom apart,
    and nothing acts on them)."""
    from difflinker_amd.noise import PredefinedNoiseSchedule
    return PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=0.4)


def xyz_rows(text):
    return [line.split() for line in text.strip().splitlines()[2:]]


def test_generate_with_relax(tmp_path):
    import json
    import os
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import POSE_NAMES, RELAX_NAMES, RELAX_TERMS
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    ddpm.edm.gamma = crowded_schedule()
    frag = os.path.join(IO_DIR, 'frag.sdf')
    runs = {'plain': dict(metrics=True), 'relaxed': dict(metrics=True, relax=30), 'both': dict(metrics=True, relax=30, pose_checks=True),
            'alone': dict(relax=30), 'bare': {}}
    files = {}
    for name, more in runs.items():
        torch.manual_seed(11)
        written = generate(frag, ddpm, str(tmp_path / name), n_samples=3, n_steps=5, linker_size='4', output_format='both', **more)
        files[name] = {os.path.basename(path): open(path).read() for path in written}
    assert files['plain'] == files['bare'] and files['relaxed'] == files['both'] == files['alone']
    assert not os.path.exists(tmp_path / 'plain' / 'relax.json') and not os.path.exists(tmp_path / 'bare' / 'metrics.json')
    before, got, both = (json.load(open(tmp_path / name / 'metrics.json')) for name in ('plain', 'relaxed', 'both'))
    assert set(got) == set(before) | set(RELAX_NAMES) and before == {k: got[k] for k in before}, 'every other score is the raw sample\'s'
    assert set(both) == set(got) | set(POSE_NAMES) | {k + '_relaxed' for k in POSE_NAMES}
    assert json.load(open(tmp_path / 'alone' / 'metrics.json')) == {k: got[k] for k in RELAX_NAMES}
    records = json.load(open(tmp_path / 'relaxed' / 'relax.json'))
    assert sorted(records) == sorted(files['relaxed']) and len(records) == 6
    for record in records.values():
        assert list(record) == ['energy_before', 'energy_after', 'steps_done', 'f_max', 'displacement', 'status', 'bonds_changed', 'converged']
        assert list(record['energy_before']) == list(RELAX_TERMS) and record['steps_done'] <= 30
    moved = 0
    for name, text in files['relaxed'].items():
        if not name.endswith('.xyz'):
            continue
        raw, new = xyz_rows(files['plain'][name]), xyz_rows(text)
        assert [r[0] for r in raw] == [r[0] for r in new]
        same = [a == b for a, b in zip(raw, new)]
        assert sum(not s for s in same) <= 4, 'at most the four linker atoms differ'
        assert all(same[:len(raw) - 4]), 'the fragment coordinates are unchanged'
        moved += sum(not s for s in same)
    assert moved > 0 and got['relax_molecules'] == 3 and got['relax_displacement_max'] > 0.0


def test_sample_with_relax(tmp_path):
    import json
    import os
    from difflinker_amd.metrics import METRIC_NAMES, POSE_NAMES, RELAX_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_rings import gentle_model
    m = gentle_model(tmp_path, False)
    m.edm.gamma = crowded_schedule().to(DEV)
    m.edm.noise_seed = 5
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    m.edm.noise_seed = 5
    out = sample(m, str(tmp_path / 'new'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, relax=20,
                 pose_checks=True)
    before, got = (json.load(open(os.path.join(d, 'metrics.json'))) for d in (plain, out))
    true_keys = {'true_' + k for k in POSE_NAMES}
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | set(RELAX_NAMES) | set(POSE_NAMES) | true_keys | {k + '_relaxed' for k in POSE_NAMES}
    assert before == {k: got[k] for k in before}, 'every other score is the raw sample\'s'
    records = json.load(open(os.path.join(out, 'relax.json')))
    assert not os.path.exists(os.path.join(plain, 'relax.json')) and records
    differ = 0
    for name in records:
        assert name.endswith('_.xyz') and os.path.exists(os.path.join(out, name))
        raw, new = (xyz_rows(open(os.path.join(d, name)).read()) for d in (plain, out))
        assert len(raw) == len(new)
        differ += raw != new
        uuid = name.split('/')[0]
        frag = xyz_rows(open(os.path.join(out, uuid, 'frag_.xyz')).read())
        assert sum(a != b for a, b in zip(raw, new)) <= len(new) - len(frag), 'only linker atoms moved'
    assert differ > 0 and got['relax_molecules'] == len(records)


def test_generate_with_pocket_and_relax(tmp_path):
    """The pocket variant: the pocket rows of the batch are the wall, the files hold no pocket atom, and the clash scores
    against the pocket stay the raw sample's."""
    import json
    import os
    import test_gpu_clash as TC
    from difflinker_amd import DDPM, io
    from difflinker_amd.generate import generate_with_pocket
    from difflinker_amd.metrics import RELAX_NAMES
    from test_gpu_generate import ddpm_hparams
    sdf = os.path.join(TC.CASES, 'jnk_fragments.sdf')
    frag = io.read_molecule(sdf)
    pocket = TC.pocket_file(tmp_path, os.path.join(TC.CASES, 'jnk_protein_12A.pdb'), frag.positions)
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(True))
    ddpm.edm.gamma = crowded_schedule()
    kw = dict(backbone_atoms_only=False, model=ddpm, n_samples=3, n_steps=5, linker_size='5', random_seed=3, clashes=True)
    plain = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'plain'), **kw)
    relaxed = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'relaxed'), relax=25, **kw)
    before, got = (json.load(open(tmp_path / name / 'metrics.json')) for name in ('plain', 'relaxed'))
    assert set(got) == set(before) | set(RELAX_NAMES) and before == {k: got[k] for k in before}
    assert json.load(open(tmp_path / 'plain' / 'clashes.json')) == json.load(open(tmp_path / 'relaxed' / 'clashes.json'))
    records = json.load(open(tmp_path / 'relaxed' / 'relax.json'))
    assert sorted(records) == sorted(os.path.basename(f) for f in relaxed) and len(records) == 3
    assert all(r['status'] == 0 and r['steps_done'] <= 25 for r in records.values()) and any(r['displacement'] > 0 for r in records.values())
    for a, b in zip(plain, relaxed):
        raw, new = xyz_rows(open(a).read()), xyz_rows(open(b).read())
        assert len(raw) == len(new) == len(frag) + 5 and raw[:len(frag)] == new[:len(frag)], 'the fragments stay'
