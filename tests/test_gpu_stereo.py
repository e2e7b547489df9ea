"""Stereo perception on the GPU (``dl_stereo_perceive``, ``csrc/stereo.hip``) against the plain-Python rule of
``tests/stereo_ref.py``.  The C entry point is called on outputs pre-filled with 0x5a bytes, so an element it should write and
does not shows, and EVERY output byte is compared with the restatement: the outputs are integers decided by fp64 comparisons
that both sides round identically, so there is no tolerance anywhere in this file.  The Python layer (``metrics.stereo``,
``metrics.stereo_codes``) comes last; the launches on side streams are in ``tests/test_gpu_streams_stereo.py``, collected after
the stream harness they use."""
import ctypes

import numpy as np
import pytest
import torch

import canon_ref
import stereo_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL = sr.FILL
SEEDS = (101, 102, 103)
BAD_ARG = -1                                     # DL_ERR_BAD_ARG of include/difflinker_hip.h


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def batch_of(molecules, N, capacity=None, seed=0, scatter=True, status=None, n_in=None, nf=8):
    batch = sr.as_batch(molecules, N, capacity, nf=nf, rng=np.random.default_rng(seed), scatter=scatter)
    batch['status_in'] = np.zeros(len(molecules), np.int32) if status is None else np.asarray(status, np.int32)
    if n_in is not None:
        batch['n_bonds_in'] = np.asarray(n_in, np.int32)
    return batch


def arguments(batch, drop=True, mark=True, planar=True, aromatic=True, status=True, flat=sr.FLAT, twist=sr.TWIST, fill=FILL):
    """``(args, outputs, everything that must stay alive)`` for the C entry point, the outputs full of 0x5a bytes."""
    from difflinker_amd import _lib
    B, N = batch['node_mask'].shape
    nf, capacity = batch['one_hot'].shape[2], batch['bonds'].shape[1]
    held = [dev(batch['x']), dev(batch['one_hot']), dev(batch['node_mask']), dev(batch['drop_mask']), dev(batch['mark_mask']),
            dev(batch['atom_planar'], torch.int32), dev(sr.default_valence(nf), torch.int32), dev(batch['n_bonds_in'], torch.int32),
            dev(batch['bonds'], torch.int32), dev(batch['bond_aromatic'], torch.int32), dev(batch['status_in'], torch.int32)]
    x, one_hot, mask, drop_t, mark_t, planar_t, valence, n_in, bonds, aromatic_t, status_in = held
    shapes = {'atom_class': (B, N), 'atom_stereo': (B, N), 'bond_stereo': (B, capacity), 'counts': (B, 2, 4)}
    out = {name: torch.full(shapes.get(name, (B,)), fill, dtype=torch.int32, device=DEV) for name in sr.FIELDS}
    args = _lib.DLStereoArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
        drop_mask=drop_t.data_ptr() if drop else None, mark_mask=mark_t.data_ptr() if mark else None,
        atom_planar=planar_t.data_ptr() if planar else None, default_valence=valence.data_ptr(), capacity=capacity,
        n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr() if bonds.numel() else None,
        bond_aromatic=aromatic_t.data_ptr() if aromatic and bonds.numel() else None,
        status_in=status_in.data_ptr() if status else None, flat=flat, twist=twist, v_ideal4=sr.V_IDEAL4, v_ideal3=sr.V_IDEAL3,
        atom_class=out['atom_class'].data_ptr(), atom_stereo=out['atom_stereo'].data_ptr(),
        bond_stereo=out['bond_stereo'].data_ptr() if capacity else None, counts=out['counts'].data_ptr(),
        status=out['status'].data_ptr())
    return args, out, held


def launch(batch, stream=None, **kwargs):
    from difflinker_amd import _lib
    args, out, held = arguments(batch, **kwargs)
    args.stream = (torch.cuda.current_stream(torch.device(DEV)) if stream is None else stream).cuda_stream
    _lib.check(_lib.load().dl_stereo_perceive(ctypes.byref(args)), 'dl_stereo_perceive')
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def reference(batch, drop=True, mark=True, planar=True, aromatic=True, status=True, flat=sr.FLAT, twist=sr.TWIST):
    return sr.perceive(batch['x'], batch['one_hot'], batch['node_mask'], batch['bonds'], batch['n_bonds_in'], None, flat, twist,
                       batch['status_in'] if status else None, batch['drop_mask'] if drop else None,
                       batch['mark_mask'] if mark else None, batch['atom_planar'] if planar else None,
                       batch['bond_aromatic'] if aromatic else None)


def check(batch, **kwargs):
    got, want = launch(batch, **kwargs), reference(batch, **kwargs)
    for name in sr.FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.int32
        differ = got[name] != want[name]
        assert not differ.any(), (name, np.argwhere(differ)[:5].tolist(), got[name][differ][:5], want[name][differ][:5])
        assert got[name].tobytes() == want[name].tobytes()
    return got


@pytest.fixture(scope='module')
def randoms():
    return [m for seed in SEEDS for m in sr.random_molecules(seed, 16, max_atoms=24)]


def test_hand_built_molecules_in_every_output_bit():
    names = sorted(sr.HAND)
    got = check(batch_of([sr.HAND[name] for name in names], 16, scatter=False))
    for b, name in enumerate(names):                 # and what the rule must find, from first principles
        m = sr.HAND[name]
        centres = {c: sr.expected_centre(got['atom_class'][b], on, 1 if name == 'ammonium' else None)
                   for c, on in sr.CENTRES.get(name, {}).items()}
        if not name.startswith('tartaric'):
            assert {c: int(s) for c, s in enumerate(got['atom_stereo'][b][:len(m['types'])]) if s} == centres, name
        bonds = {(min(i, j), max(i, j)): int(got['bond_stereo'][b][e]) for e, (i, j, _) in enumerate(m['entries'])
                 if got['bond_stereo'][b][e]}
        assert bonds == sr.DOUBLE_BONDS.get(name, {}), name
    assert (got['status'] == 0).all()


def test_random_molecules_scattered_with_every_optional_input(randoms):
    labels = np.zeros(4, np.int64)
    for at in range(0, len(randoms), 16):
        got = check(batch_of(randoms[at:at + 16], 40, seed=at))
        labels += np.bincount(got['atom_stereo'][got['atom_stereo'] >= 0], minlength=4)[:4]
        labels[0] += (got['bond_stereo'] > 0).sum()
    assert labels[1] and labels[2] and labels[3] and labels[0], 'the set exercises both hands and the undetermined label'


@pytest.mark.parametrize('missing', ['drop', 'mark', 'planar', 'aromatic', 'status'])
def test_each_optional_input_may_be_null(randoms, missing):
    batch = batch_of(randoms[:16], 40, seed=5, status=[0, 2] * 8)
    check(batch, **{missing: False})
    check(batch, drop=False, mark=False, planar=False, aromatic=False, status=False)


def test_the_list_in_both_orientations_and_any_order(randoms):
    molecules = randoms[16:32]
    base = launch(batch_of(molecules, 40, seed=7))
    rng = np.random.default_rng(8)
    turned = []
    for m in molecules:
        order = [int(v) for v in rng.permutation(len(m['entries']))]
        entries = [m['entries'][e] for e in order]
        turned.append(dict(m, entries=[(j, i, o) if rng.random() < 0.5 else (i, j, o) for i, j, o in entries],
                           aromatic=sorted(order.index(e) for e in m['aromatic'])))
        turned[-1]['order'] = order
    got = check(batch_of(turned, 40, seed=7))
    for name in ('atom_class', 'atom_stereo', 'counts', 'status'):
        assert np.array_equal(got[name], base[name]), name
    for b, m in enumerate(turned):                   # a label goes with its entry
        for new, old in enumerate(m['order']):
            assert got['bond_stereo'][b, new] == base['bond_stereo'][b, old]


def test_repeated_pairs_entries_that_are_no_bond_and_list_lengths(randoms):
    molecules = [dict(m) for m in randoms[32:40]]
    for k, m in enumerate(molecules):
        entries, n = list(m['entries']), len(m['types'])
        if entries and k % 2 == 0:                   # a repeated pair with another order, in the other orientation
            i, j, o = entries[0]
            entries.append((j, i, o % 3 + 1))
        entries.insert(len(entries) // 2, [(0, 0, 1), (n, 0, 1), (-1, 0, 1), (0, n - 1, 4), (0, n - 1, 0)][k % 5])
        m['aromatic'] = []
        m['entries'] = entries
    got = check(batch_of(molecules, 40, seed=9))
    assert (got['status'] & sr.BAD_BOND).all()
    capacity = max(len(m['entries']) for m in molecules)
    got = check(batch_of(molecules, 40, capacity=capacity, seed=9, n_in=[capacity + 3, -2, 0, 1, capacity, 2, capacity + 1, 3],
                         status=[0, 2, 0, 2, 0, 2, 0, 2]))
    assert got['status'][0] & sr.BONDS_OVERFLOW and got['status'][6] & sr.BONDS_OVERFLOW and not got['status'][1] & sr.BONDS_OVERFLOW
    assert got['status'][1] == 2 and (got['bond_stereo'][1] == 0).all()


def test_a_nan_coordinate_keeps_the_classes_and_drops_the_labels():
    names = ['chfclbr_a', 'z_butene', 'l_alanine']
    batch = batch_of([sr.HAND[name] for name in names], 8, scatter=False)
    batch['x'][0, 2, 1] = np.nan
    batch['x'][1, 0, 0] = np.inf
    got = check(batch)
    assert list(got['status']) == [sr.NONFINITE, sr.NONFINITE, 0]
    assert (got['counts'][:2] == 0).all() and (got['atom_stereo'][:2] <= 0).all() and got['atom_class'][0, 0] == 3
    assert got['counts'][2, 0, 0] == 1


def chain(n):
    return sr.mol([sr.C if k % 5 else sr.N for k in range(n)], [(1.3 * k, 0.7 * (k % 2), 0.3 * (k % 3)) for k in range(n)],
                  [(k, k + 1, 1) for k in range(n - 1)])


def test_sizes_from_no_atom_to_the_limit_and_beyond():
    small = [sr.mol([], [], []), sr.mol([sr.C], [(0, 0, 0)], []), sr.mol([sr.C, sr.O], [(0, 0, 0), (1.2, 0, 0)], [(0, 1, 2)])]
    got = check(batch_of(small, 8, capacity=2, scatter=False))
    assert (got['atom_class'][0] == -1).all() and (got['counts'] == 0).all()
    big = [chain(256), chain(257), dict(chain(257), dropped=[5])]
    big[0]['entries'][100] = (100, 101, 2)           # a double bond in the long chain: trans on the zigzag
    got = check(batch_of(big, 300, seed=3))
    assert list(got['status']) == [0, sr.TOO_LARGE, 0]
    assert (got['atom_class'][1] == -1).all() and (got['atom_stereo'][1] == -1).all() and (got['bond_stereo'][1] == 0).all()
    assert got['counts'][0, 0, 2] + got['counts'][0, 0, 3] == 1


def test_too_many_kept_list_entries():
    m = chain(6)
    m['entries'] = [(k % 5, k % 5 + 1, 1) for k in range(sr.MAX_BONDS + 1)]
    fits = dict(m, entries=m['entries'][:sr.MAX_BONDS])
    bad = dict(m, entries=m['entries'] + [(0, 0, 1)])
    got = check(batch_of([m, fits, bad], 8, scatter=False))
    assert list(got['status']) == [sr.TOO_LARGE, sr.BAD_BOND, sr.TOO_LARGE | sr.BAD_BOND]


def test_an_empty_batch_and_every_bad_argument():
    from difflinker_amd import _lib
    lib = _lib.load()
    batch = batch_of([sr.HAND['z_butene']], 8, scatter=False)
    args, out, held = arguments(batch)
    assert lib.dl_stereo_perceive(None) == BAD_ARG
    for name, value in (('B', -1), ('N', 0), ('N', 1025), ('nf', 0), ('nf', 257), ('capacity', -1), ('flat', -0.1),
                        ('flat', float('nan')), ('twist', -0.5), ('twist', float('nan')), ('v_ideal4', 0.0), ('v_ideal3', -1.0),
                        ('v_ideal4', float('nan')), ('v_ideal3', float('nan'))):
        args, out, held = arguments(batch)
        setattr(args, name, value)
        assert lib.dl_stereo_perceive(ctypes.byref(args)) == BAD_ARG, name
    for name in ('x', 'one_hot', 'node_mask', 'default_valence', 'n_bonds_in', 'bonds', 'atom_class', 'atom_stereo', 'bond_stereo',
                 'counts', 'status'):
        args, out, held = arguments(batch)
        setattr(args, name, None)
        assert lib.dl_stereo_perceive(ctypes.byref(args)) == BAD_ARG, name
    args, out, held = arguments(batch)
    args.B = 0                                       # no launch: nothing is written, and the pointers are not looked at
    args.x = args.status = None
    assert lib.dl_stereo_perceive(ctypes.byref(args)) == _lib.DL_OK
    torch.cuda.synchronize()
    assert all((t == FILL).all() for t in out.values())


def test_every_output_element_is_overwritten_whatever_it_held(randoms):
    batch = batch_of(randoms[:8] + [chain(40)], 40, seed=11)
    a, b = launch(batch, fill=FILL), launch(batch, fill=-7)
    for name in sr.FIELDS:
        assert a[name].tobytes() == b[name].tobytes(), name
        assert not (a[name] == FILL).any(), name


def test_a_molecule_does_not_depend_on_its_neighbours_or_its_rows(randoms):
    molecules = randoms[8:24]
    together = launch(batch_of(molecules, 40, seed=13))
    for b in (0, 7, 15):
        m = molecules[b]
        n = len(m['types'])
        alone = launch(batch_of([m], 32, capacity=len(m['entries']) or 1, seed=14))
        rows = np.flatnonzero(batch_of(molecules, 40, seed=13)['node_mask'][b])
        assert len(rows) == n
        for name in ('atom_class', 'atom_stereo'):   # by atom number, whatever the rows
            assert np.array_equal(alone[name][0][:n], together[name][b][:n]), name
        assert np.array_equal(alone['bond_stereo'][0][:len(m['entries'])], together['bond_stereo'][b][:len(m['entries'])])
        assert np.array_equal(alone['counts'][0], together['counts'][b]) and alone['status'][0] == together['status'][b]


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def place_on_device(v, dtype=None):
    return dev(v, dtype or torch.float32)


def bonds_of(batch, status=None, place=place_on_device):
    from difflinker_amd.molecule_builder import Bonds
    return Bonds(place(batch['n_bonds_in'], torch.int32), place(batch['bonds'], torch.int32), None, None, None,
                 place(batch['status_in'] if status is None else status, torch.int32))


def through_python(batch, found=None, place=place_on_device, host=True, **kwargs):
    """``metrics.stereo`` with every input put on the device through ``place`` (the stream tests stage them behind a delay)."""
    from difflinker_amd import metrics
    out = metrics.stereo(place(batch['one_hot']), place(batch['x']), place(batch['node_mask']), found or bonds_of(batch, place=place),
                         True, place(batch['drop_mask']), place(batch['mark_mask']), place(batch['atom_planar'], torch.int32),
                         place(batch['bond_aromatic'], torch.int32), **kwargs)
    return {name: out[name].cpu().numpy() for name in sr.FIELDS} if host else out


def test_the_python_layer_on_plain_strided_sliced_and_wide_typed_inputs(randoms):
    from difflinker_amd import metrics
    from difflinker_amd.molecule_builder import Bonds
    batch = batch_of(randoms[:16], 40, seed=17)
    want = reference(batch)
    got = through_python(batch)
    for name in sr.FIELDS:
        assert got[name].tobytes() == want[name].tobytes(), name
    B, N = batch['node_mask'].shape
    wide = torch.zeros((B, 2 * N, 3), dtype=torch.float64, device=DEV)
    wide[:, ::2] = dev(batch['x'], torch.float64)    # fp64, every second row of a wider tensor
    hot = dev(batch['one_hot'], torch.float64).transpose(1, 2).contiguous().transpose(1, 2)
    padded = torch.full((B, batch['bonds'].shape[1] + 3, 3), 9, dtype=torch.int64, device=DEV)
    padded[:, :-3] = dev(batch['bonds'], torch.int64)
    found = Bonds(dev(batch['n_bonds_in'], torch.int64), padded[:, :-3], None, None, None, dev(batch['status_in'], torch.int64))
    out = metrics.stereo(hot, wide[:, ::2], dev(batch['node_mask'])[:, :, None], found, True, dev(batch['drop_mask'], torch.float64),
                         dev(batch['mark_mask']) != 0, dev(batch['atom_planar'], torch.int64), dev(batch['bond_aromatic'], torch.int64))
    for name in sr.FIELDS:
        assert out[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    loose = reference(batch, flat=0.05, twist=0.1)
    got = through_python(batch, flat=0.05, twist=0.1)
    assert all(got[name].tobytes() == loose[name].tobytes() for name in sr.FIELDS) and (loose['counts'] != want['counts']).any()
    with pytest.raises(ValueError):
        through_python(batch, flat=-1.0)


def host_codes(m, max_leaves=256):
    """``(stereo_code, mirror_code)`` of a molecule dict by the restatement and ``canon_ref`` on the widened types."""
    r = sr.perceive_one(m)
    n = len(m['types'])
    return tuple(canon_ref.canonical_ranks(sr.wide_types(m['types'], m['entries'], r['atom_stereo'][:n], r['bond_stereo'], mirror),
                                           m['entries'], max_leaves=max_leaves)['code'] for mirror in (False, True))


def test_stereo_codes_on_the_device_against_the_host():
    from difflinker_amd import metrics
    names = [name for name in sorted(sr.HAND) if name.startswith(('tartaric', 'hexadiene'))] + ['l_alanine', 'benzene']
    batch = batch_of([sr.HAND[name] for name in names], 16, scatter=False)
    found = bonds_of(batch)
    one_hot, mask = dev(batch['one_hot']), dev(batch['node_mask'])
    result = metrics.stereo(one_hot, dev(batch['x']), mask, found, True, bond_aromatic=dev(batch['bond_aromatic'], torch.int32),
                            atom_planar=dev(batch['atom_planar'], torch.int32))
    codes = metrics.stereo_codes(result, one_hot, mask, found)
    unsigned = lambda t: [int(v) & 0xFFFFFFFFFFFFFFFF for v in t.cpu().tolist()]     # noqa: E731
    got = dict(zip(names, zip(unsigned(codes['stereo_code']), unsigned(codes['mirror_code']))))
    for name in names:
        assert got[name] == host_codes(sr.HAND[name]), name
    chiral = dict(zip(names, codes['chiral'].cpu().tolist()))
    assert codes['complete'].all()
    a, b, meso, other = (got[f'tartaric_{k}'] for k in ('chiral_a', 'chiral_b', 'meso_12', 'meso_21'))
    assert a[0] == b[1] and a[1] == b[0] and a[0] != a[1] and chiral['tartaric_chiral_a'] and chiral['tartaric_chiral_b']
    assert meso == other and meso[0] == meso[1] and not chiral['tartaric_meso_12'] and len({a[0], b[0], meso[0]}) == 3
    assert len({got[f'hexadiene_{k}'][0] for k in ('ee', 'ez', 'zz')}) == 3 and not chiral['hexadiene_ez']
    assert chiral['l_alanine'] and not chiral['benzene']
    with pytest.raises(ValueError):
        metrics.stereo_codes(result, torch.zeros((len(names), 16, 17), device=DEV), mask, found)


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------
def read_csv(path):
    import csv
    with open(path, newline='') as f:
        return list(csv.DictReader(f))


STEREO_KEYS = {'centres', 'centres_linker', 'double_bonds', 'double_bonds_linker', 'undetermined', 'stereo_code', 'chiral', 'complete',
               'isomeric_smiles', 'file'}


def test_generate_with_stereo_adds_its_files_and_changes_no_other(tmp_path, monkeypatch):
    """``generate`` behind the sampler, as ``test_gpu_canon`` drives it: hand-made linkers that bridge two fragments stand in
    for sampled ones."""
    import filecmp
    import json
    import os
    import test_gpu_select as SEL
    from difflinker_amd import metrics
    from difflinker_amd.generate import generate
    monkeypatch.setattr(SEL, 'LINKERS', ('CNCC', 'CNCC', 'CCOC'))
    ddpm = SEL.synthetic_ddpm()
    monkeypatch.setattr(ddpm, 'sample_chain', lambda data, sample_fn=None, keep_frames=None: SEL.bridging_chain(data, ddpm), raising=False)
    frag = str(tmp_path / 'bridge.sdf')
    with open(frag, 'w') as f:
        f.write(SEL.BRIDGE_SDF)
    runs = {}
    for tag, flags in (('plain', {'smiles': True, 'metrics': True}), ('stereo', {'smiles': True, 'metrics': True, 'stereo': True}),
                       ('alone', {'stereo': True}), ('bare', {})):
        torch.manual_seed(11)
        runs[tag] = generate(frag, ddpm, str(tmp_path / tag), n_samples=3, n_steps=5, linker_size='4', output_format='both', **flags)
    names = [os.path.basename(path) for path in runs['plain']]
    assert set(os.listdir(tmp_path / 'stereo')) - set(os.listdir(tmp_path / 'plain')) == {'stereo.json'}
    assert set(os.listdir(tmp_path / 'alone')) - set(os.listdir(tmp_path / 'bare')) == {'stereo.json'}
    for with_flag, without in (('stereo', 'plain'), ('alone', 'bare')):
        for name in sorted(os.listdir(tmp_path / without)):
            if name not in ('smiles.csv', 'metrics.json'):
                assert filecmp.cmp(tmp_path / without / name, tmp_path / with_flag / name, shallow=False), (with_flag, name)
    assert filecmp.cmp(tmp_path / 'stereo' / 'stereo.json', tmp_path / 'alone' / 'stereo.json', shallow=False)
    records = json.load(open(tmp_path / 'stereo' / 'stereo.json'))
    assert [r['file'] for r in records] == names and all(set(r) == STEREO_KEYS for r in records)
    assert all(len(r['stereo_code']) == 16 and r['isomeric_smiles'] for r in records)
    plain_rows, rows = read_csv(tmp_path / 'plain' / 'smiles.csv'), read_csv(tmp_path / 'stereo' / 'smiles.csv')
    assert 'isomeric_smiles' not in plain_rows[0] and list(rows[0])[-1] == 'isomeric_smiles'
    assert [{k: v for k, v in row.items() if k != 'isomeric_smiles'} for row in rows] == plain_rows
    assert [row['isomeric_smiles'] for row in rows] == [r['isomeric_smiles'] for r in records]
    scores, plain_scores = json.load(open(tmp_path / 'stereo' / 'metrics.json')), json.load(open(tmp_path / 'plain' / 'metrics.json'))
    assert {k: v for k, v in scores.items() if k not in metrics.STEREO_NAMES} == plain_scores
    assert set(metrics.STEREO_NAMES) <= set(scores) and not set(metrics.STEREO_NAMES) & set(plain_scores)
    assert not os.path.exists(tmp_path / 'alone' / 'metrics.json')


def test_sample_with_stereo_adds_its_files_and_changes_no_other(tmp_path):
    import filecmp
    import json
    import os
    import test_gpu_rings as RG
    from difflinker_amd import metrics
    from difflinker_amd.sample import sample
    m = RG.gentle_model(tmp_path, False)
    outs = {}
    for tag, flags in (('plain', {'metrics': True, 'smiles': True}), ('stereo', {'metrics': True, 'smiles': True, 'stereo': True})):
        m.edm.noise_seed = 5
        outs[tag] = sample(m, str(tmp_path / tag), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, output_format='sdf',
                           **flags)
    plain, out = outs['plain'], outs['stereo']
    names = sorted(os.path.join(u, name) for u in os.listdir(plain) if os.path.isdir(os.path.join(plain, u))
                   for name in os.listdir(os.path.join(plain, u)))
    for name in names:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain))) == ['stereo.json']
    records = json.load(open(os.path.join(out, 'stereo.json')))
    sampled = [name for name in names if name.endswith('_.sdf')]
    assert sorted(r['file'] for r in records) == sampled and all(set(r) == STEREO_KEYS for r in records)
    plain_rows, rows = read_csv(os.path.join(plain, 'smiles.csv')), read_csv(os.path.join(out, 'smiles.csv'))
    assert [{k: v for k, v in row.items() if k != 'isomeric_smiles'} for row in rows] == plain_rows
    assert 'isomeric_smiles' not in plain_rows[0] and all('isomeric_smiles' in row for row in rows)
    scores, plain_scores = json.load(open(os.path.join(out, 'metrics.json'))), json.load(open(os.path.join(plain, 'metrics.json')))
    added = set(metrics.STEREO_NAMES + metrics.STEREO_TRUE_NAMES)
    assert {k: v for k, v in scores.items() if k not in added} == plain_scores and added <= set(scores)
    assert all(0.0 <= scores[k] <= 1.0 for k in ('stereo_undetermined', 'chiral_fraction', 'stereo_uniqueness') + metrics.STEREO_TRUE_NAMES)
