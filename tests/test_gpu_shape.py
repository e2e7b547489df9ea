"""``dl_shape_scores`` (csrc/shape.hip) on the GPU against its numpy-float32 restatement ``shape_ref``: every output EXACTLY -
the rule fixes every rounding and every output is an integer, so there is no tolerance anywhere but where coordinates went
through a text file.  One mixed batch is scored once by ``shape_ref`` and shared: the atom counts at which the loops over atoms
wrap (wave and workgroup strides), the extents at which the box is split (in every direction), the extent limit on either
side, rows in random order between padding rows that hold garbage.  Around it: flagged pairs between good ones, stale output
buffers, unequal widths, an exact translation of the whole batch (which the kernel and the helper cannot share a mistake
in), two launches, another radius table, and the public path through ``sample`` and ``DDPM.sample_and_analyze``."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import shape_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NF = 9
FIELDS = shape_ref.FIELDS
EYE = np.eye(NF, dtype=np.float32)
# (n_a, n_b): 0 and 1 on either side, then the wave (64) and workgroup (256) strides of the loops over rows, and a second and
# third chunk of 256 rows on one side only
COUNTS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 63), (64, 65), (110, 110), (256, 257), (1, 600)]
NA, NB = 640, 700                                # rows of A and of B: independent, both wider than any molecule
GRID = 2.0 ** -10                                # coordinates are multiples of this: a shift by a multiple of 0.5 is exact


def cloud(rng, n, box):
    """``n`` atoms in a box of ``box`` A around a centre within +-50 A: multiples of 2^-10, a quarter of them moved onto lattice
    points and a quarter onto half-spacings (the two places where a point sits exactly on a coordinate plane of an atom)."""
    centre = rng.integers(-100, 101, size=3) * 0.5
    x = centre + np.round(rng.uniform(0, box, size=(n, 3)) / GRID) * GRID
    kind = rng.integers(0, 4, size=n)
    x[kind == 0] = np.round(x[kind == 0] * 2) / 2
    x[kind == 1] = np.round(x[kind == 1] * 2) / 2 + 0.25
    return x.astype(np.float32)


def rows_of(rng, x, types, n_rows):
    """The atoms in random rows of an ``n_rows`` wide molecule; the other rows hold finite garbage and a mask of 0."""
    n = len(x)
    full_x = rng.choice(np.float32([1e4, -3e7, 3.4e38, 0.125]), size=(n_rows, 3))
    one_hot = rng.uniform(-5, 5, size=(n_rows, NF)).astype(np.float32)
    mask = np.zeros(n_rows, np.float32)
    at = np.sort(rng.permutation(n_rows)[:n])
    order = rng.permutation(n)
    full_x[at], one_hot[at], mask[at] = x[order], EYE[np.asarray(types, dtype=np.int64)[order]], 1
    return full_x, one_hot, mask


def pair(rng, xa, xb, ta=None, tb=None, na=NA, nb=NB):
    ta = rng.integers(0, NF, size=len(xa)) if ta is None else ta
    tb = rng.integers(0, NF, size=len(xb)) if tb is None else tb
    return rows_of(rng, np.float32(xa).reshape(-1, 3), ta, na) + rows_of(rng, np.float32(xb).reshape(-1, 3), tb, nb)


def build_pairs():
    rng = np.random.default_rng(2025)
    pairs, names = [], []

    def add(name, *args, **kw):
        names.append(name)
        pairs.append(pair(rng, *args, **kw))

    for n_a, n_b in COUNTS:
        box = 8.0 if max(n_a, n_b) <= 110 else 16.0
        xa, xb = cloud(rng, n_a, box), cloud(rng, n_b, box)
        if n_a and n_b:                                                 # B onto A by a multiple of the spacing: the two overlap
            xb = (xb + np.round((xa.mean(0) - xb.mean(0)) * 2) / 2).astype(np.float32)
        add(f'counts_{n_a}_{n_b}', xa, xb)
    # a compact 50-atom zigzag chain against a jittered copy of itself, same elements
    k = np.arange(50)
    chain = np.stack([1.25 * k, 0.8 * (k % 2), 0.3 * (k % 3)], 1) * 0.6 + np.float32([-41.5, 37.25, 12.0])
    chain = (np.round(chain / GRID) * GRID).astype(np.float32)
    jitter = (np.round(rng.normal(0, 0.3, size=chain.shape) / GRID) * GRID).astype(np.float32)
    types = rng.integers(0, NF, size=50)
    add('chain', chain, chain + jitter, types, types)
    # two atoms 100 A apart along every axis in turn: every split of the box is crossed in every direction
    for axis in range(3):
        far = np.zeros(3, np.float32)
        far[axis] = 100.0
        base = np.float32([-48.75, -47.5, -52.125])
        add(f'apart_{"xyz"[axis]}', [base, base + far], [base + np.float32(0.375), base + far - np.float32(0.25)])
    # the only overlap is between the LAST rows of the two molecules
    xa, xb = cloud(rng, 40, 8.0), cloud(rng, 45, 8.0)
    xb += np.float32([40.0, 0.0, 0.0]) + (xa.mean(0) - xb.mean(0)).round()
    names.append('last_rows')
    a_rows, b_rows = rows_of(rng, xa, rng.integers(0, NF, 40), NA), rows_of(rng, xb, rng.integers(0, NF, 45), NB)
    meet = xa.mean(0).round() + np.float32([0.0, 30.0, 0.0])
    a_rows[0][np.nonzero(a_rows[2])[0][-1]] = meet
    b_rows[0][np.nonzero(b_rows[2])[0][-1]] = meet + np.float32([0.75, 0.25, 0.0])
    pairs.append(a_rows + b_rows)
    # the extent limit: hi - lo = 240 lattice steps is scored, 241 is flagged
    add('extent_240', [[-60.0, 3.0, 1.0]], [[60.25, 3.5, 1.0]])
    add('extent_241', [[-60.0, 3.0, 1.0]], [[60.5, 3.5, 1.0]])
    return names, tuple(np.stack(part) for part in zip(*pairs))


@pytest.fixture(scope='module')
def mixed():
    names, arrays = build_pairs()
    want = shape_ref.shape_scores(*arrays)                              # x_a, one_hot_a, mask_a, x_b, one_hot_b, mask_b
    for part in (*arrays, *want.values()):
        part.setflags(write=False)
    return dict(names=names, arrays=arrays, want=want)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def score(arrays, **kw):
    from difflinker_amd.metrics import analyze_shapes
    x_a, one_hot_a, mask_a, x_b, one_hot_b, mask_b = (dev(a) for a in arrays)
    return analyze_shapes(one_hot_a, x_a, mask_a, one_hot_b, x_b, mask_b, **kw)


def as_dict(got):
    return {name: getattr(got, name).cpu().numpy() for name in FIELDS}


def assert_exact(got, want, what=''):
    got = as_dict(got) if not isinstance(got, dict) else got
    for name in FIELDS:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (what, name, got[name], want[name])


def test_mixed_batch_is_exact(mixed):
    got = as_dict(score(mixed['arrays']))
    for name in FIELDS:
        print(name, got[name].tolist())
    assert_exact(got, mixed['want'], 'mixed batch')
    at = mixed['names'].index
    assert got['status'].tolist() == [0] * (len(mixed['names']) - 1) + [shape_ref.TOO_LARGE]
    assert [got[name][at('extent_241')] for name in FIELDS[:8]] == [0] * 8
    assert got['n_a'][:len(COUNTS)].tolist() == [a for a, _ in COUNTS] and got['n_b'][:len(COUNTS)].tolist() == [b for _, b in COUNTS]
    assert got['vol_min'][at('counts_110_110')] > 1000 and got['vol_min'][at('counts_256_257')] > 1000, 'the clouds overlap'
    assert got['vol_min'][at('counts_1_0')] == 0 < got['vol_a'][at('counts_1_0')] and got['vol_b'][at('counts_1_0')] == 0
    assert 0 < got['vol_min'][at('chain')] < got['vol_a'][at('chain')]
    for axis in 'xyz':
        assert got['core_both'][at(f'apart_{axis}')] > 0 and got['n_a'][at(f'apart_{axis}')] == 2
    assert 0 < got['vol_min'][at('last_rows')] < 1000, 'one atom of either molecule meets: a lone iodine, the largest, is about 650'
    assert got['vol_min'][at('extent_240')] == 0 < got['vol_b'][at('extent_240')]


def test_two_launches_give_the_same_bits(mixed):
    first, again = score(mixed['arrays']), score(mixed['arrays'])
    for name in FIELDS:
        assert torch.equal(getattr(first, name), getattr(again, name)), name


def test_translation_by_lattice_multiples_changes_nothing(mixed):
    """Both molecules of every pair moved by (8, -16, 32.5): multiples of the spacing, and exact, since every coordinate is a
    multiple of 2^-10 below 256 in size.  The box, its bricks and every clipping move; the rule's outputs do not."""
    x_a, one_hot_a, mask_a, x_b, one_hot_b, mask_b = mixed['arrays']
    shift = np.float32([8.0, -16.0, 32.5])
    moved_a, moved_b = x_a.copy(), x_b.copy()
    moved_a[mask_a != 0] += shift
    moved_b[mask_b != 0] += shift
    assert np.array_equal((moved_a[mask_a != 0] - shift), x_a[mask_a != 0]), 'the shift is exact'
    assert_exact(score((moved_a, one_hot_a, mask_a, moved_b, one_hot_b, mask_b)), mixed['want'], 'translated')


def test_c_entry_writes_every_element_of_stale_buffers(mixed):
    """The C entry on output buffers that hold 0x7f bytes, the padding rows of every input NaN."""
    from difflinker_amd import _lib, const
    arrays = [a.copy() for a in mixed['arrays']]
    for x, one_hot, mask in (arrays[:3], arrays[3:]):
        x[mask == 0] = np.nan
        one_hot[mask == 0] = np.nan
    ins = dict(zip(('x_a', 'one_hot_a', 'mask_a', 'x_b', 'one_hot_b', 'mask_b'), (dev(a) for a in arrays)))
    ins['r2'] = const.shape_radius_table(True).to(DEV)
    B = len(arrays[0])
    out = {name: torch.full((B, 4), 0x7f, dtype=torch.uint8, device=DEV) for name in FIELDS}
    args = _lib.DLShapeArgs(B=B, Na=NA, Nb=NB, nf=NF, **{k: v.data_ptr() for k, v in ins.items()},
                            **{k: v.data_ptr() for k, v in out.items()})
    _lib.check(_lib.load().dl_shape_scores(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'shape')
    torch.cuda.synchronize()
    assert_exact({name: out[name].view(torch.int32).squeeze(-1).cpu().numpy() for name in FIELDS}, mixed['want'], 'stale')


def test_flagged_pairs_leave_their_neighbours_alone(mixed):
    names = mixed['names']
    pick = [names.index(n) for n in ('counts_110_110', 'counts_64_65', 'chain', 'counts_2_63', 'counts_256_257', 'counts_1_1',
                                     'last_rows', 'counts_64_65', 'apart_y')]
    arrays = [a[pick].copy() for a in mixed['arrays']]
    x_a, _, mask_a, x_b, _, mask_b = arrays
    x_a[1, np.nonzero(mask_a[1])[0][40], 2] = np.nan                    # a NaN in a participating row of A
    x_b[3, np.nonzero(mask_b[3])[0][-1], 0] = -np.inf                   # an infinity in a participating row of B
    x_a[5, np.nonzero(mask_a[5])[0][0], 1] = 5000.0                     # out of range
    x_b[7, np.nonzero(mask_b[7] == 0)[0][3], 1] = np.nan                # a NaN in a row that takes no part: no flag
    x_a[7, np.nonzero(mask_a[7] == 0)[0][0]] = np.inf
    got = score(arrays)
    assert_exact(got, shape_ref.shape_scores(*arrays), 'flagged')
    assert got.status.tolist() == [0, 1, 0, 1, 0, 2, 0, 0, 0]
    for b in (1, 3, 5):
        assert [int(getattr(got, name)[b]) for name in FIELDS[:8]] == [0] * 8
    # a NaN decides before an out-of-range coordinate does, whichever comes first in the rows
    both = [a[[1, 5]].copy() for a in arrays]
    both[0][1, np.nonzero(both[2][1])[0][0], 0] = np.nan
    both[3][0, np.nonzero(both[5][0])[0][0], 2] = -4096.5
    assert score(both).status.tolist() == [1, 1]
    good = [0, 2, 4, 6, 7, 8]
    alone = score([a[good] for a in arrays])
    for name in FIELDS:
        assert torch.equal(getattr(got, name)[good], getattr(alone, name)), name
        assert np.array_equal(getattr(alone, name).cpu().numpy()[:5], mixed['want'][name][[pick[g] for g in good[:5]]]), name


def test_widths_do_not_matter_and_other_radii():
    rng = np.random.default_rng(7)
    atoms = [(cloud(rng, 30, 6.0), rng.integers(0, NF, 30), cloud(rng, 37, 6.0), rng.integers(0, NF, 37)) for _ in range(3)]
    atoms = [(xa, ta, xb - (xb.mean(0) - xa.mean(0)).round(), tb) for xa, ta, xb, tb in atoms]

    def batch(na, nb):
        mols = []
        for xa, ta, xb, tb in atoms:                                    # the same atoms in row order at the front of either width
            row = []
            for x, t, n in ((xa, ta, na), (xb, tb, nb)):
                full_x, one_hot, mask = np.full((n, 3), 77.0, np.float32), np.zeros((n, NF), np.float32), np.zeros(n, np.float32)
                full_x[:len(x)], one_hot[:len(x)], mask[:len(x)] = x, EYE[t], 1
                row += [full_x, one_hot, mask]
            mols.append(row)
        return [np.stack(part) for part in zip(*mols)]

    want = shape_ref.shape_scores(*batch(40, 55))
    assert (want['vol_min'] > 0).all() and (want['status'] == 0).all()
    for na, nb in ((40, 55), (55, 55), (30, 37), (300, 38)):
        assert_exact(score(batch(na, nb)), want, f'widths {na} {nb}')
    # scale 1.0, step 0.5: the same helper on the same table
    wide = shape_ref.shape_scores(*batch(40, 55), r2=shape_ref.radius_table(NF, 1.0, 0.5))
    assert (wide['vol_a'] > want['vol_a']).all()
    assert_exact(score(batch(40, 55), scale=1.0, step=0.5), wide, 'scale 1.0 step 0.5')


def test_single_pair_empty_batch_and_cpu_tensors(mixed):
    from difflinker_amd import _lib
    from difflinker_amd.metrics import ShapeRecord, analyze_shapes, shapes_to_host
    b = mixed['names'].index('chain')
    one = score([a[b:b + 1] for a in mixed['arrays']])
    assert_exact(one, {name: mixed['want'][name][b:b + 1] for name in FIELDS}, 'one pair')
    assert shapes_to_host(one) == [ShapeRecord(*(int(mixed['want'][name][b]) for name in FIELDS))]
    none = score([np.zeros((0, 5, 3)), np.zeros((0, 5, NF)), np.zeros((0, 5)), np.zeros((0, 7, 3)), np.zeros((0, 7, NF)), np.zeros((0, 7))])
    assert none.vol_min.shape == (0,) and shapes_to_host(none) == []
    gpu, cpu = torch.zeros(1, 4, NF, device=DEV), torch.zeros(1, 4, NF)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_shapes(gpu, gpu[:, :, :3], gpu[:, :, 0], cpu, gpu[:, :, :3], gpu[:, :, 0])
    with pytest.raises(ValueError, match='20 A'):
        analyze_shapes(gpu, gpu[:, :, :3], gpu[:, :, 0], gpu, gpu[:, :, :3], gpu[:, :, 0], scale=20.0)


# ---- the public path ------------------------------------------------------------------------------------------------------

def gentle_model(tmp_path, pockets):
    """The toy model and data set of ``test_gpu_metrics`` with a noise schedule that ends at alpha_T^2 = 0.05 instead of 1e-5.
    The toy denoiser is untrained and predicts next to no noise, so a chain hands back about z_T / alpha_T: with 1e-5 the
    linker atoms land +-500 A from the fragments (measured: coordinates from -640 to 660 A, 10 of 10 pairs rightly flagged
    ``DL_SHAPE_TOO_LARGE``, nothing scored); with 0.05 they stay within some tens of A and every pair is scored."""
    from difflinker_amd.noise import PredefinedNoiseSchedule
    from test_gpu_metrics import toy_model
    m = toy_model(tmp_path, pockets)
    m.edm.gamma = PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=0.05).to(DEV)
    return m


def records_from_files(out_dir, n_samples):
    """``ShapeRecord`` values of ``shape_ref`` on the atoms of the written files, over all atoms and over the linker atoms (the
    rows after the fragments', in the toy data set's layout), and the samples' atoms for ``metrics.analyze``."""
    from difflinker_amd import const
    from difflinker_amd.metrics import ShapeRecord
    from test_gpu_generate import read_xyz
    whole, linker, samples = [], [], []
    for folder in sorted(glob.glob(os.path.join(out_dir, '*', ''))):
        true_syms, true_pos = read_xyz(os.path.join(folder, 'true_.xyz'))
        n_frag = len(read_xyz(os.path.join(folder, 'frag_.xyz'))[0])
        for i in range(n_samples):
            syms, pos = read_xyz(os.path.join(folder, f'{i}_.xyz'))
            ta, tb = [const.GEOM_ATOM2IDX[s] for s in syms], [const.GEOM_ATOM2IDX[s] for s in true_syms]
            samples.append((ta, pos))
            for records, first in ((whole, 0), (linker, n_frag)):
                got = shape_ref.shape_scores(pos[None, first:], EYE[ta][None, first:], np.ones((1, len(ta) - first)),
                                             true_pos[None, first:], EYE[tb][None, first:], np.ones((1, len(tb) - first)))
                records.append(ShapeRecord(*(int(got[name][0]) for name in FIELDS)))
    return whole, linker, samples


def assert_close(got, want):
    assert set(got) == set(want)
    for key, value in want.items():
        if value is None or isinstance(value, int):
            assert got[key] == value, key
        else:
            assert abs(got[key] - value) <= 1e-6, (key, got[key], value)


def test_sample_writes_the_shape_keys(tmp_path):
    from difflinker_amd.metrics import METRIC_NAMES, SHAPE_NAMES, _good, analyze, compute_shapes, to_host
    from difflinker_amd.sample import sample
    m = gentle_model(tmp_path, False)
    out = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, shape=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    whole, linker, _ = records_from_files(out, 2)
    assert set(got) == set(SHAPE_NAMES) | {'shape_tanimoto_linker'}, 'alone when metrics are not asked for'
    assert got['shape_molecules'] == 5 * 2 and got['shape_flagged'] == 0 and type(got['shape_molecules']) is int
    assert all(r.n_a == r.n_b for r in whole) and all(r.n_a == r.n_b == 3 for r in linker)
    assert 0.0 < got['shape_tanimoto'] <= got['shape_similarity'] <= 1.0, 'the fragments are shared, so the volumes overlap'
    assert_close(got, compute_shapes(whole, linker))
    both = sample(m, str(tmp_path / 'both'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, shape=True)
    got = json.load(open(os.path.join(both, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | set(SHAPE_NAMES) | {'shape_tanimoto_linker', 'shape_tanimoto_valid'}
    whole, linker, samples = records_from_files(both, 2)
    width = max(len(t) for t, _ in samples)
    one_hot, x, mask = np.zeros((len(samples), width, 8), np.float32), np.zeros((len(samples), width, 3), np.float32), \
        np.zeros((len(samples), width, 1), np.float32)
    for k, (types, pos) in enumerate(samples):
        one_hot[k, :len(types)], x[k, :len(types)], mask[k, :len(types)] = np.eye(8, dtype=np.float32)[types], pos, 1
    pred = to_host(analyze(dev(one_hot), dev(x), dev(mask), False), dev(one_hot), dev(mask))
    assert_close({k: v for k, v in got.items() if k.startswith('shape_')}, compute_shapes(whole, linker, pred))
    assert (got['shape_tanimoto_valid'] is None) == (not any(_good(p) for p in pred))
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}


def shapes_by_hand(m):
    """The shape part of ``sample_and_analyze`` spelled out: the same chains in the same order, the true molecule centred as
    ``sample_chain`` centres its input (on the fragments, without the pocket), scored through the public functions.  Also the
    premise of the whole score: the sample's fragment atoms lie where the true molecule's do."""
    from difflinker_amd import utils
    from difflinker_amd.metrics import analyze, analyze_shapes, compute_shapes, shapes_to_host, to_host
    from test_gpu_metrics import DDPM_sample_chain
    whole, linker, pred = [], [], []
    for data in m.val_dataloader():
        drop = data['pocket_mask'] if m.pockets else None
        frag = data['fragment_only_mask'] if m.pockets else data['fragment_mask']
        ligand = data['atom_mask'] - drop if m.pockets else data['atom_mask']
        true_x = utils.remove_partial_mean_with_mask(data['positions'], data['atom_mask'], frag)
        types = data['one_hot']
        for _ in range(m.n_stability_samples):
            chain, node_mask = DDPM_sample_chain(m, data)
            assert node_mask.shape == data['atom_mask'].shape, 'the true sizes: the template is as wide as the input'
            x, one_hot = chain[0][:, :, :3], chain[0][:, :, 3:]
            pred += to_host(analyze(one_hot, x, node_mask, m.is_geom, drop_mask=drop), one_hot, node_mask, drop)
            whole += shapes_to_host(analyze_shapes(one_hot, x, ligand, types, true_x, ligand, is_geom=m.is_geom))
            linker += shapes_to_host(analyze_shapes(one_hot, x, data['linker_mask'], types, true_x, data['linker_mask'],
                                                    is_geom=m.is_geom))
            for r in shapes_to_host(analyze_shapes(one_hot, x, frag, types, true_x, frag, is_geom=m.is_geom)):
                # the same atoms up to the roundings of the chain's normalisation: a point flips only on a sphere's very surface
                assert r.status == 0 and r.n_a == r.n_b >= 6 and r.vol_min >= 0.99 * max(r.vol_a, r.vol_b), r
    return compute_shapes(whole, linker, pred)


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path, pockets):
    from difflinker_amd.metrics import METRIC_NAMES, SHAPE_NAMES
    m = gentle_model(tmp_path, pockets)
    assert m.shape_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.shape_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(SHAPE_NAMES) | {'shape_tanimoto_linker', 'shape_tanimoto_valid'}
    assert {k: got[k] for k in METRIC_NAMES} == plain
    assert got['shape_molecules'] == 5 * 3 and got['shape_flagged'] == 0
    assert 0.0 < got['shape_tanimoto'] <= got['shape_similarity'] <= 1.0, 'the fragments lie where the true molecule has them'
    m.edm.noise_seed = 5
    assert {k: v for k, v in got.items() if k.startswith('shape_')} == shapes_by_hand(m)
    json.dumps(got)
