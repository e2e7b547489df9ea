"""The shape score without a GPU: the numpy restatement ``shape_ref`` on the cases worked by hand and against its own dense
evaluation, the radius table, the new C entry (exported where the header says, arguments checked, ABI unchanged),
``compute_shapes`` on hand-written records, and the drivers' flag."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import shape_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(9, dtype=np.float32)
C, O = 0, 1


def score(xa, ta, xb, tb, **kw):
    """One pair given as atom lists; every row takes part."""
    xa, xb = np.float32(xa).reshape(1, -1, 3), np.float32(xb).reshape(1, -1, 3)
    got = shape_ref.shape_scores(xa, EYE[np.int64(ta)][None], np.ones((1, len(ta))), xb, EYE[np.int64(tb)][None], np.ones((1, len(tb))), **kw)
    return {k: int(v[0]) for k, v in got.items()}


def test_reference_reproduces_the_numbers_worked_by_hand():
    assert [float(v) for v in shape_ref.radius_table()[C]] == [np.float32(1.8496001), np.float32(2.5921001), np.float32(3.4596)]
    for dense in (False, True):
        got = score([[0, 0, 0]], [C], [[1, 0, 0]], [O], dense=dense)
        assert (got['vol_a'], got['core_a'], got['vol_b'], got['core_b']) == (431, 81, 321, 57)
        assert (got['vol_min'], got['core_both'], got['n_a'], got['n_b'], got['status']) == (196, 27, 1, 1, 0)
        got = score([[0, 0, 0]], [C], [[0.25, 0, 0]], [C], dense=dense)
        assert (got['vol_b'], got['core_b'], got['vol_min'], got['core_both']) == (460, 94, 394, 77), \
            'the lattice is fixed in space: a shift below its spacing changes the counts'
        got = score([[0, 0, 0]], [C], [[5, 0, 0]], [C], dense=dense)
        assert (got['vol_a'], got['vol_b'], got['vol_min'], got['core_both']) == (431, 431, 0, 0)
    # a shift by a multiple of the spacing changes nothing
    assert score([[7.5, -3, 0.5]], [C], [[8.5, -3, 0.5]], [O]) == score([[0, 0, 0]], [C], [[1, 0, 0]], [O])
    # no atoms on one side, or on both: not an error
    assert score(np.zeros((0, 3)), [], [[1, 0, 0]], [O]) == dict(vol_a=0, vol_b=321, vol_min=0, core_a=0, core_b=57, core_both=0,
                                                                 n_a=0, n_b=1, status=0)
    assert set(score(np.zeros((0, 3)), [], np.zeros((0, 3)), []).values()) == {0}
    # the level is a maximum over atoms, not a sum: the same atom twice is the atom once
    assert score([[0, 0, 0], [0, 0, 0]], [C, C], [[0, 0, 0]], [C])['vol_a'] == 431
    assert shape_ref.first_maximum([[0, 1, 1], [2, 2, 2], [0, 0, 3], [-1, -2, -3]]).tolist() == [1, 0, 2, 0]


def test_atom_cubes_equal_the_dense_evaluation_and_symmetries():
    rng = np.random.default_rng(3)
    xa = rng.uniform(-3, 3, size=(12, 3)).astype(np.float32) + np.float32([40.25, -17.5, 3.0])
    xb = (xa[:9] + rng.normal(0, 0.4, size=(9, 3))).astype(np.float32)
    xa[0], xb[0] = np.round(xa[0] * 2) / 2, np.round(xb[0] * 2) / 2 + 0.25        # on a lattice point, on a half-spacing
    ta, tb = rng.integers(0, 9, 12), rng.integers(0, 9, 9)
    got = score(xa, ta, xb, tb)
    assert got == score(xa, ta, xb, tb, dense=True) and 0 < got['vol_min'] < min(got['vol_a'], got['vol_b'])
    wide = shape_ref.radius_table(9, 1.0, 0.5)
    assert score(xa, ta, xb, tb, r2=wide) == score(xa, ta, xb, tb, r2=wide, dense=True)
    assert score(xa, ta, xb, tb, r2=wide)['vol_a'] > got['vol_a']
    same = score(xa, ta, xa, ta)
    assert same['vol_min'] == same['vol_a'] == same['vol_b'] and same['core_both'] == same['core_a'] == same['core_b']
    swapped = score(xb, tb, xa, ta)
    assert (swapped['vol_a'], swapped['vol_b'], swapped['core_a'], swapped['core_b'], swapped['n_a'], swapped['n_b']) == \
        (got['vol_b'], got['vol_a'], got['core_b'], got['core_a'], got['n_b'], got['n_a'])
    assert (swapped['vol_min'], swapped['core_both']) == (got['vol_min'], got['core_both'])
    # masked rows are not looked at, whatever they hold
    x = np.concatenate([xa, np.full((2, 3), np.nan, np.float32)])[None]
    mask = np.concatenate([np.ones(12), np.zeros(2)])[None]
    one_hot = np.concatenate([EYE[ta], np.full((2, 9), np.nan, np.float32)])[None]
    masked = shape_ref.shape_scores(x, one_hot, mask, xb[None], EYE[tb][None], np.ones((1, 9)))
    assert {k: int(v[0]) for k, v in masked.items()} == got


def test_flags_and_their_order():
    nan, inf = float('nan'), float('inf')
    zero = dict(vol_a=0, vol_b=0, vol_min=0, core_a=0, core_b=0, core_both=0, n_a=0, n_b=0)
    assert (shape_ref.NONFINITE, shape_ref.OUT_OF_RANGE, shape_ref.TOO_LARGE) == (1, 2, 4)
    assert score([[0, nan, 0]], [C], [[1, 0, 0]], [O]) == dict(zero, status=1)
    assert score([[0, 0, 0]], [C], [[1, 0, -inf]], [O]) == dict(zero, status=1)
    assert score([[0, 5000, 0]], [C], [[1, 0, 0]], [O]) == dict(zero, status=2)
    assert score([[0, 0, 0]], [C], [[0, 0, -4096.5]], [O]) == dict(zero, status=2)
    assert score([[0, 0, 4096]], [C], [[0, 0, 4095]], [O])['status'] == 0, 'the limit itself is in range'
    # in this order: a NaN before a far coordinate, a far coordinate before the extent
    assert score([[5000, 0, 0]], [C], [[nan, 0, 0]], [O])['status'] == 1
    assert score([[inf, 0, 0]], [C], [[1, 0, 0]], [O])['status'] == 1, 'an infinity is not finite before it is far'
    assert score([[5000, 0, 0]], [C], [[0, 0, 0]], [O])['status'] == 2, 'and 5000 A apart is out of range, not too large'
    # the extent: floor(2 * x) over both molecules, hi - lo = 240 is scored, 241 is flagged
    for axis in range(3):
        a, b = np.zeros(3), np.zeros(3)
        a[axis], b[axis] = -60.0, 60.25                                 # cells -120 and 120
        got = score([a], [C], [b], [O])
        alone = score(np.zeros((0, 3)), [], [b], [O])['vol_b']
        assert (got['status'], got['vol_a'], got['vol_b'], got['vol_min']) == (0, 431, alone, 0) and alone > 300
        b[axis] = 60.5                                                  # cell 121
        assert score([a], [C], [b], [O]) == dict(zero, status=4)
        assert score([a, b], [C, O], np.zeros((0, 3)), []) == dict(zero, status=4), 'both molecules count, and one alone does'
    # a flagged pair leaves its neighbours alone
    x_a = np.float32([[[0, 0, 0]], [[nan, 0, 0]], [[0, 0, 0]]])
    x_b = np.float32([[[1, 0, 0]], [[1, 0, 0]], [[1, 0, 0]]])
    got = shape_ref.shape_scores(x_a, EYE[[[C]] * 3], np.ones((3, 1)), x_b, EYE[[[O]] * 3], np.ones((3, 1)))
    assert got['status'].tolist() == [0, 1, 0] and got['vol_min'].tolist() == [196, 0, 196] and got['n_a'].tolist() == [1, 0, 1]


def test_radius_table():
    from difflinker_amd import const
    geom, zinc = const.shape_radius_table(True), const.shape_radius_table(False)
    assert geom.shape == (9, 3) and zinc.shape == (8, 3) and geom.dtype == torch.float32 and torch.equal(geom[:8], zinc)
    assert geom[0].tolist() == [np.float32(1.8496001), np.float32(2.5921001), np.float32(3.4596)]
    assert np.array_equal(geom.numpy(), shape_ref.radius_table(9)) and shape_ref.VDW == const.VDW_RADII
    for t in range(9):
        for k in range(3):
            r = np.float32(0.8 * const.VDW_RADII[t] + k * 0.25)
            assert geom[t, k].item() == r * r, (t, k)
    other = const.shape_radius_table(True, scale=1.0, step=0.5)
    assert np.array_equal(other.numpy(), shape_ref.radius_table(9, 1.0, 0.5))
    assert other[7].tolist() == [np.float32(1.98) ** 2, np.float32(2.48) ** 2, np.float32(2.98) ** 2]


def test_export_declared_checked_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    assert 'int32_t dl_shape_scores(const dl_shape_args* args, void* stream);' in header and hasattr(lib, 'dl_shape_scores')
    at = _lib.EXPORTS.index('dl_clash_scores')
    assert _lib.EXPORTS[at + 1] == 'dl_shape_scores' and _lib.EXPORTS[-1] == 'dl_best_rmsd', 'right after dl_clash_scores'
    assert ' *   dl_shape_scores ' in header.split('#ifndef DIFFLINKER_HIP_H')[0], 'listed in the opening comment'
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7 and '#define DL_ABI_VERSION 7' in header
    for name, bit in (('DL_SHAPE_NONFINITE', 1), ('DL_SHAPE_OUT_OF_RANGE', 2), ('DL_SHAPE_TOO_LARGE', 4)):
        assert f'#define {name} {bit} ' in header and getattr(_lib, name) == bit
    # the struct's fields in the header's order
    body = header.split('typedef struct dl_shape_args {')[1].split('} dl_shape_args;')[0]
    declared = [part.strip(' *') for line in body.splitlines() if ';' in line
                for part in line.split(';')[0].split(None, 1 + line.strip().startswith('const'))[-1].split(',')]
    assert declared == [name for name, _ in _lib.DLShapeArgs._fields_]
    assert declared == ['B', 'Na', 'Nb', 'nf', 'x_a', 'one_hot_a', 'mask_a', 'x_b', 'one_hot_b', 'mask_b', 'r2'] + list(shape_ref.FIELDS)
    # no GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1) before any device work
    assert lib.dl_shape_scores(None, None) == -1
    one = ctypes.c_void_p(16)                    # never dereferenced
    pointers = declared[4:]
    ok = dict(B=2, Na=8, Nb=11, nf=9, **{k: one for k in pointers})
    refusals = [dict(B=-1), dict(Na=0), dict(Nb=0), dict(Na=-3), dict(nf=0), dict(nf=17)]
    for bad in refusals + [{k: None} for k in pointers]:
        assert lib.dl_shape_scores(ctypes.byref(_lib.DLShapeArgs(**dict(ok, **bad))), None) == -1, bad
    empty = _lib.DLShapeArgs(B=0, Na=8, Nb=11, nf=9)
    assert lib.dl_shape_scores(ctypes.byref(empty), None) == _lib.DL_OK, 'an empty batch is DL_OK without a launch'
    for field, value in (('Na', 0), ('Nb', 0), ('nf', 17)):
        worse = _lib.DLShapeArgs(B=0, Na=8, Nb=11, nf=9)
        setattr(worse, field, value)
        assert lib.dl_shape_scores(ctypes.byref(worse), None) == -1, 'the sizes are checked before the empty batch'


def record(vol_a=400, vol_b=500, vol_min=300, status=0, n_a=5, n_b=6):
    from difflinker_amd.metrics import ShapeRecord
    return ShapeRecord(vol_a, vol_b, vol_min, 0, 0, 0, n_a, n_b, status)


def molecule(n_over=0, n_components=1, status=0):
    from difflinker_amd.metrics import Molecule
    fields = dict.fromkeys(Molecule._fields)
    fields.update(n_over=n_over, n_components=n_components, status=status)
    return Molecule(**fields)


def test_compute_shapes_on_hand_written_records():
    from difflinker_amd.metrics import SHAPE_NAMES, compute_shapes
    records = [record(400, 500, 300),                                   # similarity 0.75, tanimoto 300 / 600
               record(1000, 1000, 1000),                                # 1.0, 1.0
               record(500, 100, 50),                                    # 0.1, 50 / 550
               record(0, 0, 0, status=1),                               # flagged: out of everything
               record(0, 700, 0, n_a=0),                                # no volume of its own: not scored, not flagged
               record(800, 800, 680)]                                   # 0.85, 680 / 920
    got = compute_shapes(records)
    assert tuple(got) == SHAPE_NAMES
    assert got == {'shape_molecules': 4, 'shape_flagged': 1, 'shape_similarity': (0.75 + 1.0 + 0.1 + 0.85) / 4,
                   'shape_tanimoto': (300 / 600 + 1.0 + 50 / 550 + 680 / 920) / 4,
                   'shape_similarity_7': 75.0, 'shape_similarity_8': 50.0, 'shape_similarity_9': 25.0}
    assert type(got['shape_molecules']) is int and type(got['shape_similarity']) is float
    assert compute_shapes([record(700, 900, 490)])['shape_similarity_7'] == 0.0, 'above 0.7, not at it'
    linker = [record(100, 100, 50), record(0, 50, 0), record(80, 80, 80), record(0, 0, 0, status=2), record(60, 60, 0),
              record(10, 10, 10)]
    with_linker = compute_shapes(records, linker)
    assert tuple(with_linker) == SHAPE_NAMES + ('shape_tanimoto_linker',) and {k: with_linker[k] for k in SHAPE_NAMES} == got
    assert with_linker['shape_tanimoto_linker'] == (50 / 150 + 1.0 + 0.0 + 1.0) / 4
    pred = [molecule(), molecule(n_over=1), molecule(), molecule(), molecule(), molecule(n_components=2)]
    with_pred = compute_shapes(records, linker, pred)
    assert tuple(with_pred) == SHAPE_NAMES + ('shape_tanimoto_linker', 'shape_tanimoto_valid')
    assert with_pred['shape_tanimoto_valid'] == (300 / 600 + 50 / 550) / 2, 'scored pairs whose sample is valid and in one piece'
    assert compute_shapes(records, pred=[molecule(status=1)] * 6)['shape_tanimoto_valid'] is None
    nothing = {'shape_molecules': 0, 'shape_flagged': 0, 'shape_similarity': None, 'shape_tanimoto': None,
               'shape_similarity_7': None, 'shape_similarity_8': None, 'shape_similarity_9': None}
    assert compute_shapes([]) == nothing
    assert compute_shapes([], [], []) == dict(nothing, shape_tanimoto_linker=None, shape_tanimoto_valid=None)
    flagged = compute_shapes([record(0, 0, 0, status=1), record(0, 0, 0, status=4)], [record(0, 0, 0, status=1)] * 2)
    assert flagged == dict(nothing, shape_flagged=2, shape_tanimoto_linker=None)
    with pytest.raises(ValueError):
        compute_shapes(records, pred=pred[:2])


def test_cpu_tensors_raise():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import analyze_shapes
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_shapes(torch.zeros(1, 4, 9), torch.zeros(1, 4, 3), torch.ones(1, 4), torch.zeros(1, 5, 9), torch.zeros(1, 5, 3),
                       torch.ones(1, 5))


def test_drivers_parse_the_shape_flag(monkeypatch, capsys):
    from difflinker_amd import sample, train
    from difflinker_amd.lightning import DDPM
    assert inspect.signature(sample.sample).parameters['shape'].default is False
    seen = []
    monkeypatch.setattr(sample, 'sample', lambda *a, **kw: seen.append(kw))
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--shape'])
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p'])
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--shape', '--metrics', '--geometry'])
    assert seen == [{'shape': True}, {}, {'geometry': True, 'shape': True}], 'without the flag the call is what it was'
    for driver in (sample, train):
        with pytest.raises(SystemExit):
            driver.main(['--help'])
        assert '--shape' in capsys.readouterr().out
    assert 'self.shape_metrics = False' in inspect.getsource(DDPM.__init__)
    assert 'model.shape_metrics = bool(a.shape)' in inspect.getsource(train.main)
