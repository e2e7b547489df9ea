"""The internal-geometry checks on the GPU (``dl_pose_checks``, ``csrc/pose_checks.hip``) against the plain-Python rule of
``tests/pose_checks_ref.py``.  The C entry point is called on outputs pre-filled with 0x5a bytes, so an element it should write
and does not shows, and EVERY output byte is compared with the reference: the outputs are integers decided by fp64
comparisons that both sides round identically, so there is no tolerance anywhere in this file.  The public path
(``analyze_pose_checks``, ``sample``, ``generate``, ``DDPM.pose_metrics``) comes last; the launch on a side stream is in
``tests/test_gpu_streams_pose_checks.py``, collected after the stream harness it uses."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import pose_checks_ref as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL = 0x5a5a5a5a
OPTIONAL = ('drop', 'mark', 'planar', 'status')


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def batch_of(molecules, N, capacity=None, seed=0, scatter=True, status=None, n_in=None, nf=8):
    batch = pr.as_batch(molecules, N, capacity, nf=nf, rng=np.random.default_rng(seed), scatter=scatter)
    batch['status_in'] = np.zeros(len(molecules), np.int32) if status is None else np.asarray(status, np.int32)
    if n_in is not None:
        batch['n_bonds_in'] = np.asarray(n_in, np.int32)
    return batch


def launch(batch, tables=None, drop=True, mark=True, planar=True, status=True, stream=None):
    """The C entry point on outputs full of 0x5a bytes: a dict of numpy arrays by the names of ``pose_checks_ref.FIELDS``."""
    from difflinker_amd import _lib
    B, N = batch['node_mask'].shape
    nf, capacity = batch['one_hot'].shape[2], batch['bonds'].shape[1]
    bounds2, cosines, clashes2 = tables or pr.default_tables(nf)
    held = [dev(batch['x']), dev(batch['one_hot']), dev(batch['node_mask']), dev(batch['drop_mask']), dev(batch['mark_mask']),
            dev(batch['atom_planar'], torch.int32), dev(bounds2, torch.float64), dev(cosines, torch.float64),
            dev(clashes2, torch.float64), dev(batch['n_bonds_in'], torch.int32), dev(batch['bonds'], torch.int32),
            dev(batch['status_in'], torch.int32)]
    x, one_hot, mask, drop_t, mark_t, planar_t, bounds_t, cos_t, clash_t, n_in, bonds, status_in = held
    assert bounds_t.shape == (nf, nf, 3, 2) and cos_t.shape == (3, 2) and clash_t.shape == (nf, nf)
    shapes = {'counts': (B, 2, 8), 'atom_flags': (B, N)}
    out = {name: torch.full(shapes.get(name, (B,)), FILL, dtype=torch.int32, device=DEV) for name in pr.FIELDS}
    args = _lib.DLPoseArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
        drop_mask=drop_t.data_ptr() if drop else None, mark_mask=mark_t.data_ptr() if mark else None,
        atom_planar=planar_t.data_ptr() if planar else None, length_bounds2=bounds_t.data_ptr(), angle_cos=cos_t.data_ptr(),
        clash2=clash_t.data_ptr(), capacity=capacity, n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr() if bonds.numel() else None,
        status_in=status_in.data_ptr() if status else None, counts=out['counts'].data_ptr(),
        atom_flags=out['atom_flags'].data_ptr(), status=out['status'].data_ptr())
    args.stream = (torch.cuda.current_stream(torch.device(DEV)) if stream is None else stream).cuda_stream
    _lib.check(_lib.load().dl_pose_checks(ctypes.byref(args)), 'dl_pose_checks')
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def reference(batch, tables=None, drop=True, mark=True, planar=True, status=True):
    tables = tables or pr.default_tables(batch['one_hot'].shape[2])
    return pr.pose_checks(batch['x'], batch['one_hot'], batch['node_mask'], batch['bonds'], batch['n_bonds_in'], *tables,
                          batch['status_in'] if status else None, batch['drop_mask'] if drop else None,
                          batch['mark_mask'] if mark else None, batch['atom_planar'] if planar else None)


def same_bits(a, b):
    return all(a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes() for name in pr.FIELDS)


def check(batch, tables=None, **kwargs):
    got, want = launch(batch, tables, **kwargs), reference(batch, tables, **kwargs)
    for name in pr.FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.int32
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5].tolist(),
                                                       got[name][got[name] != want[name]][:5], want[name][got[name] != want[name]][:5])
        assert got[name].tobytes() == want[name].tobytes()
    return got


def row(batch, b):
    return {key: value[b:b + 1] for key, value in batch.items()}


NAMES = sorted(pr.HAND)
EMPTY = dict(types=[], points=[], entries=[], planar=[], marked=[], dropped=[])


@pytest.fixture(scope='module')
def hand():
    return batch_of([pr.hand_molecule(name) for name in NAMES] + [EMPTY], 12)


@pytest.fixture(scope='module')
def random_batch():
    rng = np.random.default_rng(23)
    molecules = [pr.random_molecule(rng) for _ in range(200)]
    batch = batch_of(molecules, 64, seed=24, status=rng.choice([0, 0, 2, 16], 200))
    return batch


@pytest.fixture(scope='module')
def random_reference(random_batch):
    """Computed once and shared; no test writes to it."""
    return {key: reference(random_batch, **dict(zip(OPTIONAL, key))) for key in ((True,) * 4, (False,) * 4)}


# ---- every rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_hand_molecule_alone(name):
    m = pr.hand_molecule(name)
    got = check(batch_of([m], len(m['types']), scatter=False))
    assert got['counts'][0, 0].tolist() == pr.HAND[name][4] and not got['counts'][0, 1].any() and got['status'][0] == 0
    if name in pr.CLEAN:
        assert not got['atom_flags'].any()


def test_hand_molecules_in_one_ragged_batch(hand):
    got = check(hand)
    for b, name in enumerate(NAMES):
        assert got['counts'][b, 0].tolist() == pr.HAND[name][4], name
    assert not got['counts'][-1].any() and got['status'][-1] == 0, 'the molecule with no real row'
    check(hand, drop=False, mark=False, planar=False, status=False)
    everyone = dict(hand, mark_mask=np.ones_like(hand['mark_mask']))
    got = check(everyone)
    assert np.array_equal(got['counts'][:, 0], got['counts'][:, 1]), 'every atom marked: the two rows agree'


@pytest.mark.parametrize('name', sorted(pr.ties()))
def test_ties(name):
    m, tables, want = pr.ties()[name]
    got = check(batch_of([m], 5, seed=3), tables)
    assert got['counts'][0, 0].tolist() == want


def test_the_lower_numbered_atom_indexes_the_tables_first():
    """Tables that are not symmetric: a C-O bond looks up [C][O] when the carbon has the lower number and [O][C] otherwise."""
    nf = 8
    bounds = pr.flat_bounds(nf, 0.25, 16.0)
    bounds[pr.C][pr.O][0] = [0.25, 1.0]                          # C before O: long
    clash = [[0.0] * nf for _ in range(nf)]
    clash[pr.O][pr.C] = 100.0                                    # O before C: a clash
    tables = (bounds, [[-2.0, 2.0]] * 3, clash)
    points = [(0.0, 0.0, 0.0), (1.25, 0.0, 0.0)]
    molecules = [dict(EMPTY, types=[pr.C, pr.O], points=points, entries=[(1, 0, 1)]),
                 dict(EMPTY, types=[pr.O, pr.C], points=points, entries=[(0, 1, 1)]),
                 dict(EMPTY, types=[pr.C, pr.O], points=points), dict(EMPTY, types=[pr.O, pr.C], points=points)]
    got = check(batch_of(molecules, 4), tables)
    assert got['counts'][:, 0, pr.LONG].tolist() == [1, 0, 0, 0] and got['counts'][:, 0, pr.CLASHES].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize('nf', [1, 16, 17])
def test_vocabularies_on_both_sides_of_the_staged_clash_table(nf):
    """The kernel keeps ``clash2`` in LDS up to 16 types and reads it in place beyond: random tables for 1, 16 and 17 types."""
    rng = np.random.default_rng(nf)
    molecules = [pr.random_molecule(rng, max_atoms=30, min_atoms=5) for _ in range(12)]
    for m in molecules:
        m['types'] = [int(t) for t in rng.integers(0, nf, len(m['types']))]
    bounds = rng.uniform(0.5, 3.0, (nf, nf, 3, 1)) * np.array([1.0, 2.0])
    bounds[rng.random((nf, nf, 3)) < 0.2] = 0.0
    clash = rng.uniform(2.0, 9.0, (nf, nf))
    clash[rng.random((nf, nf)) < 0.2] = 0.0
    got = check(batch_of(molecules, 32, seed=nf, nf=nf), (bounds.tolist(), pr.angle_cos(), clash.tolist()))
    assert got['counts'][:, 0, pr.CLASHES].sum() > 20 and got['counts'][:, 0, pr.UNTABLED].sum() > 5


@pytest.mark.parametrize('options', [(True,) * 4, (False,) * 4])
def test_random_molecules(random_batch, random_reference, options):
    kwargs = dict(zip(OPTIONAL, options))
    got, want = launch(random_batch, **kwargs), random_reference[options]
    assert same_bits(got, want), [(name, np.argwhere(got[name] != want[name])[:5].tolist()) for name in pr.FIELDS]
    totals = want['counts'][:, 0].sum(axis=0)
    assert (totals > 100).all(), ('every count is exercised', totals.tolist())
    assert random_batch['node_mask'].shape == (200, 64) and 1 <= random_batch['node_mask'].sum(axis=1).min() <= 40
    assert np.isnan(random_batch['x']).any() and not (want['status'] & pr.NONFINITE).any(), 'NaN on unreal rows only'
    assert len({f for f in want['atom_flags'].ravel().tolist()}) == 8, 'every combination of flags'
    if options[1]:
        assert (want['counts'][:, 1] > 0).any() and (want['counts'][:, 1] <= want['counts'][:, 0]).all()
        assert (want['counts'][:, 1] < want['counts'][:, 0]).any()


def test_one_option_at_a_time(random_batch):
    few = {key: value[:40] for key, value in random_batch.items()}
    for name in OPTIONAL:
        check(few, **{name: False})


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def test_the_first_far_pair_and_the_smallest_molecules():
    molecules = [dict(pr.chain(n), marked=[0] if n else []) for n in (0, 1, 2, 4, 5)]
    got = check(batch_of(molecules, 7, seed=2))
    assert got['counts'][:, 0, pr.PAIRS].tolist() == [0, 0, 0, 0, 1] and got['counts'][:, 1, pr.PAIRS].tolist() == [0, 0, 0, 0, 1]
    assert got['counts'][:, 0, pr.CHECKED].tolist() == [0, 0, 1, 3, 4] and got['counts'][:, 0, pr.ANGLES].tolist() == [0, 0, 0, 2, 3]
    got = check(batch_of([pr.chain(1), EMPTY], 1, capacity=0))
    assert not got['counts'].any() and not got['status'].any()


def test_the_word_boundary_of_the_ball():
    molecules = [pr.chain(n) for n in (63, 64, 65)] + [dict(pr.chain(65), dropped=[0, 64]), dict(pr.chain(130), dropped=[63, 64])]
    got = check(batch_of(molecules, 140, seed=6))
    for b, n in enumerate((63, 64, 65, 63)):
        assert got['counts'][b, 0, pr.PAIRS] == n * (n - 1) // 2 - (n - 1) - (n - 2) - (n - 3)
    assert got['counts'][:, 0, pr.CLASHES].min() > 0, 'the folds bring far atoms close'
    # a hub on each side of the boundary: atoms 62..66 all bonded to 63 and to 64
    star = pr.chain(70)
    star['entries'] = [e for e in star['entries'] if e[0] < 60] + [(63, k, 1) for k in (60, 61, 62, 64)] + [(64, k, 1) for k in (65, 66, 67, 68)]
    check(batch_of([star], 70, scatter=False))


def test_the_atom_limit_and_wide_rows():
    fits, over = pr.chain(256), pr.chain(257)
    over['entries'] = over['entries'] + [(5, 5, 1)]
    nearly = pr.chain(255)
    batch = batch_of([pr.hand_molecule('benzene'), over, fits, dict(over, dropped=[100]), nearly], 300, seed=4, status=[0, 2, 0, 0, 0])
    got = check(batch)
    assert got['status'].tolist() == [0, 2 | pr.TOO_LARGE, 0, pr.BAD_BOND, 0], 'too large: the list is not looked at'
    assert not got['counts'][1].any() and not got['atom_flags'][1].any()
    assert got['counts'][:, 0, pr.CHECKED].tolist() == [6, 0, 255, 254, 254]
    assert got['counts'][2, 0, pr.PAIRS] == 256 * 255 // 2 - 255 - 254 - 253
    got = check(batch_of([pr.hand_molecule('folded_chain'), fits], 1024, seed=5))
    assert got['counts'][:, 0, pr.CHECKED].tolist() == [4, 255] and not got['status'].any(), 'N = 1024 with 5 real rows, and with 256'


# ---- lists ---------------------------------------------------------------------------------------------------------------------
def test_no_list_and_short_lists():
    m = pr.hand_molecule('folded_chain')
    got = check(batch_of([m, m], 6, capacity=0, n_in=[4, 0]))
    assert got['status'].tolist() == [pr.BONDS_OVERFLOW, 0] and got['counts'][:, 0].tolist() == [[0, 0, 0, 0, 0, 0, 10, 10]] * 2
    batch = batch_of([m] * 4, 6, capacity=2, n_in=[5, -3, 1, 2], status=[2, 0, 0, 18])
    got = check(batch)
    assert got['status'].tolist() == [2 | pr.BONDS_OVERFLOW, 0, 0, 18] and got['counts'][:, 0, pr.CHECKED].tolist() == [2, 0, 1, 2]
    got = check(batch, status=False)
    assert got['status'].tolist() == [pr.BONDS_OVERFLOW, 0, 0, 0], 'a null status_in carries nothing'


def test_bad_and_repeated_entries():
    m = pr.hand_molecule('folded_chain')
    wrong = [(0, 1, 0), (0, 1, 4), (2, 2, 1), (-1, 2, 1), (2, 5, 1)]
    molecules = [dict(m, entries=m['entries'] + [w]) for w in wrong]
    molecules.append(dict(m, entries=m['entries'] + [(0, 1, 3)]))                 # the first entry's order counts
    molecules.append(dict(m, entries=[(0, 1, 3)] + m['entries']))
    molecules.append(dict(m, entries=wrong + [(0, 1, 2)] + m['entries'] + [(1, 0, 3), (3, 4, 3)]))
    molecules.append(dict(m, entries=m['entries'] + [(2, 1, 1)], dropped=[2]))     # repeated, but no bond of the kept graph
    molecules.append(m)
    got = check(batch_of(molecules, 7, seed=8))
    assert got['status'].tolist() == [pr.BAD_BOND] * 8 + [0, 0]
    assert got['counts'][:, 0, pr.LONG].tolist() == [0] * 6 + [1, 0, 0, 0], 'as a triple bond 1.54 A is long'
    assert got['counts'][6, 0, pr.ANGLES:pr.ANGLES + 2].tolist() == [3, 1], 'and its neighbour is a linear centre at 108 degrees'


def test_shuffled_and_turned_lists_give_the_same_bits(random_batch):
    rng = np.random.default_rng(9)
    few = {key: value[:60].copy() for key, value in random_batch.items()}
    base = launch(few)
    for b in range(60):
        n = int(few['n_bonds_in'][b])
        rows = few['bonds'][b, :n][rng.permutation(n)]
        turn = rng.random(n) < 0.5
        rows[turn] = rows[turn][:, [1, 0, 2]]
        few['bonds'][b, :n] = rows
    assert same_bits(launch(few), base) and same_bits(reference(few), base)


def test_a_nan_coordinate_stays_in_its_molecule():
    m = pr.hand_molecule('folded_chain')
    molecules = []
    for value in (float('nan'), float('inf'), -float('inf')):
        bad = [list(p) for p in m['points']]
        bad[2][1] = value
        molecules += [dict(m, points=bad), dict(m, points=bad, dropped=[2])]
    got = check(batch_of(molecules + [dict(m, entries=m['entries'] + [(9, 9, 9)], points=molecules[0]['points']), m], 6, seed=1))
    assert got['status'].tolist() == [pr.NONFINITE, 0] * 3 + [pr.NONFINITE | pr.BAD_BOND, 0]
    assert not got['counts'][[0, 2, 4, 6]].any() and not got['atom_flags'][[0, 2, 4, 6]].any()
    assert got['counts'][-1, 0].tolist() == pr.HAND['folded_chain'][4] and got['counts'][1, 0].tolist() == [2, 0, 0, 0, 0, 0, 4, 4]


def test_an_empty_batch_and_bad_arguments():
    from difflinker_amd import _lib
    batch = batch_of([pr.chain(3)], 3)
    got = launch({key: value[:0] for key, value in batch.items()})
    assert all(got[name].shape[0] == 0 for name in pr.FIELDS)
    lib = _lib.load()
    assert lib.dl_pose_checks(None) != _lib.DL_OK
    for more in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict()):
        args = _lib.DLPoseArgs(**dict(dict(B=1, N=4, nf=8, capacity=0), **more))      # every pointer null
        assert lib.dl_pose_checks(ctypes.byref(args)) != _lib.DL_OK, more


# ---- determinism and independence --------------------------------------------------------------------------------------------
def test_two_launches_give_equal_bits(random_batch, hand):
    for batch in (random_batch, hand):
        assert same_bits(launch(batch), launch(batch))


def test_each_molecule_alone_equals_its_row(random_batch):
    ragged = {key: value[[0, 9, 22, 41, 63, 150]] for key, value in random_batch.items()}
    whole = launch(ragged)
    assert len(set(ragged['node_mask'].sum(axis=1).tolist())) > 1
    for b in range(6):
        alone = launch(row(ragged, b))
        for name in pr.FIELDS:
            assert alone[name][0].tobytes() == whole[name][b].tobytes(), (name, b)


# ---- the public path ---------------------------------------------------------------------------------------------------------
def public_batch():
    import aromatic_ref as ar
    types, points, _ = ar.hand_molecule('benzene')
    benzene = dict(EMPTY, types=list(types), points=[tuple(p) for p in points], marked=[0, 1])
    # what bond perception must not close: five atoms on a circle whose ends are 1.95 A apart, and two ethanes 2 A apart
    turn = [(1.31 * np.cos(np.radians(66 * k)), 1.31 * np.sin(np.radians(66 * k)), 0.0) for k in range(5)]
    fold = dict(EMPTY, types=[pr.C] * 5, points=turn)
    pieces = dict(EMPTY, types=[pr.C] * 4, points=[(0, 0, 0), (1.54, 0, 0), (0, 2.0, 0), (1.54, 2.0, 0)])
    named = lambda name: dict(pr.hand_molecule(name), entries=[])      # noqa: E731
    molecules = [benzene] + [dict(m, marked=[0]) for m in (named('butane'), fold, named('bent_nitrile'), pieces, named('sulfone'),
                                                           named('compressed_bond'))]
    molecules.append(dict(pr.hand_molecule('hexane'), entries=[], dropped=[5], marked=[2, 3]))
    batch = batch_of(molecules, 9, capacity=0, seed=2)
    batch['x'] = np.nan_to_num(batch['x'])
    return batch


def through_the_reference_chain(batch, one_hot, x, mask, drop, linker):
    """Bond perception and refinement on the device (each is compared with its own reference elsewhere), the checks by the rule."""
    from difflinker_amd.molecule_builder import perceive_bonds, refine_bond_orders
    found = perceive_bonds(one_hot, x, mask, False)
    refined, aromatic = refine_bond_orders(found, one_hot, x, mask, False, drop, linker)
    want = pr.pose_checks(batch['x'], batch['one_hot'], batch['node_mask'], refined.bonds.cpu().numpy(), refined.n_bonds.cpu().numpy(),
                          *pr.default_tables(), aromatic.status.cpu().numpy(), batch['drop_mask'], batch['mark_mask'],
                          aromatic.atom_aromatic.cpu().numpy())
    return refined, aromatic, want


def test_the_wrapper_against_the_reference_chain():
    from difflinker_amd.metrics import PoseChecks, PoseRecord, analyze_pose_checks, compute_pose_checks, pose_checks_to_host
    batch = public_batch()
    one_hot, x, mask = dev(batch['one_hot']), dev(batch['x']), dev(batch['node_mask']).unsqueeze(2)
    drop, linker = dev(batch['drop_mask']), dev(batch['mark_mask']).unsqueeze(2)
    got = analyze_pose_checks(one_hot, x, mask, False, linker, drop_mask=drop)
    assert isinstance(got, PoseChecks) and got._fields == ('counts', 'atom_flags', 'status', 'refined', 'aromatic')
    refined, aromatic, want = through_the_reference_chain(batch, one_hot, x, mask, drop, linker.squeeze(2))
    assert aromatic.n_aromatic_rings.tolist() == [1] + [0] * 7 and refined.n_bonds.tolist() == [6, 3, 4, 2, 2, 4, 1, 5]
    for name in pr.FIELDS:
        assert getattr(got, name).dtype == torch.int32 and np.array_equal(getattr(got, name).cpu().numpy(), want[name]), name
    bad = got.counts[:, 0, [pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES]].sum(dim=1).tolist()
    assert [b > 0 for b in bad] == [False, False, True, True, True, False, True, False] and not got.status.any()
    assert got.counts[7, 0, pr.CHECKED] == 4 and got.counts[7, 1, pr.CHECKED] == 3, 'the pocket atom is dropped, the linker marked'
    records = pose_checks_to_host(got)
    assert all(isinstance(r, PoseRecord) for r in records) and [r.counts for r in records] == [tuple(c) for c in want['counts'][:, 0].tolist()]
    assert [r.n_flagged_atoms for r in records] == (want['atom_flags'] != 0).sum(axis=1).tolist()
    scores = compute_pose_checks(records)
    assert scores['pose_valid'] == 0.5 and scores['bond_lengths_valid'] == 7 / 8 and scores['bond_angles_valid'] == 7 / 8
    assert scores['internal_clash_free'] == 6 / 8 and scores['internal_clashes_per_molecule'] == 5 / 8
    looser = analyze_pose_checks(one_hot, x, mask, False, linker, drop_mask=drop, length_bounds=(0.4, 1.6), angle_tolerance=65.0,
                                 clash_scale=0.4)
    assert looser.counts[:, 0, [pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES]].sum().item() == 0
    assert torch.equal(looser.counts[:, :, [pr.CHECKED, pr.ANGLES, pr.PAIRS]], got.counts[:, :, [pr.CHECKED, pr.ANGLES, pr.PAIRS]])


def test_input_forms_give_the_same_bits():
    from difflinker_amd.metrics import analyze_pose_checks, pose_checks
    from difflinker_amd.molecule_builder import Bonds
    batch = public_batch()
    one_hot, x, mask = dev(batch['one_hot']), dev(batch['x']), dev(batch['node_mask']).unsqueeze(2)
    drop, linker = dev(batch['drop_mask']), dev(batch['mark_mask'])
    base = analyze_pose_checks(one_hot, x, mask, False, linker, drop_mask=drop)
    wide = lambda t, dtype: torch.stack([t.to(dtype), t.to(dtype)], dim=-1)[..., 0]      # noqa: E731  (strided)
    sliced = lambda t: torch.cat([t, t], dim=1)[:, :t.shape[1]]                          # noqa: E731  (a slice of a wider tensor)
    got = analyze_pose_checks(wide(one_hot, torch.float64), sliced(wide(x, torch.float64)), wide(mask[:, :, 0], torch.float64), False,
                              sliced(linker).to(torch.int8), drop_mask=wide(drop, torch.float64).unsqueeze(2))
    torch.cuda.synchronize()
    for name in pr.FIELDS:
        assert torch.equal(getattr(got, name), getattr(base, name)), name
    refined = base.refined
    padded = torch.cat([refined.bonds, torch.full_like(refined.bonds, 7)], dim=1)
    forms = Bonds(wide(refined.n_bonds, torch.int64), padded.long()[:, :refined.bonds.shape[1]], None, None, None,
                  wide(base.aromatic.status, torch.int64))
    counts, flags, status = pose_checks(wide(one_hot, torch.float64), wide(x, torch.float64), mask[:, :, 0], forms, False,
                                        drop_mask=drop, mark_mask=wide(linker, torch.float64),
                                        atom_planar=wide(base.aromatic.atom_aromatic, torch.int64))
    assert torch.equal(counts, base.counts) and torch.equal(flags, base.atom_flags) and torch.equal(status, base.status)
    with pytest.raises(ValueError, match='shapes disagree'):
        analyze_pose_checks(one_hot, x, mask, False, linker[:, :5])
    with pytest.raises(ValueError, match='shapes disagree'):
        pose_checks(one_hot, x[:, :5], mask, refined, False)


def pose_keys(with_true):
    from difflinker_amd.metrics import POSE_NAMES
    return set(POSE_NAMES) | ({'true_' + name for name in POSE_NAMES} if with_true else set())


def check_scores(got, with_true):
    for key in pose_keys(with_true):
        assert got[key] is None or got[key] >= 0.0, key
        if 'valid' in key or 'free' in key:
            assert got[key] is None or got[key] <= 1.0, key
    assert got['pose_valid'] <= min(got['bond_lengths_valid'], got['bond_angles_valid'], got['internal_clash_free'])
    json.dumps(got)


def test_sample_writes_the_keys_only_when_asked(tmp_path):
    from difflinker_amd.metrics import METRIC_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_rings import gentle_model
    m = gentle_model(tmp_path, False)
    m.edm.noise_seed = 5
    out = sample(m, str(tmp_path / 'new'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, pose_checks=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | pose_keys(True)
    check_scores(got, True)
    m.edm.noise_seed = 5
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    before = json.load(open(os.path.join(plain, 'metrics.json')))
    assert set(before) == set(METRIC_NAMES) | {'molecules'} and before == {k: got[k] for k in before}, 'unchanged without the flag'
    m.edm.noise_seed = 5
    alone = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, pose_checks=True)
    assert json.load(open(os.path.join(alone, 'metrics.json'))) == {k: got[k] for k in got if k not in before}


def test_generate_writes_the_keys_and_the_records(tmp_path):
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import POSE_COUNTS
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    runs = {'plain': dict(metrics=True), 'checked': dict(metrics=True, pose_checks=True), 'alone': dict(pose_checks=True), 'bare': {}}
    files = {}
    for name, more in runs.items():
        torch.manual_seed(11)
        written = generate(frag, ddpm, str(tmp_path / name), n_samples=3, n_steps=5, linker_size='4', output_format='sdf', **more)
        files[name] = [open(path).read() for path in written]
    assert files['plain'] == files['checked'] == files['alone'] == files['bare'], 'the files do not change'
    assert not os.path.exists(tmp_path / 'bare' / 'metrics.json') and not os.path.exists(tmp_path / 'plain' / 'pose_checks.json')
    before, got = (json.load(open(tmp_path / name / 'metrics.json')) for name in ('plain', 'checked'))
    assert set(got) == set(before) | pose_keys(False) and before == {k: got[k] for k in before}, 'unchanged without the flag'
    assert json.load(open(tmp_path / 'alone' / 'metrics.json')) == {k: got[k] for k in pose_keys(False)}
    check_scores(got, False)
    records = json.load(open(tmp_path / 'checked' / 'pose_checks.json'))
    assert sorted(records) == [f'output_{k}_frag_.sdf' for k in range(3)]
    for record in records.values():
        assert list(record) == ['counts', 'linker_counts', 'n_flagged_atoms', 'status']
        assert list(record['counts']) == list(record['linker_counts']) == list(POSE_COUNTS)
        assert all(record['linker_counts'][k] <= record['counts'][k] for k in POSE_COUNTS)
    bad = [r['counts']['bonds_short'] + r['counts']['bonds_long'] for r in records.values() if r['status'] == 0]
    assert got['bad_bonds_per_molecule'] == (sum(bad) / len(bad) if bad else None)


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path, pockets):
    from difflinker_amd.metrics import METRIC_NAMES
    from test_gpu_rings import gentle_model
    m = gentle_model(tmp_path, pockets)
    assert m.pose_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.pose_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | pose_keys(True)
    assert {k: got[k] for k in METRIC_NAMES} == plain
    check_scores(got, True)
