"""Explicit hydrogens on the GPU (``dl_add_hydrogens``, ``csrc/hydrogens.hip``) against the plain-Python rule of
``tests/hydrogens_ref.py``.  The C entry point is called on outputs pre-filled with 0x5a bytes, so an element it should write
and does not shows, and the tail of the two lists beyond ``min(n_h, Hcap)`` must still hold the fill.  The integer outputs are
compared exactly.  The positions are expected to be equal bit for bit (fp64, one rounding per operation on both sides); the
assertion is ``max |h_x - ref| <= 1e-9`` A, a bar that is derived and not measured: the rounding of a few dozen fp64
operations on coordinates below 1e3 A is of order 1e-13, and the files resolve 1e-4.  Every comparison prints the largest
difference it found.  The public path (``add_hydrogens``, ``save_sdf_file``, ``generate``) comes last; the launch on a side
stream is in ``tests/test_gpu_streams_hydrogens.py``, collected after the stream harness it uses."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import hydrogens_ref as hr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-9                                       # Angstrom
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read
INT_FIELDS = ('n_h', 'h_count', 'h_parent', 'status')
WORST = [0.0]


def pack(molecules, width, capacity=None, rng=None):
    """``molecules``: dicts with ``types``, ``points``, ``entries`` and optionally ``dropped`` / ``planar`` atom numbers,
    ``n_in``, ``status``.  With ``rng`` the real rows are scattered over ``width`` and ``one_hot``, ``x`` and the masks carry
    garbage on rows that are not real (and ``planar`` beyond the atom count); without it they come first."""
    B = len(molecules)
    capacity = max(len(m['entries']) for m in molecules) + 3 if capacity is None else capacity
    out = {'x': np.zeros((B, width, 3), np.float32), 'one_hot': np.zeros((B, width, 8), np.float32),
           'mask': np.zeros((B, width), np.float32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_in': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32),
           'drop': np.zeros((B, width), np.float32), 'planar': np.zeros((B, width), np.int32)}
    out['bonds'][:] = GARBAGE
    if rng is not None:
        out['x'][:] = rng.normal(0, 3, out['x'].shape)
        out['x'][:, ::5, 1] = np.nan                                    # garbage includes what is not a number
        out['one_hot'][:] = rng.random(out['one_hot'].shape)
        out['drop'][:] = rng.random((B, width)) < 0.5
        out['planar'][:] = rng.integers(0, 3, (B, width))
    for b, m in enumerate(molecules):
        n = len(m['types'])
        real = np.arange(n) if rng is None else np.sort(rng.choice(width, n, replace=False))
        out['mask'][b, real] = 1
        if n:
            out['x'][b, real] = np.asarray(m['points'], dtype=np.float64).reshape(n, 3)
            out['one_hot'][b, real] = 0
            out['one_hot'][b, real, m['types']] = 1
        out['drop'][b, real] = 0                                        # on real rows exactly what the molecule says
        out['drop'][b, real[np.asarray(m.get('dropped', []), dtype=int)]] = 1
        out['planar'][b, :n] = 0                                        # by atom number
        out['planar'][b, np.asarray(m.get('planar', []), dtype=int)] = 1
        rows = m['entries']
        if len(rows):
            out['bonds'][b, :len(rows)] = rows
        out['n_in'][b] = m.get('n_in', len(rows))
        out['status'][b] = m.get('status', 0)
    return out


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def tables():
    from difflinker_amd import const
    assert const.ATOM2IDX == hr.ATOM2IDX
    return hr.tables()


def launch(batch, drop=True, planar=True, status=True, Hcap=None, stream=None):
    """The C entry point on outputs full of 0x5a bytes: a dict of numpy arrays by the names of ``hydrogens_ref.FIELDS``."""
    from difflinker_amd import _lib
    B, N = batch['mask'].shape
    capacity = batch['bonds'].shape[1]
    Hcap = 4 * N if Hcap is None else Hcap
    valence, length = tables()
    held = [dev(batch['x']), dev(batch['one_hot']), dev(batch['mask']), dev(batch['drop']), dev(batch['planar'], torch.int32),
            dev(valence, torch.int32), dev(length, torch.float64), dev(batch['n_in'], torch.int32),
            dev(batch['bonds'], torch.int32), dev(batch['status'], torch.int32)]
    x, one_hot, mask, drop_t, planar_t, valence_t, length_t, n_in, bonds, status_in = held
    shapes = {'h_count': (B, N), 'h_parent': (B, Hcap), 'h_x': (B, Hcap, 3)}
    out = {name: torch.full(shapes.get(name, (B,)), hr.FILL, dtype=torch.int32, device=DEV) for name in INT_FIELDS}
    out['h_x'] = torch.full((B, Hcap, 3), hr.FILL_F64, dtype=torch.float64, device=DEV)
    ptr = lambda t: t.data_ptr() if t.numel() else None      # noqa: E731
    args = _lib.DLHydrogensArgs(
        B=B, N=N, nf=8, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
        drop_mask=drop_t.data_ptr() if drop else None, atom_planar=planar_t.data_ptr() if planar else None,
        default_valence=valence_t.data_ptr(), xh_length=length_t.data_ptr(), capacity=capacity, n_bonds_in=n_in.data_ptr(),
        bonds=ptr(bonds), status_in=status_in.data_ptr() if status else None, Hcap=Hcap, n_h=out['n_h'].data_ptr(),
        h_count=out['h_count'].data_ptr(), h_parent=ptr(out['h_parent']), h_x=ptr(out['h_x']), status=out['status'].data_ptr())
    args.stream = (torch.cuda.current_stream(torch.device(DEV)) if stream is None else stream).cuda_stream
    _lib.check(_lib.load().dl_add_hydrogens(ctypes.byref(args)), 'dl_add_hydrogens')
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def reference(batch, drop=True, planar=True, status=True, Hcap=None):
    valence, length = tables()
    Hcap = 4 * batch['mask'].shape[1] if Hcap is None else Hcap
    return hr.add_hydrogens(batch['x'], batch['one_hot'], batch['mask'], batch['bonds'], batch['n_in'], valence, length, Hcap,
                            batch['status'] if status else None, batch['drop'] if drop else None,
                            batch['planar'] if planar else None)


def same_bits(a, b):
    return all(a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes() for name in hr.FIELDS)


def check(batch, **kwargs):
    got, want = launch(batch, **kwargs), reference(batch, **kwargs)
    for name in INT_FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.int32
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5].tolist())
    assert got['h_x'].shape == want['h_x'].shape and got['h_x'].dtype == np.float64
    listed = np.arange(got['h_x'].shape[1])[None, :] < np.minimum(want['n_h'], got['h_x'].shape[1])[:, None]
    assert np.array_equal(got['h_x'][~listed].view(np.int64), want['h_x'][~listed].view(np.int64)), 'the tail is untouched'
    worst = float(np.abs(got['h_x'][listed] - want['h_x'][listed]).max()) if listed.any() else 0.0
    WORST[0] = max(WORST[0], worst)
    print(f'largest |h_x - reference| = {worst:.3e} A over {int(listed.sum())} hydrogens; so far {WORST[0]:.3e} A; '
          f'equal bits: {got["h_x"].tobytes() == want["h_x"].tobytes()}')
    assert np.isfinite(got['h_x'][listed]).all() and worst <= BAR
    got['cases'] = want['cases']
    return got


def row(batch, b):
    return {key: value[b:b + 1] for key, value in batch.items()}


NAMES = sorted(hr.HAND)
ODD = sorted(hr.DEGENERATE)


@pytest.fixture(scope='module')
def hand():
    molecules = [hr.hand_molecule(name) for name in NAMES] + [dict(types=[], points=[], entries=[])]
    return pack(molecules, 12, rng=np.random.default_rng(0))


@pytest.fixture(scope='module')
def random_batch():
    rng = np.random.default_rng(17)
    molecules, draws = hr.random_molecules(rng, 64)
    assert 64 / draws >= 0.9
    return pack(molecules, 64, rng=rng)


# ---- every branch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_hand_molecule_alone(name):
    m = hr.hand_molecule(name)
    got = check(pack([m], len(m['types'])), drop=False)
    want = hr.HAND[name][3]
    assert got['h_count'][0].tolist() == want and got['n_h'][0] == sum(want) and got['status'][0] == 0


def test_hand_molecules_in_one_ragged_batch(hand):
    got = check(hand)
    assert got['cases'] == {(hr.T4, 0), (hr.T4, 1), (hr.T4, 2), (hr.T4, 3), (hr.T3, 1), (hr.T3, 2), (hr.T2, 1)}, 'every branch'
    for b, name in enumerate(NAMES):
        want = hr.HAND[name][3]
        assert got['h_count'][b, :len(want)].tolist() == want and not got['h_count'][b, len(want):].any(), name
    assert got['n_h'][-1] == 0 and got['status'][-1] == 0, 'the molecule with no real row'
    check(hand, drop=False, planar=False, status=False)
    flat, bent = NAMES.index('pyrrole'), NAMES.index('pyrrole_unflagged')
    centre = lambda b: hand['x'][b][hand['mask'][b] != 0].astype(np.float64).mean(axis=0)    # noqa: E731
    assert got['h_parent'][flat, 0] == got['h_parent'][bent, 0] == 0
    assert abs(got['h_x'][flat, 0, 2] - centre(flat)[2]) < 1e-6 < 0.5 < abs(got['h_x'][bent, 0, 2] - centre(bent)[2])


@pytest.mark.parametrize('name', ODD)
def test_degenerate_branches(name):
    m = hr.hand_molecule(name)
    got = check(pack([m], len(m['types']) + 1), drop=False)
    assert got['h_count'][0, :len(m['types'])].tolist() == hr.DEGENERATE[name][3] and got['status'][0] == 0
    decisions = []
    valence, length = hr.tables()
    n = len(m['types'])
    hr.molecule(np.asarray(m['points'], np.float32), m['types'], np.ones(n), m['entries'], len(m['entries']), valence, length,
                decisions=decisions)
    assert not hr.near_threshold(decisions), 'decided exactly, or orders of magnitude from EPS'
    if name == 'antiparallel':
        up = [0.0, 1.09 / math.sqrt(3), 1.09 * math.sqrt(2 / 3)]
        assert np.allclose(got['h_x'][0, 3:5], [up, [up[0], up[1], -up[2]]], rtol=0, atol=1e-12)
    if name == 't_shaped':
        assert np.allclose(got['h_x'][0, 0], [0.0, -1.09, 0.0], rtol=0, atol=1e-12)
    if name == 'trigonal_planar':
        assert got['h_x'][0, 0, :2].tolist() == [0.0, 0.0] and abs(got['h_x'][0, 0, 2]) == 1.09, 'out of the plane'


def test_random_molecules(random_batch):
    got = check(random_batch)
    assert random_batch['mask'].shape == (64, 64) and 1 <= random_batch['mask'].sum(axis=1).min() <= 40
    assert got['cases'] == {(hr.T4, 0), (hr.T4, 1), (hr.T4, 2), (hr.T4, 3), (hr.T3, 1), (hr.T3, 2), (hr.T2, 1)}, 'every class'
    assert got['n_h'].sum() > 256 and not got['status'].any()
    check(random_batch, drop=False)
    assert reference(random_batch, planar=False)['n_h'].sum() == got['n_h'].sum(), 'a flag moves a hydrogen, it adds none'
    check(random_batch, planar=False, status=False)


# ---- limits and flags --------------------------------------------------------------------------------------------------------
def test_a_short_list_keeps_the_true_count_and_an_intact_prefix(hand):
    full = launch(hand)
    got = check(hand, Hcap=3)
    assert np.array_equal(got['n_h'], full['n_h']) and np.array_equal(got['h_count'], full['h_count'])
    assert got['status'].tolist() == [hr.OVERFLOW if n > 3 else 0 for n in full['n_h']] and (full['n_h'] > 3).any()
    assert np.array_equal(got['h_x'][:, :3][full['n_h'] >= 3], full['h_x'][:, :3][full['n_h'] >= 3])
    got = check(hand, Hcap=0)
    assert got['h_x'].shape == (len(NAMES) + 1, 0, 3) and np.array_equal(got['n_h'], full['n_h'])


def test_counts_beyond_the_capacity_and_below_zero():
    m = hr.hand_molecule('propane')
    molecules = [dict(m, n_in=5, status=2), dict(m, n_in=-3), dict(m, n_in=1), dict(m, status=16 | 2)]
    batch = pack(molecules, 4, capacity=2)
    got = check(batch, drop=False)
    assert got['status'].tolist() == [2 | hr.BONDS_OVERFLOW, 0, 0, 18] and got['n_h'].tolist() == [8, 12, 10, 8]
    got = check(batch, drop=False, status=False)
    assert got['status'].tolist() == [hr.BONDS_OVERFLOW, 0, 0, 0], 'a null status_in carries nothing'
    got = check(pack([dict(m, entries=[], n_in=2)], 3, capacity=0), drop=False)
    assert got['status'].tolist() == [hr.BONDS_OVERFLOW] and got['n_h'].tolist() == [12]


def test_bad_entries_set_the_bit_and_are_skipped():
    m = hr.hand_molecule('propane')
    wrong = [(0, 1, 0), (0, 1, 4), (2, 2, 1), (-1, 2, 1), (2, 3, 1)]
    molecules = [dict(m, entries=m['entries'] + [w]) for w in wrong]
    molecules.append(dict(m, entries=[(1, 0, 1), (0, 1, 3), (2, 1, 1)]))          # the first entry's order counts
    molecules.append(dict(m, entries=[(0, 1, 3), (1, 0, 1), (2, 1, 1)]))
    molecules.append(dict(m, entries=wrong + [(0, 1, 2), (2, 1, 1), (1, 0, 1), (1, 2, 3)]))
    molecules.append(m)
    got = check(pack(molecules, 5, rng=np.random.default_rng(8)), drop=False)
    assert got['status'].tolist() == [hr.BAD_BOND] * 8 + [0]
    assert got['n_h'].tolist() == [8] * 6 + [4, 6, 8], 'a repeated pair counts once, with its first order'
    assert got['h_count'][6, :3].tolist() == [1, 0, 3] and got['h_count'][7, :3].tolist() == [2, 1, 3]


def test_non_finite_coordinates():
    m = hr.hand_molecule('propane')
    molecules = []
    for value in (float('nan'), float('inf'), -float('inf')):
        bad = [list(p) for p in m['points']]
        bad[2][1] = value
        molecules.append(dict(m, points=bad))
        molecules.append(dict(m, points=bad, dropped=[2]))
    got = check(pack(molecules + [m], 4))
    assert got['status'].tolist() == [hr.NONFINITE, 0] * 3 + [0]
    assert got['n_h'].tolist() == [0, 6] * 3 + [8], 'none on a kept atom\'s account; a dropped atom\'s has no effect'
    assert not got['h_count'][0].any() and got['h_count'][1].tolist() == [3, 3, 0, 0]


def test_the_atom_limit_and_wide_rows():
    fits, over = hr.chain(256), hr.chain(257)
    over['entries'] = over['entries'] + [(5, 5, 1)]
    batch = pack([hr.hand_molecule('benzene'), over, fits, dict(over, dropped=[100])], 300, rng=np.random.default_rng(4))
    got = check(batch)
    assert got['status'].tolist() == [0, hr.TOO_LARGE, 0, hr.BAD_BOND], 'too large: the list is not looked at'
    assert got['n_h'].tolist() == [6, 0, 2 * 256 + 2, 2 * 256 + 4] and not got['h_count'][1].any(), 'one chain; two chains'
    got = check(pack([hr.hand_molecule('propane'), fits], 1024, rng=np.random.default_rng(5)), drop=False)
    assert got['n_h'].tolist() == [8, 514] and not got['status'].any(), 'N = 1024 with 3 real rows, and with 256'


def test_one_row_no_row_and_no_molecule():
    lone = hr.hand_molecule('lone_N')
    got = check(pack([lone, dict(types=[], points=[], entries=[])], 1, capacity=0), drop=False)
    assert got['n_h'].tolist() == [3, 0] and got['h_count'].tolist() == [[3], [0]] and not got['status'].any()
    batch = pack([lone], 1)
    got = launch({key: value[:0] for key, value in batch.items()})
    assert all(got[name].shape[0] == 0 for name in hr.FIELDS)


def test_bad_arguments_are_refused():
    from difflinker_amd import _lib
    lib = _lib.load()
    assert lib.dl_add_hydrogens(None) != _lib.DL_OK
    for more in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict(Hcap=-1), dict()):
        args = _lib.DLHydrogensArgs(**dict(dict(B=1, N=4, nf=8, capacity=0, Hcap=0), **more))      # every pointer null
        assert lib.dl_add_hydrogens(ctypes.byref(args)) != _lib.DL_OK, more
    assert lib.dl_add_hydrogens(ctypes.byref(_lib.DLHydrogensArgs(B=0, N=4, nf=8))) == _lib.DL_OK


# ---- determinism and independence --------------------------------------------------------------------------------------------
def test_two_launches_give_equal_bits(random_batch, hand):
    for batch in (random_batch, hand):
        assert same_bits(launch(batch), launch(batch))


def test_each_molecule_alone_equals_its_row(random_batch):
    ragged = {key: value[[0, 9, 22, 41, 63]] for key, value in random_batch.items()}
    whole = launch(ragged)
    assert len(set(ragged['mask'].sum(axis=1).tolist())) > 1
    for b in range(5):
        alone = launch(row(ragged, b))
        for name in hr.FIELDS:
            assert alone[name][0].tobytes() == whole[name][b].tobytes(), (name, b)


# ---- the public path ---------------------------------------------------------------------------------------------------------
def public_batch():
    import aromatic_ref as ar
    types, points, _ = ar.hand_molecule('benzene')
    benzene = dict(types=list(types), points=[tuple(p) for p in points], entries=[])
    propane = dict(hr.hand_molecule('propane'), entries=[])
    return pack([benzene, propane, benzene], 9, capacity=0, rng=np.random.default_rng(2))


def through_the_public_path(one_hot, x, mask):
    from difflinker_amd.molecule_builder import add_hydrogens, perceive_bonds, refine_bond_orders
    found = perceive_bonds(one_hot, x, mask, False)
    refined, aromatic = refine_bond_orders(found, one_hot, x, mask, False)
    return refined, aromatic, add_hydrogens(refined, one_hot, x, mask, False, atom_planar=aromatic.atom_aromatic)


def test_benzene_through_the_public_path():
    from difflinker_amd.molecule_builder import Hydrogens
    batch = public_batch()
    x = np.nan_to_num(batch['x'])
    one_hot, xt, mask = dev(batch['one_hot']), dev(x), dev(batch['mask']).unsqueeze(2)
    refined, aromatic, got = through_the_public_path(one_hot, xt, mask)
    assert isinstance(got, Hydrogens) and got._fields == ('n_h', 'h_count', 'parent', 'x', 'status')
    assert got.parent.shape == (3, 36) and got.x.shape == (3, 36, 3) and got.x.dtype == torch.float64
    assert got.n_h.tolist() == [6, 8, 6] and not got.status.any() and aromatic.n_aromatic_rings.tolist() == [1, 0, 1]
    for b in (0, 2):
        ring = x[b][batch['mask'][b] != 0].astype(np.float64)
        assert np.abs(ring[:, 2]).max() == 0, 'the ring lies in the plane z = 0'
        positions = got.x[b, :6].cpu().numpy()
        assert np.abs(positions[:, 2]).max() <= 1e-6 and got.parent[b, :6].tolist() == list(range(6))
        assert np.allclose(np.linalg.norm(positions - ring, axis=1), 1.09, atol=1e-12)
        assert not got.x[b, 6:].any() and not got.parent[b, 6:].any(), 'zero beyond the count'
    want = hr.add_hydrogens(x, batch['one_hot'], batch['mask'], refined.bonds.cpu().numpy(), refined.n_bonds.cpu().numpy(),
                            *hr.tables(), 36, refined.status.cpu().numpy(), None, aromatic.atom_aromatic.cpu().numpy())
    assert np.array_equal(got.n_h.cpu().numpy(), want['n_h']) and np.array_equal(got.h_count.cpu().numpy(), want['h_count'])
    worst = max(float(np.abs(got.x[b, :n].cpu().numpy() - want['h_x'][b, :n]).max()) for b, n in enumerate(want['n_h']))
    print(f'largest |h_x - reference| = {worst:.3e} A through the public path')
    assert worst <= BAR


def test_input_forms_give_the_same_bits():
    from difflinker_amd.molecule_builder import Bonds, add_hydrogens
    batch = public_batch()
    one_hot, x, mask = dev(batch['one_hot']), dev(np.nan_to_num(batch['x'])), dev(batch['mask']).unsqueeze(2)
    refined, aromatic, base = through_the_public_path(one_hot, x, mask)
    planar = aromatic.atom_aromatic
    wide = lambda t, dtype: torch.stack([t.to(dtype), t.to(dtype)], dim=-1)[..., 0]      # noqa: E731  (strided)
    padded = torch.cat([refined.bonds, torch.full_like(refined.bonds, 7)], dim=1)
    forms = Bonds(wide(refined.n_bonds, torch.int64), padded.long()[:, :refined.bonds.shape[1]], None, None, None,
                  wide(refined.status, torch.int64))
    got = add_hydrogens(forms, wide(one_hot, torch.float64), wide(x, torch.float64), wide(mask[:, :, 0], torch.float64), False,
                        atom_planar=wide(planar, torch.int64))
    torch.cuda.synchronize()
    for name in base._fields:
        assert torch.equal(getattr(got, name), getattr(base, name)), name
    with pytest.raises(ValueError, match='shapes disagree'):
        add_hydrogens(refined, one_hot, x[:, :5], mask, False)
    short = add_hydrogens(refined, one_hot, x, mask, False, atom_planar=planar, capacity=5)
    assert short.n_h.tolist() == [6, 8, 6] and short.status.tolist() == [hr.OVERFLOW] * 3
    assert torch.equal(short.x, base.x[:, :5])


def test_generate_writes_the_hydrogens(tmp_path, capsys):
    """``generate`` with ``hydrogens=True`` writes the heavy atoms and bonds of the same call without it, then the hydrogens."""
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.io import read_sdf_molecules
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    files, lines = {}, {}
    for name, more in (('plain', {}), ('with', dict(hydrogens=True))):
        torch.manual_seed(11)
        capsys.readouterr()
        files[name] = generate(frag, ddpm, str(tmp_path / name), n_samples=3, n_steps=5, linker_size='4', output_format='sdf',
                               bond_orders='geometric', **more)
        lines[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'hydrogens_per_molecule' not in lines['plain'] and len(files['with']) == 3
    assert {k: v for k, v in lines['with'].items() if k != 'hydrogens_per_molecule'} == lines['plain']
    total = 0
    for plain, full in zip(files['plain'], files['with']):
        a, b = open(plain).read().splitlines(), open(full).read().splitlines()
        n, nb = int(a[3][0:3]), int(a[3][3:6])
        nh = int(b[3][0:3]) - n
        assert nh >= 0 and int(b[3][3:6]) == nb + nh and len(b) == len(a) + 2 * nh
        assert b[4:4 + n] == a[4:4 + n] and all(ln[31:34].strip() == 'H' for ln in b[4 + n:4 + n + nh])
        assert b[4 + n + nh:4 + n + nh + nb] == a[4 + n:4 + n + nb]
        (before,), _ = read_sdf_molecules(plain)
        (after,), _ = read_sdf_molecules(full)
        assert after.symbols == before.symbols and after.bonds == before.bonds and np.array_equal(after.positions, before.positions)
        total += nh
    assert total > 0 and abs(lines['with']['hydrogens_per_molecule'] - total / 3) < 1e-6
