"""Circular fingerprints and their Tanimoto similarity on the GPU (``dl_fingerprints`` and ``dl_tanimoto_nearest``,
``csrc/fingerprint.hip``) against the plain-Python rule of ``tests/fingerprint_ref.py``.  Every output is an integer and every
comparison is exact; every output buffer holds 0x5a bytes before its launch.  The fingerprint batches are fed as bond lists
directly, no geometry needed.  Then the stream contract of both entry points (they take the stream inside their args struct,
so ``tests/test_gpu_streams.py`` does not list them: its harness is used here), and the public path last
(``analyze_fingerprints``, ``sample(..., diversity=True)``, ``generate(..., diversity=True)``, ``DDPM.diversity_metrics``)."""
import ctypes
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import fingerprint_ref as fr
import test_gpu_rings as RG
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, NF = 300, 5
KEPT = (1, 2, 3, 63, 64, 65, 255, 256, 257)      # around the wave, the workgroup and DL_FP_MAX_ATOMS
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read
STALE = 0x5a


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def stale(shape, dtype=torch.int32):
    """An output buffer of ``shape`` whose every byte is 0x5a."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if t.numel():
        t.view(torch.uint8).fill_(STALE)
    return t


# ---- fingerprints -------------------------------------------------------------------------------------------------------------

def pack(rng, molecules, width=N, capacity=None):
    """``molecules``: dicts with ``atoms``, ``types``, ``entries`` ``(i, j, order)`` and optionally ``dropped`` / ``centres`` atom
    numbers, ``n_in``, ``status``.  Real rows are scattered over ``width``; the optional masks carry garbage on the other rows."""
    B = len(molecules)
    capacity = max(len(m['entries']) for m in molecules) + 3 if capacity is None else capacity
    out = {'one_hot': rng.random((B, width, NF)).astype(np.float32) * 0.5, 'mask': np.zeros((B, width), np.float32),
           'bonds': np.zeros((B, capacity, 3), np.int32), 'n_in': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32),
           'drop': (rng.random((B, width)) < 0.5).astype(np.float32), 'centre': (rng.random((B, width)) < 0.5).astype(np.float32)}
    out['bonds'][:] = GARBAGE
    for b, m in enumerate(molecules):
        out['mask'][b] = RG.scattered_rows(rng, m['atoms'], width)
        real = np.nonzero(out['mask'][b])[0]
        out['one_hot'][b, real, np.asarray(m['types'], dtype=int)] = 1.0              # the largest entry of the row
        for key, atoms in (('drop', m.get('dropped', [])), ('centre', m.get('centres', range(m['atoms'])))):
            out[key][b, real] = 0                                                      # on real rows what the molecule says
            out[key][b, real[np.asarray(list(atoms), dtype=int)]] = 1
        rows = m['entries'][:capacity]
        if rows:
            out['bonds'][b, :len(rows)] = rows
        out['n_in'][b] = m.get('n_in', len(m['entries']))
        out['status'][b] = m.get('status', 0)
    return out


def random_molecule(rng, n_kept, n_dropped):
    atoms, pairs, dropped = RG.random_graph(rng, n_kept, n_dropped)
    return {'atoms': atoms, 'types': rng.integers(0, NF, atoms), 'dropped': dropped,
            'entries': [(i, j, int(rng.integers(1, 4))) for i, j in pairs],
            'centres': rng.choice(atoms, (atoms + 1) // 2, replace=False)}


def build_mixed():
    rng = np.random.default_rng(21)
    molecules = [random_molecule(rng, n_kept, min(n_kept // 8 + 1, N - n_kept)) for n_kept in KEPT]
    molecules[3]['status'] = 2
    for types, bonds in (fr.BENZENE, fr.TOLUENE, fr.HEXANE):
        molecules.append({'atoms': len(types), 'types': types, 'entries': bonds})
    return molecules, pack(rng, molecules)


def launch(batch, drop=True, centre=True, radius=2, n_bits=2048):
    """The C entry on output buffers full of 0x5a bytes, on torch's current stream."""
    from difflinker_amd import _lib
    B, width = batch['mask'].shape
    capacity = batch['bonds'].shape[1]
    ins = {'one_hot': dev(batch['one_hot']), 'node_mask': dev(batch['mask']), 'n_bonds_in': dev(batch['n_in'], torch.int32),
           'bonds': dev(batch['bonds'], torch.int32), 'status_in': dev(batch['status'], torch.int32)}
    if drop:
        ins['drop_mask'] = dev(batch['drop'])
    if centre:
        ins['centre_mask'] = dev(batch['centre'])
    out = {name: stale((B, n_bits // 32) if name == 'bits' else (B,)) for name in fr.FIELDS}
    pointers = {k: v.data_ptr() for k, v in {**ins, **out}.items() if v.numel()}
    args = _lib.DLFingerprintArgs(B=B, N=width, nf=batch['one_hot'].shape[2], capacity=capacity, radius=radius, n_bits=n_bits,
                                  stream=torch.cuda.current_stream().cuda_stream, **pointers)
    _lib.check(_lib.load().dl_fingerprints(ctypes.byref(args)), 'dl_fingerprints')
    return out


def reference(batch, drop=True, centre=True, radius=2, n_bits=2048):
    return fr.fingerprints(batch['one_hot'], batch['mask'], batch['bonds'], batch['n_in'], batch['status'],
                           batch['drop'] if drop else None, batch['centre'] if centre else None, radius, n_bits)


def assert_exact(got, want, fields, what=''):
    for name in fields:
        if want[name] is None:
            assert got.get(name) is None, (what, name)
            continue
        g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
        g = g.view(want[name].dtype) if g.dtype != want[name].dtype and g.dtype.itemsize == want[name].dtype.itemsize else g
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, (what, name, g.shape, g.dtype)
        assert np.array_equal(g, want[name]), (what, name, np.argwhere(g != want[name])[:5].tolist())


@pytest.fixture(scope='module')
def mixed():
    molecules, batch = build_mixed()
    return {'molecules': molecules, 'batch': batch}


def test_every_radius_and_width_is_exact(mixed):
    batch = mixed['batch']
    assert batch['mask'].shape == (12, N) and batch['bonds'].shape[1] > 256
    for radius in range(5):
        for n_bits in (512, 1024, 2048):
            want = reference(batch, radius=radius, n_bits=n_bits)
            assert want['n_atoms'][:9].tolist() == list(KEPT) and want['status'][8] == fr.TOO_LARGE and want['status'][3] == 2
            assert_exact(launch(batch, radius=radius, n_bits=n_bits), want, fr.FIELDS, f'radius {radius}, {n_bits} bits')
    want = reference(batch)
    assert (want['n_on'][1:8] > 0).all() and want['n_on'][8] == 0 and want['n_centres'][8] == 0 and not want['bits'][8].any()
    assert want['n_on'][7] > 100, 'many bits: the ORs of different atoms meet in the same words'
    assert set(np.nonzero(np.unpackbits(want['bits'][9].view(np.uint8), bitorder='little'))[0].tolist()) == {92, 1852, 2031}
    assert want['n_on'][9:].tolist() == [3, 9, 6], 'benzene, toluene, hexane: the pinned counts'


def test_the_optional_masks(mixed):
    batch = mixed['batch']
    nan = {k: v.copy() for k, v in batch.items()}
    for key in ('drop', 'centre'):
        nan[key][batch['mask'] == 0] = np.nan                              # rows that are not real are never looked at
    for drop, centre in ((True, True), (False, True), (True, False), (False, False)):
        want = reference(batch, drop, centre)
        assert_exact(launch(nan, drop, centre), want, fr.FIELDS, f'drop {drop} centre {centre}')
        if not drop:
            assert (want['status'][6:9] == fr.TOO_LARGE).all(), '255 + 32 atoms and more, none dropped'
        if not centre:
            assert (want['n_centres'] == want['n_atoms'])[want['status'] == 0].all()
    with_centres, without = reference(batch, True, True), reference(batch, True, False)
    assert (with_centres['bits'] & ~without['bits']).sum() == 0 and (with_centres['n_on'][:8] <= without['n_on'][:8]).all()
    assert (with_centres['n_on'][4:8] < without['n_on'][4:8]).all(), 'fewer centres, fewer bits'


def test_renumbering_and_list_order_change_no_bit(mixed):
    rng = np.random.default_rng(22)
    m = mixed['molecules'][5]                                            # 65 kept atoms, 9 dropped
    n = m['atoms']
    perm = rng.permutation(n)                                            # old atom k becomes atom perm[k]
    moved = {'atoms': n, 'types': np.asarray(m['types'])[np.argsort(perm)], 'dropped': perm[np.asarray(m['dropped'])],
             'centres': perm[np.asarray(m['centres'])],
             'entries': [(int(perm[j]), int(perm[i]), o) if rng.random() < 0.5 else (int(perm[i]), int(perm[j]), o)
                         for i, j, o in (m['entries'][k] for k in rng.permutation(len(m['entries'])))]}
    batch = pack(rng, [m, moved])
    want = reference(batch, radius=4)
    assert np.array_equal(want['bits'][0], want['bits'][1]) and want['n_on'][0] > 100
    got = launch(batch, radius=4)
    assert_exact(got, want, fr.FIELDS, 'renumbered')
    again = launch(batch, radius=4)
    assert all(torch.equal(got[name], again[name]) for name in fr.FIELDS), 'two launches: the same bits'


def test_bad_entries_counts_and_status():
    rng = np.random.default_rng(23)
    square = [(0, 1, 1), (1, 2, 2), (2, 3, 3), (3, 0, 1)]
    cases = [[(2, 2, 1)], [(0, 6, 1)], [(-1, 2, 1)], [(0, 2, 0)], [(0, 2, 4)], [(4, 5, 1)], []]
    molecules = [{'atoms': 6, 'types': [0, 1, 2, 0, 1, 2], 'entries': square[:2] + extra + square[2:], 'dropped': [5]} for extra in cases]
    molecules[-1]['status'] = 2
    batch = pack(rng, molecules, width=40)
    for radius in (0, 2):                                                # radius 0 never needs the list, but reports on it
        want = reference(batch, radius=radius)
        assert want['status'].tolist() == [fr.BAD_BOND] * 5 + [0, 2], 'a bond to a dropped atom is no error'
        assert all(np.array_equal(want['bits'][k], want['bits'][6]) for k in range(5)), 'skipped entries change nothing'
        assert_exact(launch(batch, radius=radius), want, fr.FIELDS, f'bad entries, radius {radius}')
    # n_bonds_in beyond the capacity, and below zero
    types, bonds = fr.TOLUENE
    counted = [{'atoms': 7, 'types': types, 'entries': bonds, 'n_in': n_in, 'status': status}
               for n_in, status in ((7, 0), (8, 0), (1 << 30, 2), (-1, 0), (-(1 << 31), 2), (5, 0), (0, 0))]
    batch = pack(rng, counted, width=33, capacity=7)
    want = reference(batch)
    over = fr.BONDS_OVERFLOW
    assert want['status'].tolist() == [0, over, over | 2, 0, 2, 0, 0] and want['n_on'].tolist() == [9, 9, 9, 3, 3, 8, 3]
    assert_exact(launch(batch), want, fr.FIELDS, 'counts')


def test_capacity_zero_a_null_list_and_an_empty_batch():
    from difflinker_amd.metrics import fingerprints
    from difflinker_amd.molecule_builder import Bonds
    rng = np.random.default_rng(24)
    batch = pack(rng, [{'atoms': 5, 'types': [0, 1, 0, 1, 2], 'entries': [], 'dropped': [1]},
                       {'atoms': 1, 'types': [3], 'entries': []},
                       {'atoms': 40, 'types': [0] * 40, 'entries': [], 'n_in': 7, 'status': 2}], width=64, capacity=0)
    assert batch['bonds'].shape == (3, 0, 3)
    want = reference(batch)
    assert want['status'].tolist() == [0, 0, 2 | fr.BONDS_OVERFLOW] and want['n_on'].tolist() == [9, 3, 3]
    assert_exact(launch(batch), want, fr.FIELDS, 'capacity 0')
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)     # noqa: E731
    none = fingerprints(torch.zeros(0, 5, NF, device=DEV), torch.zeros(0, 5, 1, device=DEV),
                        Bonds(i32(0), i32(0, 20, 3), None, None, None, i32(0)), n_bits=512)
    assert none.bits.shape == (0, 16) and none.status.shape == (0,)


def test_the_python_wrapper_gives_the_same(mixed):
    from difflinker_amd.metrics import Fingerprints, fingerprints
    from difflinker_amd.molecule_builder import Bonds
    batch = mixed['batch']
    found = Bonds(dev(batch['n_in'], torch.int32), dev(batch['bonds'], torch.int32), None, None, None, dev(batch['status'], torch.int32))
    got = fingerprints(dev(batch['one_hot']), dev(batch['mask'])[:, :, None], found, dev(batch['drop']), dev(batch['centre'])[:, :, None],
                       radius=3, n_bits=1024)
    assert isinstance(got, Fingerprints) and got.bits.dtype == torch.int32 and got.bits.shape == (12, 32)
    assert_exact(got._asdict(), reference(batch, radius=3, n_bits=1024), fr.FIELDS, 'wrapper')


# ---- Tanimoto -----------------------------------------------------------------------------------------------------------------

def random_rows(rng, m, w, density):
    return np.packbits(rng.random((m, w * 32)) < density, axis=1, bitorder='little').view(np.uint32).reshape(m, w)


def nearest(a, b, a_off=None, b_off=None, exclude=False, want_sum=True, same=False):
    """The C entry on output buffers full of 0x5a bytes; ``same``: B is the very buffer of A."""
    from difflinker_amd import _lib
    a_dev = dev(a.view(np.int32), torch.int32)
    b_dev = a_dev if same else dev(b.view(np.int32), torch.int32)
    G = 0 if a_off is not None and len(a_off) == 0 else (1 if a_off is None else len(a_off) - 1)
    if a_off is None:
        a_off, b_off = [0, len(a)], [0, len(b)]
    offsets = {'a_offsets': dev(np.asarray(a_off, np.int32), torch.int32), 'b_offsets': dev(np.asarray(b_off, np.int32), torch.int32)}
    out = {name: stale((len(a),), torch.int64 if name == 'sum_q20' else torch.int32) for name in fr.NEAREST_FIELDS
           if want_sum or name != 'sum_q20'}
    pointers = {k: v.data_ptr() for k, v in {'a_bits': a_dev, 'b_bits': b_dev, **offsets, **out}.items() if v.numel()}
    args = _lib.DLTanimotoArgs(Ma=len(a), Mb=len(b), W=a.shape[1], G=G, exclude_diagonal=int(exclude),
                               stream=torch.cuda.current_stream().cuda_stream, **pointers)
    _lib.check(_lib.load().dl_tanimoto_nearest(ctypes.byref(args)), 'dl_tanimoto_nearest')
    return out


def plant(rng, a, b):
    """Duplicated rows (the tie goes to the lowest index), all-zero rows in both (u == 0) and an all-ones row in both."""
    if len(b) >= 6:
        b[len(b) - 1] = b[1]
        b[len(b) // 2] = b[1]
        b[3] = 0
        b[len(b) - 2] = 0xFFFFFFFF
    if len(a) >= 4:
        a[0] = 0
        a[2] = 0xFFFFFFFF
        if len(b) >= 6:
            a[3] = b[1]
    return a, b


@pytest.mark.parametrize('w', [16, 32, 64])
def test_one_group_of_every_size(w):
    from difflinker_amd import _lib
    T = _lib.DL_TANIMOTO_TILE
    rng = np.random.default_rng(w)
    sizes_a, sizes_b = (1, 63, 64, 65, 255, 256, 257), (0, 1, T - 1, T, T + 1, 2 * T + 1)
    for k, ma in enumerate(sizes_a):                                     # every Ma and every Mb, every Ma with two Mb
        for mb in (sizes_b[k % 6], sizes_b[(k + 3) % 6]):
            density = (0.02, 0.5)[(k + (mb > T)) % 2]
            a, b = plant(rng, random_rows(rng, ma, w, density), random_rows(rng, mb, w, density))
            want = fr.tanimoto_nearest(a, b)
            assert_exact(nearest(a, b), want, fr.NEAREST_FIELDS, f'W {w} Ma {ma} Mb {mb}')
            if ma >= 4 and mb >= 6:
                assert want['nn_index'][3] == 1 and want['nn_common'][3] == want['nn_union'][3], 'of equal rows the lowest'
                assert want['nn_index'][0] == 3 and want['nn_union'][0] == 0, 'two empty fingerprints are equal'
                assert want['nn_index'][2] == mb - 2 and want['nn_common'][2] == 32 * w, 'the all-ones pair'
    assert (32 * 64) << 20 == 1 << 31, 'the numerator that needs an unsigned word'


def grouped_case(rng, w):
    from difflinker_amd import _lib
    T = _lib.DL_TANIMOTO_TILE
    a, b = plant(rng, random_rows(rng, 600, w, 0.1), random_rows(rng, 2 * T + 40, w, 0.1))
    # seven uneven groups: the third and the fifth straddle a 256-row boundary of A, the fourth has no A rows, the second no
    # B rows, the sixth an inverted B range, the last one B rows beyond Mb; rows 0-9 and 580-599 are in no group
    a_off = [10, 100, 250, 300, 300, 520, 540, 580]
    b_off = [0, 5, 5, T + 3, T + 9, 2 * T + 30, 2 * T + 10, 1 << 30]
    return a, b, a_off, b_off


@pytest.mark.parametrize('w', [16, 64])
def test_groups(w):
    rng = np.random.default_rng(100 + w)
    a, b, a_off, b_off = grouped_case(rng, w)
    want = fr.tanimoto_nearest(a, b, a_off, b_off)
    assert want['n_pairs'][:10].sum() == 0 and want['n_pairs'][100:250].sum() == 0 and want['n_pairs'][520:540].sum() == 0
    assert (want['nn_index'][want['n_pairs'] == 0] == -1).all() and want['n_pairs'][560] == 30 and want['n_pairs'][255] == want['n_pairs'][256] > 0
    assert_exact(nearest(a, b, a_off, b_off), want, fr.NEAREST_FIELDS, 'seven groups')
    none = fr.tanimoto_nearest(a, b, [], [])
    assert (none['nn_index'] == -1).all() and not none['sum_q20'].any()
    assert_exact(nearest(a, b, [], []), none, fr.NEAREST_FIELDS, 'no group')
    # offsets below zero and beyond M are clamped
    wild = fr.tanimoto_nearest(a, b, [-5, 300, 1 << 30], [-(1 << 31), 17, (1 << 31) - 1])
    assert wild['n_pairs'][0] == 17 and wild['n_pairs'][599] == len(b) - 17
    assert_exact(nearest(a, b, [-5, 300, 1 << 30], [-(1 << 31), 17, (1 << 31) - 1]), wild, fr.NEAREST_FIELDS, 'clamped')


@pytest.mark.parametrize('w', [32, 64])
def test_a_set_against_itself_and_without_the_sum(w):
    rng = np.random.default_rng(200 + w)
    a, _ = plant(rng, random_rows(rng, 300, w, 0.3), np.zeros((0, w), np.uint32))
    a[7] = a[5]
    offsets = [0, 1, 120, 300]                                           # a group of one row: no candidate but itself
    want = fr.tanimoto_nearest(a, a, offsets, offsets, exclude_diagonal=True)
    assert want['n_pairs'].tolist() == [0] + [118] * 119 + [179] * 180 and want['nn_index'][5] == 7 and want['nn_index'][7] == 5
    assert (want['nn_index'] != np.arange(300)).all()
    got = nearest(a, a, offsets, offsets, exclude=True, same=True)
    assert_exact(got, want, fr.NEAREST_FIELDS, 'itself')
    with_diagonal = fr.tanimoto_nearest(a, a, offsets, offsets)
    assert (with_diagonal['nn_index'][1:] <= np.arange(1, 300)).all() and (with_diagonal['nn_common'] == with_diagonal['nn_union']).all()
    assert_exact(nearest(a, a, offsets, offsets, same=True), with_diagonal, fr.NEAREST_FIELDS, 'itself, diagonal kept')
    bare = nearest(a, a, offsets, offsets, exclude=True, want_sum=False, same=True)
    assert 'sum_q20' not in bare
    assert_exact(bare, want, fr.NEAREST_FIELDS[:4], 'no sum: the other outputs are what they were')


def test_the_python_wrapper_of_the_similarity():
    from difflinker_amd.metrics import Nearest, tanimoto_nearest
    rng = np.random.default_rng(300)
    a, b, a_off, b_off = grouped_case(rng, 32)
    a_dev, b_dev = dev(a.view(np.int32), torch.int32), dev(b.view(np.int32), torch.int32)
    names = dict(zip(fr.NEAREST_FIELDS, ('index', 'common', 'union', 'n_pairs', 'sum_q20')))
    as_dict = lambda got: {k: getattr(got, v) for k, v in names.items()}       # noqa: E731
    got = tanimoto_nearest(a_dev, b_dev)
    assert isinstance(got, Nearest) and got.sum_q20.dtype == torch.int64
    assert_exact(as_dict(got), fr.tanimoto_nearest(a, b), fr.NEAREST_FIELDS, 'one group')
    got = tanimoto_nearest(a_dev, b_dev, dev(a_off, torch.int32), dev(b_off, torch.int32), want_sum=False)
    assert got.sum_q20 is None
    assert_exact(as_dict(got), fr.tanimoto_nearest(a, b, a_off, b_off, want_sum=False), fr.NEAREST_FIELDS, 'groups')
    empty = tanimoto_nearest(a_dev[:0], b_dev)
    assert empty.index.shape == (0,) and empty.sum_q20.shape == (0,)


# ---- the stream contract of both entry points ----------------------------------------------------------------------------------

def test_fingerprints_on_a_side_stream(monkeypatch, delay):  # noqa: F811
    """Part A of tests/test_gpu_streams.py for ``dl_fingerprints``: the inputs hold poison until copies queued on the side
    stream behind a delay have written them, the outputs are read on that stream, and equal the default stream's bits."""
    batch = build_mixed()[1]
    make = GS._through_dev(sys.modules[__name__], lambda: launch(batch, radius=3))
    base = GS.check_stream_contract(lambda: make(monkeypatch), delay)
    assert_exact(base, reference(batch, radius=3), fr.FIELDS, 'the baseline')


def test_tanimoto_on_a_side_stream(monkeypatch, delay):  # noqa: F811
    rng = np.random.default_rng(400)
    a, b, a_off, b_off = grouped_case(rng, 64)
    make = GS._through_dev(sys.modules[__name__], lambda: nearest(a, b, a_off, b_off))
    base = GS.check_stream_contract(lambda: make(monkeypatch), delay)
    assert_exact(base, fr.tanimoto_nearest(a, b, a_off, b_off), fr.NEAREST_FIELDS, 'the baseline')


# ---- the public path ------------------------------------------------------------------------------------------------------------

def kekule_ring(single=1.50, double=1.34):
    """A planar six-ring whose sides alternate between a carbon-carbon single and double bond length, atom 0 first."""
    points, at, heading = [], np.zeros(2), 0.0
    for k in range(6):
        points.append(at.copy())
        at = at + (single, double)[k % 2] * np.array([np.cos(heading), np.sin(heading)])
        heading += np.pi / 3
    ring = np.asarray(points)
    return np.concatenate([ring - ring.mean(0), np.zeros((6, 1))], 1)


def hand_batch():
    """Benzene, toluene, pyridine and hexane from coordinates; width 12, a padding row in front of the last two."""
    ring = kekule_ring()
    methyl = ring[0] + 1.50 * ring[0] / np.linalg.norm(ring[0])
    chain = np.stack([1.25 * np.arange(6), 0.8 * (np.arange(6) % 2), np.zeros(6)], 1)
    molecules = [(ring, [0] * 6), (np.concatenate([ring, methyl[None]]), [0] * 7), (ring, [2] + [0] * 5), (chain, [0] * 6)]
    x, mask, one_hot = np.full((4, 12, 3), 40.0, np.float32), np.zeros((4, 12), np.float32), np.zeros((4, 12, 8), np.float32)
    for b, (pos, types) in enumerate(molecules):
        at = b // 2
        x[b, at:at + len(pos)], mask[b, at:at + len(pos)] = pos, 1
        one_hot[b, np.arange(at, at + len(pos)), types] = 1
    linker = np.zeros((4, 12), np.float32)
    linker[1, 6] = 1                                                     # toluene: the methyl carbon
    linker[3, 1:4] = 1
    return one_hot, x, mask, linker


def on_bits_of(row):
    return set(np.nonzero(np.unpackbits(row.cpu().numpy().view(np.uint8), bitorder='little'))[0].tolist())


def test_analyze_fingerprints_on_hand_molecules():
    from difflinker_amd.metrics import analyze_fingerprints
    from difflinker_amd.molecule_builder import perceive_all_bonds
    one_hot, x, mask, linker = hand_batch()
    whole, alone = analyze_fingerprints(dev(one_hot), dev(x), dev(mask)[:, :, None], False, dev(linker)[:, :, None])
    found = perceive_all_bonds(dev(one_hot), dev(x), dev(mask), False)
    assert found.n_bonds.tolist() == [6, 7, 6, 5]
    lists = (one_hot, mask, found.bonds.cpu().numpy(), found.n_bonds.cpu().numpy(), found.status.cpu().numpy())
    assert_exact(whole._asdict(), fr.fingerprints(*lists), fr.FIELDS, 'every atom a centre')
    assert_exact(alone._asdict(), fr.fingerprints(*lists, centre_mask=linker), fr.FIELDS, 'the linker atoms the centres')
    assert on_bits_of(whole.bits[0]) == {92, 1852, 2031} == fr.on_bits(*fr.BENZENE), 'orders 1, 2, 1, 2, 1, 2 from the distances'
    assert on_bits_of(whole.bits[1]) == fr.on_bits(*fr.TOLUENE) and on_bits_of(alone.bits[1]) == {380, 1098, 2031}
    assert on_bits_of(whole.bits[3]) == fr.on_bits(*fr.HEXANE) and whole.n_on.tolist()[:2] == [3, 9] and whole.n_on.tolist()[3] == 6
    assert on_bits_of(whole.bits[2]) != on_bits_of(whole.bits[0]), 'pyridine is not benzene'
    assert alone.n_centres.tolist() == [0, 1, 0, 3] and alone.n_on.tolist()[0] == 0 and whole.status.tolist() == [0] * 4


def written(path, n_linker):
    """A written ``.sdf`` file as the reference takes a molecule: types, bonds, and the last ``n_linker`` atoms as centres."""
    from difflinker_amd import const
    from difflinker_amd.io import read_sdf_molecules
    (mol,), bad = read_sdf_molecules(path)
    assert bad == 0
    n = len(mol.symbols)
    return [const.ATOM2IDX[s] for s in mol.symbols], list(mol.bonds), [k >= n - n_linker for k in range(n)]


def prints_of(types, bonds, centres):
    as_int = lambda bits: sum(1 << k for k in bits)                            # noqa: E731
    return as_int(fr.on_bits(types, bonds)), as_int(fr.on_bits(types, bonds, centres=centres))


def similarity(a, b):
    c, u = fr.popcount(a & b), fr.popcount(a | b)
    return (c, u)


def expected_scores(samples, true=None):
    """``compute_diversity``'s keys from ``samples[input] = [(whole, linker), ...]`` (Python integers) in the order the
    drivers gather them: the inputs in order, and within a batch of two inputs sample by sample."""
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    q = lambda c, u: (c << 20) // u if u else 1 << 20                               # noqa: E731
    out = {'diversity_molecules': sum(len(rows) for rows in samples)}
    for view, tail in ((0, ''), (1, '_linker')):
        values = []
        for rows in samples:
            if len(rows) >= 2:
                total = sum(q(*similarity(rows[i][view], rows[j][view])) for i in range(len(rows)) for j in range(len(rows)) if i != j)
                values.append(1.0 - total / (len(rows) * (len(rows) - 1)) / (1 << 20))
        out['internal_diversity' + tail] = mean(values)
        if true is not None:
            order = [(g, k) for first in range(0, len(samples), 2) for k in range(len(samples[first]))
                     for g in range(first, min(first + 2, len(samples)))]
            pairs = [similarity(samples[g][k][view], true[g][view]) for g, k in order]
            out['similarity_to_true' + tail] = mean([1.0 if u == 0 else c / u for c, u in pairs])
    return out


def test_sample_writes_the_diversity_keys(tmp_path):
    from difflinker_amd.metrics import DIVERSITY_NAMES, DIVERSITY_REFERENCE_NAMES, DIVERSITY_TRUE_NAMES, METRIC_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_metrics import toy_dataset
    m = RG.gentle_model(tmp_path, False)
    keys = set(DIVERSITY_NAMES + DIVERSITY_TRUE_NAMES)
    out = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, output_format='both',
                 diversity=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == keys, 'alone when metrics are not asked for'
    samples = [[prints_of(*written(os.path.join(out, str(u), f'{i}_.sdf'), 3)) for i in range(2)] for u in range(5)]
    true = []
    for item in toy_dataset(5, 8):                                       # zigzag chains: single bonds between neighbours
        n = item['num_atoms']
        true.append(prints_of(item['one_hot'].argmax(1).tolist(), [(k, k + 1, 1) for k in range(n - 1)], [k >= n - 3 for k in range(n)]))
    assert got == expected_scores(samples, true)
    assert got['diversity_molecules'] == 10 and 0.0 <= got['internal_diversity'] <= got['internal_diversity_linker'] <= 1.0
    # against a reference set: the test set itself, so every true molecule is in it
    both = sample(m, str(tmp_path / 'both'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, output_format='both',
                  diversity_reference='zinc_final_test')
    got = json.load(open(os.path.join(both, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | keys | set(DIVERSITY_REFERENCE_NAMES)
    samples = [[prints_of(*written(os.path.join(both, str(u), f'{i}_.sdf'), 3)) for i in range(2)] for u in range(5)]
    want = expected_scores(samples, true)
    assert {k: got[k] for k in want} == want
    order = [(g, k) for first in range(0, 5, 2) for k in range(2) for g in range(first, min(first + 2, 5))]
    best = []
    for g, k in order:                                                   # the greatest fraction, compared exactly
        pairs = [similarity(samples[g][k][0], t[0]) for t in true]
        best.append(max(pairs, key=lambda cu: Fraction(cu[0], cu[1]) if cu[1] else Fraction(1)))
    assert got['nearest_reference_similarity'] == sum(1.0 if u == 0 else c / u for c, u in best) / 10
    assert got['nearest_reference_identical'] == sum(c == u for c, u in best) / 10
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}


def test_generate_writes_the_diversity_keys(tmp_path):
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import DIVERSITY_NAMES
    from difflinker_amd.noise import PredefinedNoiseSchedule
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    ddpm.edm.gamma = PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=0.05)   # the atoms stay within the file format
    frag = os.path.join(IO_DIR, 'frag.sdf')
    torch.manual_seed(11)
    files = generate(frag, ddpm, str(tmp_path / 'diverse'), n_samples=3, n_steps=5, linker_size='4', output_format='sdf', diversity=True)
    got = json.load(open(tmp_path / 'diverse' / 'metrics.json'))
    assert set(got) == set(DIVERSITY_NAMES), 'no true molecule here'
    assert len(files) == 3 and got == expected_scores([[prints_of(*written(path, 4)) for path in files]])
    assert got['diversity_molecules'] == 3 and 0.0 <= got['internal_diversity'] <= 1.0
    torch.manual_seed(11)
    generate(frag, ddpm, str(tmp_path / 'plain'), n_samples=3, n_steps=5, linker_size='4')
    assert not os.path.exists(tmp_path / 'plain' / 'metrics.json')


def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path):
    from difflinker_amd.metrics import DIVERSITY_NAMES, DIVERSITY_TRUE_NAMES, METRIC_NAMES
    m = RG.gentle_model(tmp_path, True)
    assert m.diversity_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.diversity_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(DIVERSITY_NAMES + DIVERSITY_TRUE_NAMES)
    assert {k: got[k] for k in METRIC_NAMES} == plain
    assert got['diversity_molecules'] == 5 * 3 and 0.0 <= got['internal_diversity'] <= 1.0 and 0.0 <= got['similarity_to_true'] <= 1.0
    json.dumps(got)
