"""Clusters and diverse subsets of fingerprint sets on the GPU (``dl_tanimoto_cluster`` and ``dl_tanimoto_pick``,
``csrc/select.hip``) against the plain-Python rules of ``tests/select_ref.py``.  Every output is an integer and every
comparison is exact; every output buffer holds 0x5a bytes before its launch.  Then the Python wrappers (a side stream, a
misaligned slice, another dtype) and the tools end to end: ``generate`` with ``cluster`` and ``pick`` on the synthetic
checkpoint (whose samples are never eligible) and behind a sampler of hand-made valid linkers, and ``sample``."""
import ctypes
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import fingerprint_ref as fr
import select_ref as sr
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STALE = 0x5a
WIDTHS = (16, 32, 64)
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def stale(shape, dtype=torch.int32):
    """An output buffer of ``shape`` whose every byte is 0x5a."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if t.numel():
        t.view(torch.uint8).fill_(STALE)
    return t


def assert_exact(got, want, fields, what=''):
    for name in fields:
        g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, (what, name, g.shape, g.dtype)
        assert np.array_equal(g, want[name]), (what, name, np.argwhere(g != want[name])[:5].tolist())


# ---- rows -----------------------------------------------------------------------------------------------------------------------

def random_rows(rng, m, w, density):
    return np.packbits(rng.random((m, w * 32)) < density, axis=1, bitorder='little').view(np.uint32).reshape(m, w)


def rows_of(bit_sets, w):
    """Rows from sets of bit numbers below 64; bit ``k`` goes to ``(37 k) mod (32 w)``, so every word of a wide row is used."""
    out = np.zeros((len(bit_sets), w), np.uint32)
    for r, bits in enumerate(bit_sets):
        for k in bits:
            at = (37 * k) % (32 * w)
            out[r, at // 32] |= np.uint32(1 << (at % 32))
    return out


def swapped(rng, row, n_swaps):
    """``row`` with ``n_swaps`` of its on-bits moved to off positions: similarity ``(p - s) / (p + s)`` to the original."""
    bits = np.unpackbits(row.view(np.uint8), bitorder='little').copy()
    on, off = np.nonzero(bits)[0], np.nonzero(bits == 0)[0]
    bits[rng.choice(on, n_swaps, replace=False)] = 0
    bits[rng.choice(off, n_swaps, replace=False)] = 1
    return np.packbits(bits, bitorder='little').view(np.uint32)


def planted_rows(rng, m, w, n_seeds=6, on=60, max_swaps=12):
    """Near-duplicates of a few seed rows of ``on`` bits: every row is a seed with 0 .. ``max_swaps`` of its bits moved, so
    that rows around one seed are neighbours at 0.65 or not depending on how far each went."""
    seeds = []
    for _ in range(n_seeds):
        row = np.zeros(w * 32, np.uint8)
        row[rng.choice(w * 32, on, replace=False)] = 1
        seeds.append(np.packbits(row, bitorder='little').view(np.uint32))
    rows = [swapped(rng, seeds[int(rng.integers(n_seeds))], int(rng.integers(0, max_swaps + 1))) for _ in range(m)]
    return np.stack(rows) if rows else np.zeros((0, w), np.uint32)


def bridged_rows(rng, m, w, n_seeds=3, on=60, path=24, stray=3):
    """Rows between pairs of seeds: each seed has a twin ``path`` swaps away (far from a neighbour at 0.65: 36 / 84), and
    every row is a seed with the first ``k`` of those swaps made: ``k`` near 0 or near ``path`` and up to ``stray`` swaps
    elsewhere for the two crowds at the ends, or exactly half way (48 / 72 to either end itself, and below 0.65 to a row that
    strayed further): a row that neighbours the middle of both crowds and few of their members."""
    rows = []
    ends = []
    for _ in range(n_seeds):
        bits = np.zeros(w * 32, np.uint8)
        bits[rng.choice(w * 32, on, replace=False)] = 1
        on_bits, off_bits = np.nonzero(bits)[0], np.nonzero(bits == 0)[0]
        ends.append((bits, rng.choice(on_bits, path, replace=False), rng.choice(off_bits, path, replace=False)))
    for _ in range(m):
        bits, leave, enter = ends[int(rng.integers(n_seeds))]
        k = int(rng.choice([0, 1, 2, path // 2, path - 2, path - 1, path], p=[.25, .1, .1, .1, .1, .1, .25]))
        row = bits.copy()
        row[leave[:k]], row[enter[:k]] = 0, 1
        extra = 0 if k == path // 2 else int(rng.choice([0, 0, 1, 2, stray]))
        rows.append(swapped(rng, np.packbits(row, bitorder='little').view(np.uint32), extra))
    return np.stack(rows)


def pooled_rows(rng, m, w, n_patterns=40):
    """``m`` rows drawn from ``n_patterns`` planted patterns: a large group whose reference costs a few dozen popcounts a row."""
    patterns = planted_rows(rng, n_patterns, w)
    return patterns[rng.integers(0, n_patterns, m)]


# ---- the C entry points -----------------------------------------------------------------------------------------------------------

def _set(bits, offsets):
    M = len(bits)
    G = 1 if offsets is None else max(len(offsets) - 1, 0)
    offsets = [0, M] if offsets is None else offsets
    return M, G, dev(bits.view(np.int32), torch.int32), dev(np.asarray(offsets, np.int32), torch.int32)


def cluster(bits, offsets=None, num=13, den=20):
    """``dl_tanimoto_cluster`` on output buffers full of 0x5a bytes, on torch's current stream."""
    from difflinker_amd import _lib
    M, G, bits_dev, off_dev = _set(bits, offsets)
    out = {name: stale((G,) if name in ('n_clusters', 'status') else (M,)) for name in sr.CLUSTER_FIELDS}
    pointers = {k: v.data_ptr() for k, v in {'bits': bits_dev, 'offsets': off_dev, **out}.items() if v.numel()}
    if G == 0:
        pointers.pop('offsets', None)
    args = _lib.DLClusterArgs(M=M, W=bits.shape[1], G=G, num=num, den=den, stream=torch.cuda.current_stream().cuda_stream,
                              **pointers)
    _lib.check(_lib.load().dl_tanimoto_cluster(ctypes.byref(args)), 'dl_tanimoto_cluster')
    return out


def pick(bits, k, offsets=None, first=None):
    """``dl_tanimoto_pick`` likewise."""
    from difflinker_amd import _lib
    M, G, bits_dev, off_dev = _set(bits, offsets)
    out = {name: stale((M,) if name == 'pick_rank' else (G,) if name in ('n_picked', 'status') else (G, k))
           for name in sr.PICK_FIELDS}
    ins = {'bits': bits_dev, 'offsets': off_dev}
    if first is not None:
        ins['first'] = dev(np.asarray(first, np.int32), torch.int32)
    pointers = {name: v.data_ptr() for name, v in {**ins, **out}.items() if v.numel()}
    if G == 0:
        pointers.pop('offsets', None)
    args = _lib.DLPickArgs(M=M, W=bits.shape[1], G=G, K=k, stream=torch.cuda.current_stream().cuda_stream, **pointers)
    _lib.check(_lib.load().dl_tanimoto_pick(ctypes.byref(args)), 'dl_tanimoto_pick')
    return out


# ---- every group size in one launch --------------------------------------------------------------------------------------------

SIZES = (0, 1, 2, 255, 256, 257, 4096, 4097)     # around the workgroup, DL_SELECT_MAX_ROWS and one past it
BEFORE, AFTER = 5, 7                             # rows in no group


def sizes_case(w):
    rng = np.random.default_rng(w)
    parts = [random_rows(rng, BEFORE, w, 0.1)]
    for n in SIZES:
        parts.append(pooled_rows(rng, n, w) if n >= 4096 else planted_rows(rng, n, w))
    parts.append(random_rows(rng, AFTER, w, 0.1))
    offsets = (BEFORE + np.concatenate([[0], np.cumsum(SIZES)])).tolist()
    return np.concatenate(parts), offsets


@pytest.fixture(scope='module', params=WIDTHS)
def sizes(request):
    """The case and both references, computed once per width."""
    bits, offsets = sizes_case(request.param)
    return bits, offsets, sr.clusters(bits, offsets, 13, 20), sr.picks(bits, 5, offsets)


def test_clusters_of_every_group_size(sizes):
    from difflinker_amd import _lib
    bits, offsets, want, _ = sizes
    assert want['status'].tolist() == [0] * 7 + [sr.TOO_LARGE] and sr.TOO_LARGE == _lib.DL_SELECT_TOO_LARGE
    assert want['n_clusters'][0] == 0 and want['n_clusters'][1] == 1 and want['n_clusters'][7] == 0
    assert (want['n_clusters'][3:7] >= 2).all() and want['n_neighbours'][offsets[6]:offsets[7]].max() > 255
    nothing = np.r_[0:BEFORE, offsets[7]:len(bits)]
    assert (want['cluster'][nothing] == -1).all() and (want['centroid'][nothing] == -1).all() and not want['n_neighbours'][nothing].any()
    assert (want['cluster'][BEFORE:offsets[7]] >= 0).all()
    assert_exact(cluster(bits, offsets), want, sr.CLUSTER_FIELDS, f'W {bits.shape[1]}')


def test_picks_of_every_group_size(sizes):
    bits, offsets, _, want = sizes
    assert want['n_picked'].tolist() == [0, 1, 2, 5, 5, 5, 5, 0] and want['status'].tolist() == [0] * 7 + [sr.TOO_LARGE]
    assert (want['picks'][1] == [offsets[1], -1, -1, -1, -1]).all(), 'K larger than the group'
    assert (want['pick_rank'][:BEFORE] == -1).all() and (want['pick_rank'][offsets[7]:] == -1).all()
    assert_exact(pick(bits, 5, offsets), want, sr.PICK_FIELDS, f'W {bits.shape[1]}')


@pytest.mark.parametrize('w', WIDTHS)
def test_no_group_and_no_rows(w):
    bits = random_rows(np.random.default_rng(w), 300, w, 0.1)
    want = sr.clusters(bits, [])
    assert (want['cluster'] == -1).all() and want['n_clusters'].shape == (0,)
    assert_exact(cluster(bits, []), want, sr.CLUSTER_FIELDS, 'no group')
    assert_exact(pick(bits, 3, []), sr.picks(bits, 3, []), sr.PICK_FIELDS, 'no group')
    none = bits[:0]
    assert_exact(cluster(none, [0, 0, 0]), sr.clusters(none, [0, 0, 0]), sr.CLUSTER_FIELDS, 'no rows')
    assert_exact(pick(none, 3, [0, 0, 0], first=[0, 0]), sr.picks(none, 3, [0, 0, 0], [0, 0]), sr.PICK_FIELDS, 'no rows')
    # offsets below zero and beyond M are clamped
    wild = [-(1 << 31), 120, (1 << 31) - 1]
    assert_exact(cluster(bits, wild), sr.clusters(bits, wild), sr.CLUSTER_FIELDS, 'clamped')
    assert_exact(pick(bits, 4, wild), sr.picks(bits, 4, wild), sr.PICK_FIELDS, 'clamped')


# ---- ties -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('w', WIDTHS)
def test_identical_rows_and_empty_rows(w):
    """Every tie rule at once: a group of equal rows, a group of empty rows (u == 0), and a group of both."""
    rng = np.random.default_rng(10 + w)
    one = random_rows(rng, 1, w, 0.2)
    bits = np.concatenate([np.repeat(one, 300, 0), np.zeros((300, w), np.uint32), np.repeat(one, 3, 0), np.zeros((3, w), np.uint32)])
    offsets = [0, 300, 600, 606]
    want = sr.clusters(bits, offsets)
    assert want['n_clusters'].tolist() == [1, 1, 2] and want['n_neighbours'].tolist() == [299] * 600 + [2] * 6
    assert want['centroid'].tolist() == [0] * 300 + [300] * 300 + [600] * 3 + [603] * 3, 'the lowest row of equal ones'
    assert_exact(cluster(bits, offsets), want, sr.CLUSTER_FIELDS, 'equal rows')
    picks = sr.picks(bits, 4, offsets)
    assert picks['picks'].tolist() == [[0, 1, 2, 3], [300, 301, 302, 303], [600, 603, 601, 602]]
    assert picks['pick_union'][1].tolist() == [-1, 0, 0, 0], 'u == 0 is reported as it is'
    assert_exact(pick(bits, 4, offsets), picks, sr.PICK_FIELDS, 'equal rows')


@pytest.mark.parametrize('w', WIDTHS)
def test_the_threshold_tie(w):
    """Three pairs, a group each: c / u is 13 / 20, 13 / 21 and 13 / 19 against the threshold 65 / 100."""
    shared = set(range(13))
    pairs = [(shared | {13, 14, 15}, shared | {16, 17, 18, 19}),          # u = 13 + 3 + 4
             (shared | {13, 14, 15}, shared | {16, 17, 18, 19, 20}),      # one bit more in the union: below
             (shared | {13, 14, 15}, shared | {16, 17, 18})]              # one bit fewer: above
    bits = rows_of([s for pair in pairs for s in pair], w)
    ints = fr.row_ints(bits)
    assert [sr.Pairs()(ints[2 * k], ints[2 * k + 1]) for k in range(3)] == [(13, 20), (13, 21), (13, 19)]
    offsets = [0, 2, 4, 6]
    want = sr.clusters(bits, offsets, 65, 100)
    assert want['n_neighbours'].tolist() == [1, 1, 0, 0, 1, 1] and want['n_clusters'].tolist() == [1, 2, 1]
    assert_exact(cluster(bits, offsets, 65, 100), want, sr.CLUSTER_FIELDS, '65 / 100')
    assert_exact(cluster(bits, offsets, 13, 20), want, sr.CLUSTER_FIELDS, 'the same threshold in lowest terms')
    assert_exact(cluster(bits, offsets, 65000, 65536), sr.clusters(bits, offsets, 65000, 65536), sr.CLUSTER_FIELDS, 'the largest den')


def planted_case(w):
    rng = np.random.default_rng(500 + w)
    return np.concatenate([bridged_rows(rng, 210, w), planted_rows(rng, 90, w)]), [0, 210, 300]


@pytest.mark.parametrize('w', WIDTHS)
def test_planted_near_duplicates(w):
    """Random sparse rows alone would be singletons: near-duplicates of a few seeds, and the reference's own result is
    checked to be a real clustering before anything is compared with it."""
    bits, offsets = planted_case(w)
    want = sr.clusters(bits, offsets)
    ints, pairs = fr.row_ints(bits), sr.Pairs()
    neighbours = lambda i, j: (lambda c, u: c * 20 >= 13 * u)(*pairs(ints[i], ints[j]))      # noqa: E731
    lo, hi = offsets[0], offsets[1]
    sizes = np.bincount(want['cluster'][lo:hi])
    assert want['n_clusters'][0] >= 2 and sizes.max() >= 3
    centroids = sorted(set(want['centroid'][lo:hi].tolist()))
    torn = [i for i in range(lo, hi) if i not in centroids and sum(neighbours(i, c) for c in centroids) >= 2]
    assert torn, 'a member that neighbours two centroids'
    assert all(want['centroid'][i] == min((c for c in centroids if neighbours(i, c)), key=lambda c: want['cluster'][c])
               for i in torn), 'it belongs to the earlier one'
    assert len(set(want['n_neighbours'][lo:hi].tolist())) < hi - lo, 'two rows tie on n_neighbours'
    assert_exact(cluster(bits, offsets), want, sr.CLUSTER_FIELDS, 'planted')
    assert_exact(cluster(bits, offsets, 4, 5), sr.clusters(bits, offsets, 4, 5), sr.CLUSTER_FIELDS, 'planted, 0.8')
    first = [offsets[0] + 17, offsets[2] - 1]
    assert_exact(pick(bits, 100, offsets, first), sr.picks(bits, 100, offsets, first), sr.PICK_FIELDS, 'planted picks')


# ---- picks ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('w', WIDTHS)
def test_pick_cases(w):
    from difflinker_amd import _lib
    a = {0, 1, 2, 3}
    hand = [a, {20, 21, 22}, {20, 21, 22}, {0, 1, 2, 30}]                 # the second and the third tie on m(i) after the first
    ratio = [a, {0, 1}, {0, 1, 2, 10, 11}, {40}]                          # 2 / 4 and 3 / 6: equal fractions of different (c, u)
    rng = np.random.default_rng(20 + w)
    bits = np.concatenate([rows_of(hand + ratio, w), planted_rows(rng, 5, w), planted_rows(rng, 40, w)])
    offsets = [0, 4, 8, 13, 53]
    want = sr.picks(bits, 9, offsets)
    assert want['picks'][0].tolist() == [0, 1, 3, 2] + [-1] * 5, 'of two rows that tie on m(i) the lower; its twin goes last'
    assert want['pick_common'][0].tolist()[:4] == [-1, 0, 3, 3] and want['pick_union'][0].tolist()[:4] == [-1, 7, 5, 3]
    assert want['picks'][1].tolist()[:4] == [4, 7, 5, 6] and (want['pick_common'][1, 2], want['pick_union'][1, 2]) == (2, 4)
    assert want['n_picked'].tolist() == [4, 4, 5, 9], 'K larger than three of the groups'
    assert_exact(pick(bits, 9, offsets), want, sr.PICK_FIELDS, 'no first')
    one = sr.picks(bits, 1, offsets)
    assert one['picks'].tolist() == [[0], [4], [8], [13]] and one['pick_rank'].tolist().count(0) == 4
    assert_exact(pick(bits, 1, offsets), one, sr.PICK_FIELDS, 'K = 1')
    first = [3, 8, 12, 30]                                               # group 1: a row of group 2 - outside
    given = sr.picks(bits, 9, offsets, first)
    assert given['status'].tolist() == [0, sr.BAD_FIRST, 0, 0] and sr.BAD_FIRST == _lib.DL_SELECT_BAD_FIRST
    assert given['picks'][:, 0].tolist() == [3, -1, 12, 30] and given['n_picked'].tolist() == [4, 0, 5, 9]
    assert (given['pick_rank'][4:8] == -1).all()
    assert_exact(pick(bits, 9, offsets, first), given, sr.PICK_FIELDS, 'first given')
    low = [-1, 3, 13, 53]                                                # one before and one past the group
    assert sr.picks(bits, 2, offsets, low)['status'].tolist() == [sr.BAD_FIRST] * 4
    assert_exact(pick(bits, 2, offsets, low), sr.picks(bits, 2, offsets, low), sr.PICK_FIELDS, 'every first outside')
    assert_exact(pick(bits, 4096, offsets), sr.picks(bits, 4096, offsets), sr.PICK_FIELDS, 'the largest K')


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------

def test_the_python_wrappers():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import Clusters, Picks, tanimoto_clusters, tanimoto_picks
    bits, offsets = planted_case(32)
    bits_dev, off_dev = dev(bits.view(np.int32), torch.int32), dev(offsets, torch.int32)
    got = tanimoto_clusters(bits_dev, off_dev)
    assert isinstance(got, Clusters) and (got.num, got.den) == (13, 20)
    assert_exact(got._asdict(), sr.clusters(bits, offsets), sr.CLUSTER_FIELDS, 'groups')
    got = tanimoto_clusters(bits_dev, threshold=0.8)
    assert (got.num, got.den) == (4, 5)
    assert_exact(got._asdict(), sr.clusters(bits, None, 4, 5), sr.CLUSTER_FIELDS, 'one group over everything')
    first = dev([5, 299], torch.int32)
    got = tanimoto_picks(bits_dev, 7, off_dev, first)
    assert isinstance(got, Picks)
    assert_exact(got._asdict(), sr.picks(bits, 7, offsets, [5, 299]), sr.PICK_FIELDS, 'groups, first given')
    assert_exact(tanimoto_picks(bits_dev, 3)._asdict(), sr.picks(bits, 3), sr.PICK_FIELDS, 'one group over everything')
    # a row set that is aligned to 4 bytes only: the wrappers clone it, the C entry points refuse it
    flat = torch.zeros(bits.size + 1, dtype=torch.int32, device=DEV)
    shifted = flat[1:].view(bits.shape)
    shifted.copy_(bits_dev)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert_exact(tanimoto_clusters(shifted, off_dev)._asdict(), sr.clusters(bits, offsets), sr.CLUSTER_FIELDS, 'misaligned')
    assert_exact(tanimoto_picks(shifted, 7, off_dev, first)._asdict(), sr.picks(bits, 7, offsets, [5, 299]), sr.PICK_FIELDS, 'misaligned')
    out = stale((300,))
    per_group = stale((2, 7))
    refused = _lib.DLClusterArgs(M=300, W=32, G=2, bits=shifted.data_ptr(), offsets=off_dev.data_ptr(), num=13, den=20,
                                 cluster=out.data_ptr(), centroid=out.data_ptr(), n_neighbours=out.data_ptr(),
                                 n_clusters=per_group.data_ptr(), status=per_group.data_ptr())
    assert _lib.load().dl_tanimoto_cluster(ctypes.byref(refused)) == BAD_ARG
    refused = _lib.DLPickArgs(M=300, W=32, G=2, K=7, bits=shifted.data_ptr(), offsets=off_dev.data_ptr(),
                              picks=per_group.data_ptr(), pick_common=per_group.data_ptr(), pick_union=per_group.data_ptr(),
                              n_picked=per_group.data_ptr(), status=per_group.data_ptr(), pick_rank=out.data_ptr())
    assert _lib.load().dl_tanimoto_pick(ctypes.byref(refused)) == BAD_ARG
    torch.cuda.synchronize()
    assert (out.cpu().view(torch.uint8) == STALE).all(), 'a refused call writes nothing'
    # a strided view of a wider set is taken as it is; another dtype is refused
    wide = torch.zeros(300, 40, dtype=torch.int32, device=DEV)
    wide[:, 3:35] = bits_dev
    assert_exact(tanimoto_clusters(wide[:, 3:35], off_dev)._asdict(), sr.clusters(bits, offsets), sr.CLUSTER_FIELDS, 'strided')
    for other in (torch.int64, torch.uint8, torch.float32):
        with pytest.raises(ValueError, match='int32 words'):
            tanimoto_clusters(bits_dev.to(other), off_dev)
        with pytest.raises(ValueError, match='int32 words'):
            tanimoto_picks(bits_dev.to(other), 3, off_dev)
    with pytest.raises(ValueError):
        tanimoto_picks(bits_dev, 0)
    with pytest.raises(ValueError):
        tanimoto_clusters(bits_dev, threshold='1.5')


@pytest.mark.parametrize('w', [16, 64])
def test_clusters_on_a_side_stream(monkeypatch, delay, w):  # noqa: F811
    """Part A of tests/test_gpu_streams.py for the wrapper: the inputs hold poison until copies queued on the side stream
    behind a delay have written them, the outputs are read on that stream, and equal the default stream's bits."""
    from difflinker_amd.metrics import tanimoto_clusters
    bits, offsets = planted_case(w)
    call = lambda: tanimoto_clusters(dev(bits.view(np.int32), torch.int32), dev(offsets, torch.int32))      # noqa: E731
    base = GS.check_stream_contract(lambda: GS._through_dev(sys.modules[__name__], call)(monkeypatch), delay)
    assert_exact(base, sr.clusters(bits, offsets), sr.CLUSTER_FIELDS, 'the baseline')


@pytest.mark.parametrize('w', [16, 64])
def test_picks_on_a_side_stream(monkeypatch, delay, w):  # noqa: F811
    from difflinker_amd.metrics import tanimoto_picks
    bits, offsets = planted_case(w)
    call = lambda: tanimoto_picks(dev(bits.view(np.int32), torch.int32), 20, dev(offsets, torch.int32),      # noqa: E731
                                  dev([9, 250], torch.int32))
    base = GS.check_stream_contract(lambda: GS._through_dev(sys.modules[__name__], call)(monkeypatch), delay)
    assert_exact(base, sr.picks(bits, 20, offsets, [9, 250]), sr.PICK_FIELDS, 'the baseline')


# ---- the public path ------------------------------------------------------------------------------------------------------------

def eligible_file(path, is_geom):
    """Is the written molecule valid under the valence rule and in one piece?  From the file alone."""
    from difflinker_amd import const
    from test_gpu_fingerprint import written
    types, bonds, _ = written(path, 0)
    limits = const.max_valence_table(is_geom).tolist()
    valence, root = [0] * len(types), list(range(len(types)))

    def find(k):
        while root[k] != k:
            k = root[k]
        return k
    for i, j, order in bonds:
        valence[i] += order
        valence[j] += order
        root[find(i)] = find(j)
    return all(v <= limits[t] for v, t in zip(valence, types)) and len({find(k) for k in range(len(types))}) == 1


def synthetic_ddpm():
    """The synthetic checkpoint of ``tests/test_gpu_generate.py``, as ``test_gpu_fingerprint`` sets it up."""
    from difflinker_amd import DDPM
    from difflinker_amd.noise import PredefinedNoiseSchedule
    from test_gpu_generate import ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    ddpm.edm.gamma = PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=0.05)   # the atoms stay within the file format
    return ddpm


def run_twice(ddpm, tmp_path, n_samples, frag=None, **flags):
    """``generate`` without and with the flags, same seed: the file names, after checking that the flags changed no file and
    added ``selection.json`` and ``metrics.json`` alone."""
    from difflinker_amd.generate import generate
    from test_gpu_generate import IO_DIR
    frag = frag or os.path.join(IO_DIR, 'frag.sdf')
    torch.manual_seed(11)
    plain = generate(frag, ddpm, str(tmp_path / 'plain'), n_samples=n_samples, n_steps=5, linker_size='4', output_format='sdf')
    torch.manual_seed(11)
    files = generate(frag, ddpm, str(tmp_path / 'chosen'), n_samples=n_samples, n_steps=5, linker_size='4', output_format='sdf',
                     **flags)
    names = [os.path.basename(path) for path in files]
    assert names == [os.path.basename(path) for path in plain] and len(names) == n_samples
    for name in sorted(os.listdir(tmp_path / 'plain')):
        assert filecmp.cmp(tmp_path / 'plain' / name, tmp_path / 'chosen' / name, shallow=False), name
    assert set(os.listdir(tmp_path / 'chosen')) - set(os.listdir(tmp_path / 'plain')) == {'selection.json', 'metrics.json'}
    assert not os.path.exists(tmp_path / 'plain' / 'selection.json')
    return files, names


def check_selection(files, names, got, scores, is_geom, k):
    """``selection.json`` and the ``metrics.json`` keys against the files alone: eligibility from the written bonds, fingerprints
    with the four linker atoms as centres, and the plain-Python rules on them.  Returns the eligible samples."""
    from difflinker_amd.metrics import SELECTION_NAMES, SelectRecord
    from test_gpu_fingerprint import prints_of, written
    assert set(got) == set(names) | {'picked', 'clusters'}
    assert all(set(got[name]) == set(SelectRecord._fields) for name in names)
    eligible = [eligible_file(path, is_geom) for path in files]
    assert [got[name]['eligible'] for name in names] == eligible
    rows = [at for at in range(len(files)) if eligible[at]]
    for at in range(len(files)):
        if not eligible[at]:
            assert all(got[names[at]][field] is None for field in SelectRecord._fields[2:]), 'never clustered, never picked'
    assert set(scores) == set(SELECTION_NAMES) and scores['selection_molecules'] == len(rows)
    if not rows:
        assert got['picked'] == [] and got['clusters'] == [] and scores['clusters_per_input'] is None
        return rows
    linker = [prints_of(*written(files[at], 4))[1] for at in rows]
    bits = np.array([[(v >> (32 * word)) & 0xFFFFFFFF for word in range(64)] for v in linker], np.uint32)
    near = fr.tanimoto_nearest(bits, bits, exclude_diagonal=True)
    first = int(np.argmax(near['sum_q20']))                              # the first of the greatest sums
    clusters, picks = sr.clusters(bits, None, 13, 20), sr.picks(bits, k, None, [first])
    for at, sample in enumerate(rows):
        record = got[names[sample]]
        assert (record['cluster'], record['n_neighbours']) == (clusters['cluster'][at], clusters['n_neighbours'][at]), names[sample]
        assert record['is_centroid'] == (clusters['centroid'][at] == at)
        assert record['cluster_size'] == int((clusters['cluster'] == clusters['cluster'][at]).sum())
        rank = int(picks['pick_rank'][at])
        assert record['pick_rank'] == (rank if rank >= 0 else None)
        c, u = (int(picks[name][0, rank]) for name in ('pick_common', 'pick_union')) if rank > 0 else (None, None)
        assert record['pick_similarity'] == (None if c is None else 1.0 if u == 0 else c / u)
    members = [name for entry in got['clusters'] for name in entry['members']]
    assert sorted(members) == sorted(names[sample] for sample in rows), 'the clusters partition the eligible files'
    assert all(entry['centroid'] in entry['members'] for entry in got['clusters']) and len(got['clusters']) == clusters['n_clusters'][0]
    assert got['picked'] == [names[rows[at]] for at in picks['picks'][0] if at >= 0]
    assert len(set(got['picked'])) == len(got['picked']) == min(k, len(rows)) and got['picked'][0] == names[rows[first]]
    assert scores['clusters_per_input'] == clusters['n_clusters'][0]
    assert scores['largest_cluster_share'] == np.bincount(clusters['cluster']).max() / len(rows)
    return rows


def test_generate_with_the_flags_changes_no_file(tmp_path):
    """The sampler itself, on the synthetic checkpoint and ``frag.sdf``.  No sample of this pair is ever eligible: the
    untrained denoiser leaves the linker atoms far from the fragments, and the oxygen of ``frag.sdf`` is 1.58 A from its carbon,
    a piece of its own under the bond table (0 eligible of 64 samples at each of four seeds and three linker sizes).  So every
    record says "not eligible" here, and the checks on eligible samples are those of the next test."""
    ddpm = synthetic_ddpm()
    files, names = run_twice(ddpm, tmp_path, 3, cluster='0.65', pick=3)
    got = json.load(open(tmp_path / 'chosen' / 'selection.json'))
    scores = json.load(open(tmp_path / 'chosen' / 'metrics.json'))
    check_selection(files, names, got, scores, ddpm.is_geom, 3)


LINKERS = ('CCCC', 'CCCC', 'CNCC', 'CCOC', None, 'CCCC', 'NCCO', 'OCCC', None)     # None: a linker that bridges nothing


BRIDGE_SDF = """two_sane_fragments
  handmade          3D

  5  3  0  0  0  0  0  0  0  0999 V2000
    1.2000    0.0000    0.1000 C   0  0  0  0  0  0  0  0  0  0  0  0
    2.6000    0.4000   -0.2000 C   0  0  0  0  0  0  0  0  0  0  0  0
    3.2000    1.7000    0.2000 N   0  0  0  0  0  0  0  0  0  0  0  0
   -4.0000    0.5000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0
   -5.3000    1.2000    0.3000 C   0  0  0  0  0  0  0  0  0  0  0  0
  1  2  1  0
  2  3  1  0
  4  5  1  0
M  END
$$$$
"""                                              # every bond 1.49 - 1.51 A; atoms 0 and 3 are 5.2 A apart


def bridging_chain(data, ddpm):
    """What ``DDPM.sample_chain`` returns for the batch ``data`` of ``BRIDGE_SDF``, with hand-made linkers in place of sampled
    ones: four atoms on a circular arc from atom 0 to atom 3, every chord 1.5 A (a single bond for C, N and O alike; atoms
    two apart are 2.9 A from each other), types from ``LINKERS``."""
    from difflinker_amd import const
    positions, one_hot = data['positions'], data['one_hot']
    B, n_frag, nf = one_hot.shape
    a, b = positions[0, 0].cpu().numpy().astype(np.float64), positions[0, 3].cpu().numpy().astype(np.float64)
    span = np.linalg.norm(b - a)
    theta = 0.5
    for _ in range(60):                                                  # 5 chords of 1.5 span |b - a|: Newton on the angle
        f = 1.5 * np.sin(2.5 * theta) / np.sin(0.5 * theta) - span
        df = 1.5 * (2.5 * np.cos(2.5 * theta) * np.sin(0.5 * theta) - 0.5 * np.sin(2.5 * theta) * np.cos(0.5 * theta)) / np.sin(0.5 * theta) ** 2
        theta -= f / df
    radius = 0.75 / np.sin(0.5 * theta)
    along = (b - a) / span
    up = np.cross([0.0, 1.0, 0.0], along)
    up /= np.linalg.norm(up)
    centre = (a + b) / 2 - up * radius * np.cos(2.5 * theta)
    arc = [centre + radius * (np.sin((k - 2.5) * theta) * along + np.cos((k - 2.5) * theta) * up) for k in range(1, 5)]
    assert abs(np.linalg.norm(arc[0] - a) - 1.5) < 1e-9 and abs(np.linalg.norm(arc[3] - b) - 1.5) < 1e-9
    x = torch.zeros(B, n_frag + 4, 3, device=positions.device)
    h = torch.zeros(B, n_frag + 4, nf, device=positions.device)
    x[:, :n_frag], h[:, :n_frag] = positions, one_hot
    for k in range(B):
        symbols = LINKERS[k % len(LINKERS)]
        shift = np.zeros(3) if symbols else 9.0 * up
        x[k, n_frag:] = torch.as_tensor(np.stack(arc) + shift, dtype=x.dtype)
        for at, symbol in enumerate(symbols or 'CCCC'):
            h[k, n_frag + at, const.ATOM2IDX[symbol]] = 1
    x = x - positions.mean(1, keepdim=True)                              # the frame of the chain: the fragments' centre of mass
    return torch.cat([x, h], 2)[None], torch.ones(B, n_frag + 4, 1, device=positions.device)


def test_generate_selects_among_valid_samples(tmp_path, monkeypatch):
    """``generate`` end to end behind the sampler: hand-made linkers that bridge the two fragments stand in for sampled ones, so
    that there are valid samples in one piece to cluster and to pick from, equal ones, different ones and broken ones."""
    ddpm = synthetic_ddpm()
    monkeypatch.setattr(ddpm, 'sample_chain', lambda data, sample_fn=None, keep_frames=None: bridging_chain(data, ddpm), raising=False)
    with open(tmp_path / 'bridge.sdf', 'w') as f:
        f.write(BRIDGE_SDF)
    files, names = run_twice(ddpm, tmp_path, len(LINKERS), frag=str(tmp_path / 'bridge.sdf'), cluster='0.65', pick=3)
    got = json.load(open(tmp_path / 'chosen' / 'selection.json'))
    scores = json.load(open(tmp_path / 'chosen' / 'metrics.json'))
    rows = check_selection(files, names, got, scores, ddpm.is_geom, 3)
    assert rows == [at for at, symbols in enumerate(LINKERS) if symbols], 'the bridging linkers are eligible, the others are not'
    assert got[names[0]]['cluster'] == got[names[1]]['cluster'] == got[names[5]]['cluster'], 'equal molecules share a cluster'
    assert len(got['clusters']) >= 2 and len(got['picked']) == 3 and not {names[4], names[8]} & set(got['picked'])


def test_sample_writes_the_selection(tmp_path):
    """``sample`` with the flags on the toy data set: the inputs are the groups, ``metrics.json`` gets the four keys alone,
    ``selection.json`` a record per written file, and the files are those of a run without the flags."""
    import test_gpu_rings as RG
    from difflinker_amd.metrics import SELECTION_NAMES, SelectRecord
    from difflinker_amd.sample import sample
    m = RG.gentle_model(tmp_path, False)
    m.edm.noise_seed = 5
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, output_format='sdf')
    m.edm.noise_seed = 5
    out = sample(m, str(tmp_path / 'chosen'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, output_format='sdf',
                 cluster='0.65', pick=1, select_view='whole')
    names = sorted(os.path.join(u, name) for u in os.listdir(out) if os.path.isdir(os.path.join(out, u))
                   for name in os.listdir(os.path.join(out, u)))
    for name in names:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain))) == ['metrics.json', 'selection.json']
    scores = json.load(open(os.path.join(out, 'metrics.json')))
    got = json.load(open(os.path.join(out, 'selection.json')))
    sampled = [name for name in names if name.endswith('_.sdf')]
    assert set(scores) == set(SELECTION_NAMES) and set(got) == set(sampled) | {'picked', 'clusters'} and len(sampled) == 10
    eligible = {name: eligible_file(os.path.join(out, name), m.is_geom) for name in sampled}
    assert {name: got[name]['eligible'] for name in sampled} == eligible and scores['selection_molecules'] == sum(eligible.values())
    inputs = {name: got[name]['input'] for name in sampled}
    assert all(inputs[name] == name.split(os.sep)[0] for name in sampled), 'the groups are the inputs'
    with_eligible = {inputs[name] for name in sampled if eligible[name]}
    assert sorted(got[name]['input'] for name in got['picked']) == sorted(with_eligible), 'one pick per input that has a sample'
    assert all(got[name]['pick_rank'] == 0 and got[name]['pick_similarity'] is None for name in got['picked'])
    for name in sampled:
        record = got[name]
        assert set(record) == set(SelectRecord._fields)
        assert (record['cluster'] is not None) == eligible[name] and (record['pick_rank'] is not None) == (name in got['picked'])
    members = [name for entry in got['clusters'] for name in entry['members']]
    assert sorted(members) == sorted(name for name in sampled if eligible[name])
    only = sample(m, str(tmp_path / 'clusters'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, cluster='0.65')
    assert not os.path.exists(os.path.join(only, 'selection.json')) and set(json.load(open(os.path.join(only, 'metrics.json')))) == set(SELECTION_NAMES)
