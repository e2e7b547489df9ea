"""Clusters and diverse subsets without a GPU: the plain-Python rules of ``tests/select_ref.py`` on hand cases with known
answers, the ABI of ``dl_tanimoto_cluster`` and ``dl_tanimoto_pick`` (struct layout, exports, constants, every argument check
- they all come before any device work), ``metrics.select_records`` / ``compute_selection`` / ``selection_report`` on stubbed
device results, the threshold's fraction and the command lines."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import fingerprint_ref as fr
import select_ref as sr
from difflinker_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


def rows(*bit_sets, w=16):
    out = np.zeros((len(bit_sets), w), np.uint32)
    for r, bits in enumerate(bit_sets):
        for k in bits:
            out[r, k // 32] |= np.uint32(1 << (k % 32))
    return out


# ---- the reference itself -----------------------------------------------------------------------------------------------------

def test_three_identical_rows_and_a_far_one():
    same = set(range(10))
    got = sr.clusters(rows(same, {100, 101}, same, same))
    assert got['n_clusters'].tolist() == [2] and got['status'].tolist() == [0]
    assert got['cluster'].tolist() == [0, 1, 0, 0] and got['centroid'].tolist() == [0, 1, 0, 0], 'the lowest of equal rows'
    assert got['n_neighbours'].tolist() == [2, 0, 2, 2]


def test_a_neighbour_of_two_centroids_belongs_to_the_earlier_one():
    """X and Y are far apart, each with a crowd of its own; Z lies half way: 16 / 24 to X and to Y, and 15 / 25 to every
    member of either crowd.  X has the most neighbours and comes first, so Z is its member - not Y's, the lower row."""
    x, y, z = set(range(0, 20)), set(range(8, 28)), set(range(4, 24))
    crowd_x = [x - {19 - k} | {200 + k} for k in range(3)]                # 19 / 21 to X, 18 / 22 to each other
    crowd_y = [y - {8 + k} | {300 + k} for k in range(2)]
    got = sr.clusters(rows(y, *crowd_y, z, x, *crowd_x))
    assert got['n_neighbours'].tolist() == [3, 2, 2, 2, 4, 3, 3, 3]
    assert got['centroid'].tolist() == [0, 0, 0, 4, 4, 4, 4, 4] and got['cluster'].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert got['n_clusters'].tolist() == [2]
    # at 2 / 3 the pair Z - X (16 / 24) is still a neighbour, exactly; at 0.67 it is not, and Z is a cluster of its own
    assert sr.clusters(rows(y, *crowd_y, z, x, *crowd_x), num=2, den=3)['centroid'].tolist() == [0, 0, 0, 4, 4, 4, 4, 4]
    alone = sr.clusters(rows(y, *crowd_y, z, x, *crowd_x), num=67, den=100)
    assert alone['n_neighbours'].tolist() == [2, 2, 2, 0, 3, 3, 3, 3] and alone['cluster'].tolist() == [1, 1, 1, 2, 0, 0, 0, 0]


def test_maxmin_on_four_rows():
    a = {0, 1, 2, 3}
    got = sr.picks(rows(a, {20, 21, 22}, {20, 21, 22}, {0, 1, 2, 30}), 4)
    assert got['picks'].tolist() == [[0, 1, 3, 2]] and got['pick_rank'].tolist() == [0, 1, 3, 2]
    assert got['pick_common'].tolist() == [[-1, 0, 3, 3]] and got['pick_union'].tolist() == [[-1, 7, 5, 3]]
    started = sr.picks(rows(a, {20, 21, 22}, {20, 21, 22}, {0, 1, 2, 30}), 2, first=[3])
    assert started['picks'].tolist() == [[3, 1]] and started['pick_rank'].tolist() == [-1, 1, -1, 0]
    ratio = sr.picks(rows(a, {0, 1}, {0, 1, 2, 10, 11}), 2)              # 2 / 4 and 3 / 6: the lower row
    assert ratio['picks'].tolist() == [[0, 1]] and (ratio['pick_common'][0, 1], ratio['pick_union'][0, 1]) == (2, 4)


def test_more_picks_than_rows_an_empty_group_and_the_limits():
    bits = rows({0}, {1}, {2}, {3}, {4})
    got = sr.picks(bits, 4, [0, 2, 2, 5])
    assert got['n_picked'].tolist() == [2, 0, 3] and got['picks'].tolist() == [[0, 1, -1, -1], [-1] * 4, [2, 3, 4, -1]]
    assert got['status'].tolist() == [0, 0, 0] and got['pick_rank'].tolist() == [0, 1, 0, 1, 2]
    assert sr.picks(bits, 2, [0, 2, 2, 5], first=[1, 99, 5])['status'].tolist() == [0, 0, sr.BAD_FIRST], 'an empty group has no first'
    found = sr.clusters(bits, [1, 1, 3])
    assert found['n_clusters'].tolist() == [0, 2] and found['cluster'].tolist() == [-1, 0, 1, -1, -1]
    assert found['centroid'].tolist() == [-1, 1, 2, -1, -1] and found['n_neighbours'].tolist() == [0] * 5
    big = np.zeros((sr.MAX_ROWS + 1, 16), np.uint32)
    assert sr.clusters(big)['status'].tolist() == [sr.TOO_LARGE] and (sr.clusters(big)['cluster'] == -1).all()
    assert sr.picks(big, 3)['status'].tolist() == [sr.TOO_LARGE] and sr.picks(big, 3)['n_picked'].tolist() == [0]
    assert sr.clusters(big[:-1])['n_clusters'].tolist() == [1], 'empty rows are neighbours'


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_sample_chain_fc_join')
    assert _lib.EXPORTS[at + 1:at + 4] == ('dl_tanimoto_cluster', 'dl_tanimoto_pick', 'dl_bonds_workspace_bytes')
    assert _lib.EXPORTS[-1] == 'dl_best_rmsd'
    # their own table beside STRUCT_ENTRY_POINTS (tests/test_lib_host.py pins that one name by name), declared the same way
    assert _lib.SELECT_ENTRY_POINTS == {'dl_tanimoto_cluster': _lib.DLClusterArgs, 'dl_tanimoto_pick': _lib.DLPickArgs}
    assert not set(_lib.SELECT_ENTRY_POINTS) & set(_lib.STRUCT_ENTRY_POINTS) and set(_lib.SELECT_ENTRY_POINTS) <= set(_lib.EXPORTS)
    for name, struct in _lib.SELECT_ENTRY_POINTS.items():
        fn = getattr(_lib.load(), name)
        assert fn.restype is ctypes.c_int32 and fn.argtypes == [ctypes.POINTER(struct)], name
        assert _lib.entry_struct(name) is struct and _lib._stream_is_field(struct)
    assert _lib.entry_struct('dl_tanimoto_nearest') is _lib.DLTanimotoArgs
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_tanimoto_cluster(const dl_cluster_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert 'int32_t dl_tanimoto_pick(const dl_pick_args* args);' in header
    opening = header.split('#ifndef DIFFLINKER_HIP_H')[0]
    for name in ('dl_tanimoto_cluster', 'dl_tanimoto_pick'):
        assert re.search(rf' \*   {name} +<- \(no reference counterpart\)', opening), 'listed in the opening comment'
    for name, value in (('DL_SELECT_MAX_ROWS', 4096), ('DL_SELECT_TOO_LARGE', 4), ('DL_SELECT_BAD_FIRST', 16)):
        assert re.search(rf'#define {name} {value}\s', header) and getattr(_lib, name) == value
    assert (sr.MAX_ROWS, sr.TOO_LARGE, sr.BAD_FIRST) == (_lib.DL_SELECT_MAX_ROWS, _lib.DL_SELECT_TOO_LARGE, _lib.DL_SELECT_BAD_FIRST)
    lib = _lib.load()
    assert hasattr(lib, 'dl_tanimoto_cluster') and hasattr(lib, 'dl_tanimoto_pick') and lib.dl_abi_version() == 7
    for struct, args in (('dl_cluster_args', _lib.DLClusterArgs), ('dl_pick_args', _lib.DLPickArgs)):
        body = header.split('typedef struct %s {' % struct)[1].split('} %s;' % struct)[0]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = [n for line in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', line.strip().split('*')[-1])]
        assert names == [n for n, _ in args._fields_], struct
        assert names[-1] == 'stream' and args._fields_[-1] == ('stream', ctypes.c_void_p)
    assert set(sr.CLUSTER_FIELDS) <= {n for n, _ in _lib.DLClusterArgs._fields_}
    assert set(sr.PICK_FIELDS) <= {n for n, _ in _lib.DLPickArgs._fields_}


def test_struct_sizes_are_the_compilers(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'a C compiler is needed to read include/difflinker_hip.h'
    source, program = os.path.join(tmp_path, 'size.c'), os.path.join(tmp_path, 'size')
    with open(source, 'w') as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "difflinker_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dl_cluster_args), '
                'offsetof(dl_cluster_args, bits), offsetof(dl_cluster_args, num), offsetof(dl_cluster_args, cluster), '
                'offsetof(dl_cluster_args, stream), sizeof(dl_pick_args), offsetof(dl_pick_args, bits), '
                'offsetof(dl_pick_args, first), offsetof(dl_pick_args, stream)); return 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), source, '-o', program], check=True)
    sizes = [int(v) for v in subprocess.run([program], check=True, capture_output=True, text=True).stdout.split()]
    C, P = _lib.DLClusterArgs, _lib.DLPickArgs
    assert sizes == [ctypes.sizeof(C), C.bits.offset, C.num.offset, C.cluster.offset, C.stream.offset,
                     ctypes.sizeof(P), P.bits.offset, P.first.offset, P.stream.offset]
    assert C.stream.offset + 8 == ctypes.sizeof(C) and P.stream.offset + 8 == ctypes.sizeof(P), 'the stream is the last field'


ONE = 16                                         # a pointer that is never dereferenced (and 16-byte aligned)


def cluster_args(**kw):
    fields = dict(M=4, W=64, G=1, num=13, den=20,
                  **{name: ONE for name in ('bits', 'offsets', 'cluster', 'centroid', 'n_neighbours', 'n_clusters', 'status')})
    fields.update(kw)
    return _lib.DLClusterArgs(**fields)


def pick_args(**kw):
    fields = dict(M=4, W=64, G=1, K=2, **{name: ONE for name in ('bits', 'offsets', 'first', 'picks', 'pick_common', 'pick_union',
                                                                'n_picked', 'status', 'pick_rank')})
    fields.update(kw)
    return _lib.DLPickArgs(**fields)


SET_CHECKS = (dict(M=-1), dict(G=-1), dict(W=0), dict(W=8), dict(W=48), dict(W=128), dict(bits=None), dict(offsets=None),
              dict(bits=ONE + 4), dict(bits=ONE + 8))


def test_cluster_argument_checks_come_before_device_work():
    call = _lib.load().dl_tanimoto_cluster
    assert call(None) == BAD_ARG
    for bad in SET_CHECKS + (dict(num=0), dict(num=-1), dict(num=21), dict(den=0), dict(num=65537, den=65537), dict(den=65537),
                             dict(cluster=None), dict(centroid=None), dict(n_neighbours=None), dict(n_clusters=None),
                             dict(status=None)):
        assert call(ctypes.byref(cluster_args(**bad))) == BAD_ARG, bad
    assert call(ctypes.byref(cluster_args(M=0, G=0, bits=None, offsets=None, cluster=None, status=None))) == 0, 'nothing to write'
    assert call(ctypes.byref(cluster_args(M=0, G=0, W=24))) == BAD_ARG, 'the width is checked first'
    assert call(ctypes.byref(cluster_args(M=0, G=0, num=3, den=2))) == BAD_ARG, 'and the threshold'
    assert call(ctypes.byref(cluster_args(M=0, bits=None, cluster=None, n_clusters=None))) == BAD_ARG, 'groups without rows are written'
    assert call(ctypes.byref(cluster_args(G=0, offsets=None, status=None, cluster=None))) == BAD_ARG, 'rows without groups are written'


def test_pick_argument_checks_come_before_device_work():
    call = _lib.load().dl_tanimoto_pick
    assert call(None) == BAD_ARG
    for bad in SET_CHECKS + (dict(K=0), dict(K=-1), dict(K=4097), dict(picks=None), dict(pick_common=None), dict(pick_union=None),
                             dict(n_picked=None), dict(status=None), dict(pick_rank=None)):
        assert call(ctypes.byref(pick_args(**bad))) == BAD_ARG, bad
    assert call(ctypes.byref(pick_args(M=0, G=0, bits=None, offsets=None, first=None, picks=None, pick_rank=None))) == 0
    assert call(ctypes.byref(pick_args(M=0, G=0, K=0))) == BAD_ARG, 'K is checked first'
    assert call(ctypes.byref(pick_args(M=0, bits=None, pick_rank=None, picks=None))) == BAD_ARG
    assert call(ctypes.byref(pick_args(G=0, offsets=None, picks=None, pick_rank=None))) == BAD_ARG


def test_python_layer_refuses_host_tensors_and_bad_parameters():
    bits = torch.zeros(2, 64, dtype=torch.int32)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.tanimoto_clusters(bits)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.tanimoto_picks(bits, 2)
    for k in (0, -3, 4097):
        with pytest.raises(ValueError, match='k must be'):
            metrics.tanimoto_picks(bits, k)
    assert metrics.Clusters._fields == ('cluster', 'centroid', 'n_neighbours', 'n_clusters', 'status', 'num', 'den')
    assert metrics.Picks._fields == ('picks', 'pick_common', 'pick_union', 'n_picked', 'status', 'pick_rank')
    assert inspect.signature(metrics.tanimoto_clusters).parameters['threshold'].default == '0.65'
    assert inspect.signature(metrics.select_records).parameters['view'].default == 'linker'


def test_the_threshold_becomes_a_fraction():
    assert metrics.threshold_fraction('0.65') == (13, 20) == metrics.threshold_fraction(0.65) == metrics.threshold_fraction(Fraction(65, 100))
    assert metrics.threshold_fraction('1') == (1, 1) and metrics.threshold_fraction('0.7') == (7, 10) == metrics.threshold_fraction(0.7)
    assert metrics.threshold_fraction('0.3333') == (1, 3), 'the denominator is limited to 1000'
    assert metrics.threshold_fraction('0.001') == (1, 1000) and metrics.threshold_fraction('2/3') == (2, 3)
    for bad in ('0', '-0.5', '1.01', 0.0001, 2):
        with pytest.raises(ValueError, match='threshold'):
            metrics.threshold_fraction(bad)


# ---- select_records on stubbed device results ------------------------------------------------------------------------------------

def as_words(t):
    return t.numpy().view(np.uint32)


@pytest.fixture
def stubbed(monkeypatch):
    """The three launches of ``select_records`` answered by the plain-Python rules, on host tensors; the calls are kept."""
    calls = []
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32))                      # noqa: E731

    def clusters(bits, offsets=None, threshold='0.65'):
        num, den = metrics.threshold_fraction(threshold)
        got = sr.clusters(as_words(bits), offsets.tolist(), num, den)
        calls.append(('clusters', bits.clone(), offsets.tolist()))
        return metrics.Clusters(*(i32(got[name]) for name in sr.CLUSTER_FIELDS), num, den)

    def picks(bits, k, offsets=None, first=None):
        got = sr.picks(as_words(bits), k, offsets.tolist(), first.tolist())
        calls.append(('picks', bits.clone(), offsets.tolist(), first.tolist(), k))
        return metrics.Picks(*(i32(got[name]) for name in sr.PICK_FIELDS))

    def nearest(a, b, a_offsets=None, b_offsets=None, exclude_diagonal=False, want_sum=True):
        got = fr.tanimoto_nearest(as_words(a), as_words(b), a_offsets.tolist(), b_offsets.tolist(), exclude_diagonal, want_sum)
        return metrics.Nearest(i32(got['nn_index']), i32(got['nn_common']), i32(got['nn_union']),
                               torch.as_tensor(got['sum_q20'].astype(np.int64)), i32(got['n_pairs']))
    monkeypatch.setattr(metrics, 'tanimoto_clusters', clusters)
    monkeypatch.setattr(metrics, 'tanimoto_picks', picks)
    monkeypatch.setattr(metrics, 'tanimoto_nearest', nearest)
    return calls


def prints(bit_sets, status=None):
    bits = torch.as_tensor(rows(*bit_sets, w=64).view(np.int32))
    n = len(bit_sets)
    zeros = torch.zeros(n, dtype=torch.int32)
    return metrics.Fingerprints(bits, zeros, zeros, zeros, zeros if status is None else torch.as_tensor(status, dtype=torch.int32))


A, B = set(range(0, 20)), set(range(100, 120))
NEAR_A = set(range(1, 21))                                               # 19 / 21 to A


def test_select_records_groups_the_eligible_samples_of_every_input(stubbed):
    # sample:   0     1       2    3    4      5 (input 'y')   6 (broken: far from everything)
    linker = [A, NEAR_A, B, A, B, A, {500, 501}]
    whole = prints([{7}] * 7)                                            # the other view: all equal
    inputs = ['x', 'x', 'x', 'y', 'x', 'x', 'x']
    good = [True] * 6 + [False]
    records = metrics.select_records(whole, prints(linker), inputs, good, threshold='0.65', k=2)
    assert [m.input for m in records] == inputs and [m.eligible for m in records] == good
    # input x has samples 0, 1, 2, 4, 5 (sorted rows 0 .. 4), input y sample 3 (row 5)
    kind, bits, offsets = stubbed[0]
    assert kind == 'clusters' and offsets == [0, 5, 6] and bits.shape == (6, 64)
    assert torch.equal(bits, prints([linker[k] for k in (0, 1, 2, 4, 5, 3)]).bits), 'the linker view, sorted by input'
    assert stubbed[1][0] == 'picks' and stubbed[1][3] == [0, 5] and stubbed[1][4] == 2, 'the most typical row of each input first'
    x = [records[k] for k in (0, 1, 2, 4, 5)]
    assert [m.cluster for m in x] == [0, 0, 1, 1, 0] and [m.is_centroid for m in x] == [True, False, True, False, False]
    assert [m.cluster_size for m in x] == [3, 3, 2, 2, 3] and [m.n_neighbours for m in x] == [2, 2, 1, 1, 2]
    assert [m.pick_rank for m in x] == [0, None, 1, None, None] and x[2].pick_similarity == 0.0 and x[0].pick_similarity is None
    assert records[3] == metrics.SelectRecord('y', True, 0, True, 1, 0, 0, None), 'a single sample is its own cluster and pick'
    assert records[6] == metrics.SelectRecord('x', False, None, None, None, None, None, None), 'never clustered, never picked'
    assert metrics.compute_selection(records) == {'selection_molecules': 6, 'clusters_per_input': 1.5,
                                                  'cluster_ratio': (2 / 5 + 1) / 2, 'largest_cluster_share': (3 / 5 + 1) / 2}


def test_an_ineligible_sample_is_never_clustered_or_picked(stubbed):
    """MaxMin would pick the broken outlier second; a status bit in EITHER view or a false ``good`` keeps a sample out."""
    linker = [A, NEAR_A, A, {500, 501}, {600}, {700}]
    for status_whole, status_linker, good in (([0, 0, 0, 4, 0, 0], None, [True] * 4 + [False, True]),
                                              (None, [0, 0, 0, 0, 8, 1], [True, True, True, False, True, True])):
        del stubbed[:]
        whole = prints([{7}] * 6, status_whole)
        records = metrics.select_records(whole, prints(linker, status_linker), [0] * 6, good, threshold='0.65', k=6)
        eligible = [m.eligible for m in records]
        assert eligible == [True, True, True, False, False, (status_linker is None)]
        assert all(stubbed[0][1].shape[0] == sum(eligible) for _ in (0,)), 'the launches never see the others'
        for m in records:
            if not m.eligible:
                assert m[2:] == (None,) * 6
        assert sorted(m.pick_rank for m in records if m.pick_rank is not None) == list(range(sum(eligible)))
    everything = metrics.select_records(prints([{7}] * 6), prints(linker), [0] * 6, [True] * 6, k=2)
    assert [m.pick_rank for m in everything] == [0, None, None, 1, None, None], 'without the gate the outlier is picked'
    assert all(m.cluster is None and m.n_neighbours is None for m in everything), 'no threshold: no clusters'


def test_select_records_views_and_bad_arguments(stubbed):
    whole, linker = prints([A, B, A]), prints([A, A, A])
    by_linker = metrics.select_records(whole, linker, [0] * 3, [True] * 3, threshold='0.65')
    by_whole = metrics.select_records(whole, linker, [0] * 3, [True] * 3, view='whole', threshold='0.65')
    assert [m.cluster for m in by_linker] == [0, 0, 0] and [m.cluster for m in by_whole] == [0, 1, 0]
    assert all(m.pick_rank is None and m.pick_similarity is None for m in by_linker), 'no k: no picks'
    assert len(stubbed) == 2 and all(call[0] == 'clusters' for call in stubbed)
    assert metrics.select_records(prints([]), prints([]), [], [], threshold='0.65', k=3) == []
    with pytest.raises(ValueError, match='view'):
        metrics.select_records(whole, linker, [0] * 3, [True] * 3, view='fragments')
    with pytest.raises(ValueError, match='flags'):
        metrics.select_records(whole, linker, [0] * 3, [True] * 2)
    big = metrics.select_records(whole, linker, [0] * 3, [True] * 3, k=10 ** 6)
    assert stubbed[-1][4] == _lib.DL_SELECT_MAX_ROWS and [m.pick_rank for m in big] == [0, 1, 2]


def test_compute_selection_is_a_mean_over_inputs():
    record = lambda input, cluster, eligible=True: metrics.SelectRecord(input, eligible, cluster, False, None, None, None, None)   # noqa: E731
    records = [record('a', 0), record('a', 0), record('a', 1), record('a', 0), record('b', 0), record('b', 1),
               record('c', None, False), record('d', None)]                  # c: nothing eligible; d: eligible, not clustered
    assert metrics.compute_selection(records) == {'selection_molecules': 7, 'clusters_per_input': 2.0,
                                                  'cluster_ratio': (2 / 4 + 2 / 2) / 2, 'largest_cluster_share': (3 / 4 + 1 / 2) / 2}
    assert metrics.compute_selection([]) == {'selection_molecules': 0, 'clusters_per_input': None, 'cluster_ratio': None,
                                             'largest_cluster_share': None}
    assert tuple(metrics.compute_selection([])) == metrics.SELECTION_NAMES


def test_the_report_names_files():
    R = metrics.SelectRecord
    records = [R(0, True, 1, True, 1, 0, 1, 0.25), R(0, False, None, None, None, None, None, None),
               R(0, True, 0, False, 2, 1, None, None), R(0, True, 0, True, 2, 1, 0, None)]
    names = [['a.sdf'], ['b.sdf'], ['c.sdf'], ['d.xyz', 'd.sdf']]
    report = metrics.selection_report(records, names)
    assert set(report) == {'a.sdf', 'b.sdf', 'c.sdf', 'd.xyz', 'd.sdf', 'picked', 'clusters'}
    assert report['picked'] == ['d.xyz', 'd.sdf', 'a.sdf'] and report['b.sdf']['eligible'] is False
    assert report['clusters'] == [{'centroid': 'd.xyz', 'members': ['c.sdf', 'd.xyz', 'd.sdf']},
                                  {'centroid': 'a.sdf', 'members': ['a.sdf']}]
    assert report['a.sdf'] == records[0]._asdict() and report['a.sdf']['pick_similarity'] == 0.25
    two = metrics.selection_report([R('u', True, 0, True, 1, 0, 0, None), R('v', True, 0, True, 1, 0, 0, None)], [['u/0'], ['v/0']])
    assert two['picked'] == ['u/0', 'v/0'] and [c['centroid'] for c in two['clusters']] == ['u/0', 'v/0']
    with pytest.raises(ValueError):
        metrics.selection_report(records, names[:2])


# ---- the command lines ------------------------------------------------------------------------------------------------------------

def test_command_lines_keep_their_defaults(monkeypatch):
    """Without the new flags ``generate`` and ``sample`` are called exactly as before; with them the keywords appear."""
    from difflinker_amd import generate as gen, sample as smp
    for function in (gen.generate, gen.generate_with_pocket, gen.generate_with_protein, gen._sample_and_save, smp.sample):
        parameters = inspect.signature(function).parameters
        assert parameters['cluster'].default is None and parameters['pick'].default is None
        assert parameters['select_view'].default == 'linker'
    seen = {}
    for name in ('generate', 'generate_with_pocket', 'generate_with_protein'):
        monkeypatch.setattr(gen, name, lambda *a, **k: seen.update(k) or [])
    base = ['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3']
    for more in ([], ['--pocket', 'p.pdb'], ['--protein', 'p.pdb']):
        seen.clear()
        gen.main(base + more)
        assert not {'cluster', 'pick', 'select_view'} & set(seen)
        gen.main(base + more + ['--select_view', 'whole'])
        assert not {'cluster', 'pick', 'select_view'} & set(seen), 'a view alone selects nothing'
        gen.main(base + more + ['--cluster', '0.65'])
        assert (seen['cluster'], seen['pick'], seen['select_view']) == ('0.65', None, 'linker')
        gen.main(base + more + ['--pick', '5', '--select_view', 'whole', '--cluster', '0.7'])
        assert (seen['cluster'], seen['pick'], seen['select_view']) == ('0.7', 5, 'whole')
    with pytest.raises(SystemExit):
        gen.main(base + ['--select_view', 'fragments'])
    with pytest.raises(SystemExit):
        gen.main(base + ['--pick', 'many'])
    seen.clear()
    monkeypatch.setattr(smp, 'sample', lambda *a, **k: seen.update(k) or 'out')
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p'])
    assert not {'cluster', 'pick', 'select_view'} & set(seen)
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p', '--cluster', '0.5', '--pick', '2'])
    assert (seen['cluster'], seen['pick'], seen['select_view']) == ('0.5', 2, 'linker')


def test_bad_selections_are_refused_before_any_work(tmp_path):
    from difflinker_amd import generate as gen, sample as smp
    for bad in (dict(cluster='1.5'), dict(cluster='0'), dict(pick=0), dict(pick=3, select_view='fragments')):
        with pytest.raises(ValueError):
            gen.generate('f.sdf', 'm', str(tmp_path / 'never'), 1, None, '3', **bad)
        with pytest.raises(ValueError):
            gen.generate_with_pocket('f.sdf', 'p.pdb', False, 'm', str(tmp_path / 'never'), 1, None, '3', **bad)
        with pytest.raises(ValueError):
            gen.generate_with_protein('f.sdf', 'p.pdb', False, 'm', str(tmp_path / 'never'), 1, None, '3', **bad)
        with pytest.raises(ValueError):
            smp.sample('c', str(tmp_path / 'never'), 'p', 1, 'cpu', **bad)
    assert not os.path.exists(tmp_path / 'never')
    assert gen._selection_arguments(None, None, 'whole') == {}
    assert gen._selection_arguments('0.65', None, 'linker') == {'cluster': '0.65', 'pick': None, 'select_view': 'linker'}
    assert gen._files_of_samples(['/o/output_1_frag_.sdf', '/o/output_0_frag_.xyz', '/o/output_0_frag_.sdf'], 'frag', 3) == \
        [['output_0_frag_.xyz', 'output_0_frag_.sdf'], ['output_1_frag_.sdf'], []]
