"""Pharmacophore features without a GPU: ``tests/pharmacophore_ref.py`` on hand-built molecules whose features are worked out
by hand, the ABI of ``dl_pharmacophore_features`` and ``dl_feature_match`` (struct layout, exports, constants, every argument
check - they all come before any device work), ``metrics.compute_pharmacophores`` on hand-made records and the flags' defaults.
The rule is this project's own, after RDKit's ``BaseFeatures.fdef``: nothing here is compared with RDKit."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pharmacophore_ref as pr
from difflinker_amd import _lib, const, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


# ---- the reference itself -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(pr.EXAMPLES))
def test_hand_built_molecules(name):
    """Families, anchors and the list's order: atom features by (atom, family), then the rings in order, Aromatic before
    LumpedHydrophobe."""
    symbols, bonds, want = pr.EXAMPLES[name]
    arrays = pr.as_batch([(symbols, bonds)])
    got = pr.batch_features(arrays, Fcap=32)
    n = int(got['n_features'][0])
    assert list(zip(got['family'][0, :n].tolist(), got['anchor'][0, :n].tolist())) == want
    assert got['status'][0] == 0 and (got['family'][0, n:] == -1).all() and (got['anchor'][0, n:] == -1).all()
    assert got['family_count'][0].tolist() == [sum(f == k for f, _ in want) for k in range(pr.FAMILIES)]
    for f in range(n):                                                      # positions: the atom's own, or the ring's centroid
        if got['family'][0, f] < pr.AROMATIC:
            assert np.array_equal(got['position'][0, f], arrays['x'][0, got['anchor'][0, f]])


def test_the_stated_features_of_the_examples():
    """The sentences of the rule, one by one."""
    at = lambda name, atom: {f for f, a in pr.EXAMPLES[name][2] if a == atom and f < pr.AROMATIC}      # noqa: E731
    rings = lambda name: [f for f, _ in pr.EXAMPLES[name][2] if f >= pr.AROMATIC]                      # noqa: E731
    assert at('acetic acid', 1) == {pr.NEGATIVE} and at('acetic acid', 3) == {pr.DONOR, pr.ACCEPTOR}
    assert at('acetate', 1) == {pr.NEGATIVE}, 'a carboxylate read as two C=O'
    assert not any(f == pr.NEGATIVE for f, _ in pr.EXAMPLES['dimethyl sulfone'][2])
    assert at('methanesulfonate', 1) == {pr.NEGATIVE}
    assert at('trimethylamine', 0) == {pr.ACCEPTOR, pr.POSITIVE}
    assert at('dimethylacetamide', 3) == set()
    assert at('aniline', 6) == {pr.DONOR}
    assert at('pyridine', 0) == {pr.ACCEPTOR} and at('pyrrole', 0) == {pr.DONOR} and at('furan', 0) == set()
    assert rings('pyridine') == rings('pyrrole') == rings('furan') == [pr.AROMATIC]
    assert rings('benzene') == [pr.AROMATIC, pr.LUMPED] and sum(f == pr.HYDROPHOBE for f, _ in pr.EXAMPLES['benzene'][2]) == 6
    assert at('chlorobenzene', 6) == {pr.HYDROPHOBE} and at('chlorobenzene', 0) == set()
    assert at('acetamidine', 1) == {pr.POSITIVE}
    assert rings('naphthalene') == [pr.AROMATIC, pr.LUMPED] * 2


def test_the_centroid_is_fp64_in_canonical_order_rounded_once():
    symbols, bonds, _ = pr.EXAMPLES['benzene']
    arrays = pr.as_batch([(symbols, bonds)], seed=3)
    got = pr.batch_features(arrays, Fcap=8)
    x = arrays['x'][0].astype(np.float64)
    want = (((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]) / 6.0
    assert got['family'][0].tolist() == [pr.HYDROPHOBE] * 6 + [pr.AROMATIC, pr.LUMPED]
    assert np.array_equal(got['position'][0, 6], want.astype(np.float32)) and np.array_equal(got['position'][0, 7], got['position'][0, 6])


def test_list_order_limits_and_flags():
    symbols, bonds, want = pr.EXAMPLES['naphthalene']
    arrays = pr.as_batch([(symbols, bonds)])
    full = pr.batch_features(arrays, Fcap=len(want))
    assert full['status'][0] == 0 and full['n_features'][0] == len(want)
    short = pr.batch_features(arrays, Fcap=len(want) - 1)
    assert short['status'][0] == pr.OVERFLOW and short['n_features'][0] == len(want)
    assert np.array_equal(short['family'][0], full['family'][0, :-1]) and short['family_count'][0].tolist() == full['family_count'][0].tolist()
    # a permuted, re-oriented list says the same
    rng = np.random.default_rng(1)
    order = rng.permutation(len(bonds))
    arrays2 = pr.as_batch([(symbols, [(bonds[k][1], bonds[k][0]) + bonds[k][2:] for k in order])])
    arrays2['x'] = arrays['x']
    again = pr.batch_features(arrays2, Fcap=len(want))
    assert all(np.array_equal(again[k], full[k]) for k in pr.FIELDS)
    # marks: an atom feature by its anchor, a ring feature when every atom of the ring is marked
    mark = np.zeros((1, 10), np.float32)
    mark[0, [4, 5, 6, 7, 8, 9]] = 1
    marked = pr.batch_features(arrays, Fcap=len(want), mark_mask=mark)
    assert marked['marked'][0].tolist() == [0] * 4 + [1] * 6 + [0, 0, 1, 1]
    # dropping an atom of the first ring leaves the second
    drop = np.zeros((1, 10), np.float32)
    drop[0, 1] = 1
    dropped = pr.batch_features(arrays, Fcap=len(want), drop_mask=drop)
    n = int(dropped['n_features'][0])
    assert dropped['family'][0, n - 2:n].tolist() == [pr.AROMATIC, pr.LUMPED] and dropped['anchor'][0, n - 1] == 4
    assert 1 not in dropped['anchor'][0, :n].tolist()
    # bad and repeated entries: the first entry of a pair decides
    twice = pr.as_batch([(symbols[:2], [(0, 1, 1, 0), (1, 0, 2, 1), (0, 0, 1, 0), (0, 5, 1, 0)])])
    got = pr.batch_features(twice, Fcap=4)
    assert got['status'][0] == pr.BAD_BOND and got['family'][0].tolist() == [pr.HYDROPHOBE, pr.HYDROPHOBE, -1, -1]


def test_the_reference_of_the_match():
    fam_a = np.array([[pr.DONOR, pr.DONOR, pr.ACCEPTOR, 9]], np.int32)
    pos_a = np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]], np.float32)
    fam_b = np.array([[pr.DONOR, pr.ACCEPTOR, pr.HYDROPHOBE]], np.int32)
    pos_b = np.array([[[1.5, 2, 0], [1, 0, 1], [0, 0, 0]]], np.float32)
    ones = lambda t: np.ones_like(t)      # noqa: E731
    got = pr.feature_match(fam_a, pos_a, ones(fam_a), [4], fam_b, pos_b, ones(fam_b), [3], 6.25)
    assert got['best_index'].tolist() == [[-1, 2, -1]], 'd2 == 6.25 exactly is no match'
    assert got['best_d2'].tolist() == [[math.inf, 1.0, math.inf]] and (got['n_a'][0], got['n_b'][0], got['n_matched'][0]) == (3, 3, 1)
    nearer = pr.feature_match(fam_a, pos_a, ones(fam_a), [4], fam_b, pos_b, ones(fam_b), [3], np.nextafter(np.float32(6.25), np.float32(7)))
    assert nearer['best_index'].tolist() == [[0, 2, -1]], 'an exact tie goes to the lower index'
    assert pr.feature_score([math.inf, 1.0, math.inf], 3, 3) == math.exp(-1.0) / 3 and pr.feature_score([], 0, 3) is None


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_tanimoto_nearest')
    assert _lib.EXPORTS[at + 1:at + 4] == ('dl_pharmacophore_features', 'dl_feature_match', 'dl_best_rmsd')
    assert _lib.EXPORTS[-1] == 'dl_best_rmsd'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_pharmacophore_features(const dl_pharm_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert 'int32_t dl_feature_match(const dl_feature_match_args* args);' in header
    opening = header.split('#ifndef DIFFLINKER_HIP_H')[0]
    assert ' *   dl_pharmacophore_features ' in opening and ' *   dl_feature_match ' in opening, 'listed in the opening comment'
    block = header.split('pharmacophore features and their feature-map match (pharmacophore.hip)')[1]
    block = ' '.join(block.split('typedef struct dl_pharm_args')[0].replace('\n *', ' ').split())
    assert "THE RULE BELOW IS THIS PROJECT'S OWN" in block and "NOT RDKit's feature factory" in block
    assert "these are NOT RDKit's numbers" in block and 'BaseFeatures.fdef' in block and 'FeatMapParams' in block
    assert 'ZnBinder' in block and 'Limits of the rule' in block
    for name, value in (('DL_PHARM_MAX_ATOMS', 256), ('DL_PHARM_MAX_RINGS', 64), ('DL_PHARM_FAMILIES', 7), ('DL_PHARM_TOO_LARGE', 4),
                        ('DL_PHARM_BAD_BOND', 8), ('DL_PHARM_MANY_RINGS', 16), ('DL_PHARM_OVERFLOW', 32), ('DL_PHARM_NONFINITE', 64)):
        assert re.search(rf'#define {name} {value}\s', header) and getattr(_lib, name) == value
    assert (_lib.DL_PHARM_TOO_LARGE, _lib.DL_PHARM_BAD_BOND) == (_lib.DL_AROM_TOO_LARGE, _lib.DL_AROM_BAD_BOND)
    assert (pr.MAX_ATOMS, pr.MAX_RINGS, pr.FAMILIES, pr.BONDS_OVERFLOW, pr.TOO_LARGE, pr.BAD_BOND, pr.MANY_RINGS, pr.OVERFLOW,
            pr.NONFINITE) == (_lib.DL_PHARM_MAX_ATOMS, _lib.DL_PHARM_MAX_RINGS, _lib.DL_PHARM_FAMILIES, _lib.DL_BONDS_OVERFLOW,
                              _lib.DL_PHARM_TOO_LARGE, _lib.DL_PHARM_BAD_BOND, _lib.DL_PHARM_MANY_RINGS, _lib.DL_PHARM_OVERFLOW,
                              _lib.DL_PHARM_NONFINITE)
    lib = _lib.load()
    assert hasattr(lib, 'dl_pharmacophore_features') and hasattr(lib, 'dl_feature_match') and lib.dl_abi_version() == 7
    for struct, args in (('dl_pharm_args', _lib.DLPharmArgs), ('dl_feature_match_args', _lib.DLFeatureMatchArgs)):
        body = header.split('typedef struct %s {' % struct)[1].split('} %s;' % struct)[0]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = [n for line in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', line.strip().split('*')[-1])]
        assert names == [n for n, _ in args._fields_], struct
        assert names[-1] == 'stream' and args._fields_[-1] == ('stream', ctypes.c_void_p)


def test_the_tables_of_const():
    for is_geom, n in ((False, 8), (True, 9)):
        assert const.feature_class_table(is_geom).tolist() == list(pr.FEATURE_CLASS[:n])
        assert const.default_valence_table(is_geom).tolist() == list(pr.DEFAULT_VALENCE[:n])
    assert const.DEFAULT_VALENCE == {'C': 4, 'N': 3, 'O': 2, 'F': 1, 'S': 2, 'Cl': 1, 'Br': 1, 'I': 1, 'P': 3}
    assert [const.GEOM_ATOM2IDX[s] for s in pr.TYPE] == list(pr.TYPE.values())


def test_struct_sizes_are_the_compilers(tmp_path):
    """``sizeof`` and field offsets of both structs from the C compiler."""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'a C compiler is needed to read include/difflinker_hip.h'
    source, program = os.path.join(tmp_path, 'size.c'), os.path.join(tmp_path, 'size')
    P, M = _lib.DLPharmArgs, _lib.DLFeatureMatchArgs
    fields = [('dl_pharm_args', P, n) for n, _ in P._fields_] + [('dl_feature_match_args', M, n) for n, _ in M._fields_]
    with open(source, 'w') as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "difflinker_hip.h"\nint main(void) {\n'
                'printf("%zu %zu\\n", sizeof(dl_pharm_args), sizeof(dl_feature_match_args));\n'
                + ''.join(f'printf("%zu\\n", offsetof({struct}, {name}));\n' for struct, _, name in fields)
                + 'return 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), source, '-o', program], check=True)
    sizes = [int(v) for v in subprocess.run([program], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes[:2] == [ctypes.sizeof(P), ctypes.sizeof(M)]
    assert sizes[2:] == [getattr(cls, name).offset for _, cls, name in fields]
    assert P.stream.offset + 8 == ctypes.sizeof(P) and M.stream.offset + 8 == ctypes.sizeof(M), 'the stream is the last field'


ONE = 16                                         # a pointer that is never dereferenced


def pharm_args(**kw):
    fields = dict(B=1, N=8, nf=9, capacity=4, Fcap=8,
                  **{name: ONE for name, kind in _lib.DLPharmArgs._fields_ if kind is ctypes.c_void_p and name != 'stream'})
    fields.update(kw)
    return _lib.DLPharmArgs(**fields)


def match_args(**kw):
    fields = dict(B=1, Fa=4, Fb=4, radius2=6.25,
                  **{name: ONE for name, kind in _lib.DLFeatureMatchArgs._fields_ if kind is ctypes.c_void_p and name != 'stream'})
    fields.update(kw)
    return _lib.DLFeatureMatchArgs(**fields)


def test_feature_argument_checks_come_before_device_work():
    call = _lib.load().dl_pharmacophore_features
    assert call(None) == BAD_ARG
    for bad in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1), dict(Fcap=-1)):
        assert call(ctypes.byref(pharm_args(**bad))) == BAD_ARG, bad
        assert call(ctypes.byref(pharm_args(B=0, **{k: v for k, v in bad.items() if k != 'B'}))) == (0 if 'B' in bad else BAD_ARG)
    optional = ('drop_mask', 'mark_mask', 'stream')
    for name, kind in _lib.DLPharmArgs._fields_:
        if kind is ctypes.c_void_p and name not in optional:
            assert call(ctypes.byref(pharm_args(**{name: None}))) == BAD_ARG, name
    assert call(ctypes.byref(pharm_args(B=0, one_hot=None, family=None))) == 0, 'an empty batch has nothing to point at'


def test_match_argument_checks_come_before_device_work():
    call = _lib.load().dl_feature_match
    assert call(None) == BAD_ARG
    for bad in (dict(B=-1), dict(Fa=-1), dict(Fb=-1), dict(radius2=-1.0), dict(radius2=math.nan)):
        assert call(ctypes.byref(match_args(**bad))) == BAD_ARG, bad
        assert call(ctypes.byref(match_args(B=0, **{k: v for k, v in bad.items() if k != 'B'}))) == (0 if 'B' in bad else BAD_ARG)
    for name, kind in _lib.DLFeatureMatchArgs._fields_:
        if kind is ctypes.c_void_p and name != 'stream':
            assert call(ctypes.byref(match_args(**{name: None}))) == BAD_ARG, name
    assert call(ctypes.byref(match_args(B=0, family_a=None, best_d2=None))) == 0


def test_python_layer_refuses_host_tensors_and_bad_parameters():
    import torch
    from difflinker_amd.molecule_builder import Bonds
    one_hot, x, mask = torch.zeros(1, 4, 9), torch.zeros(1, 4, 3), torch.ones(1, 4)
    found = Bonds(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 3, dtype=torch.int32), None, None, None,
                  torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.pharmacophore_features(one_hot, x, mask, found, torch.zeros(1, 2, dtype=torch.int32), True)
    empty = metrics.Features(torch.zeros(1, 2, dtype=torch.int32), None, torch.zeros(1, 2, 3), torch.zeros(1, 2, dtype=torch.int32),
                             torch.zeros(1, dtype=torch.int32), None, None)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.feature_match(empty, empty)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.analyze_pharmacophores(one_hot, x, mask, mask, one_hot, x, mask, mask)
    assert list(inspect.signature(metrics.pharmacophore_features).parameters) == [
        'one_hot', 'x', 'node_mask', 'found', 'bond_aromatic', 'is_geom', 'drop_mask', 'mark_mask', 'capacity']
    match = inspect.signature(metrics.feature_match).parameters
    assert list(match) == ['a', 'b', 'radius', 'marked_only'] and match['radius'].default == 2.5 and match['marked_only'].default is False
    analyze = inspect.signature(metrics.analyze_pharmacophores).parameters
    assert list(analyze)[:9] == ['one_hot_a', 'x_a', 'mask_a', 'linker_a', 'one_hot_b', 'x_b', 'mask_b', 'linker_b', 'is_geom']
    assert analyze['is_geom'].default is True
    assert metrics.Features._fields == ('family', 'anchor', 'position', 'marked', 'n_features', 'family_count', 'status')
    assert metrics.FeatureMatch._fields == pr.MATCH_FIELDS
    for function in (metrics.pharmacophore_features, metrics.feature_match, metrics.analyze_pharmacophores, metrics.compute_pharmacophores):
        assert "NOT RDKit's" in function.__doc__, function.__name__


def test_flags_are_off_by_default():
    from difflinker_amd import sample, train
    from difflinker_amd.lightning import DDPM
    assert inspect.signature(sample.sample).parameters['pharmacophore'].default is False
    assert 'pharmacophore_metrics = False' in inspect.getsource(DDPM.__init__)
    assert "'--pharmacophore', action='store_true'" in inspect.getsource(sample.main)
    assert "'--pharmacophore', action='store_true'" in inspect.getsource(train.main)


# ---- the scores ---------------------------------------------------------------------------------------------------------------

def test_the_score_is_the_gaussian_sum_over_the_smaller_list():
    d2 = [0.0, math.inf, 0.25, 6.0]
    assert metrics.feature_score(d2, 5, 4) == (math.exp(-0.0) + math.exp(-0.25) + math.exp(-6.0)) / 4
    assert metrics.feature_score(d2, 3, 4) == (math.exp(-0.0) + math.exp(-0.25) + math.exp(-6.0)) / 3
    assert metrics.feature_score([math.inf], 2, 1) == 0.0
    assert metrics.feature_score([], 0, 0) is None and metrics.feature_score([math.inf], 0, 1) is None
    assert metrics.feature_score(d2, 5, 4) == pr.feature_score(d2, 5, 4)


def record(score, status=0, n_a=2, n_b=2):
    return metrics.PharmRecord(n_a, n_b, 0 if not score else 1, score, status)


def shape(vol_a, vol_min, status=0):
    return metrics.ShapeRecord(vol_a, vol_a, vol_min, 0, 0, 0, 1, 1, status)


def test_compute_pharmacophores_keys_and_values():
    records = [record(1.0), record(0.5), record(0.9, status=_lib.DL_PHARM_OVERFLOW), record(None, n_a=0),
               record(0.25, status=_lib.DL_BONDS_NONFINITE)]
    linker = [record(0.5), record(None, n_b=0), record(1.0, status=_lib.DL_PHARM_OVERFLOW), record(0.0), record(1.0)]
    got = metrics.compute_pharmacophores(records, linker)
    assert tuple(got) == metrics.PHARM_NAMES == ('feature_molecules', 'feature_flagged', 'feature_similarity',
                                                 'feature_similarity_linker')
    assert got == {'feature_molecules': 3, 'feature_flagged': 1, 'feature_similarity': (1.0 + 0.5 + 0.25) / 3,
                   'feature_similarity_linker': (0.5 + 0.0 + 1.0) / 3}
    assert metrics.compute_pharmacophores(records)['feature_similarity_linker'] is None
    shapes = [shape(10, 7), shape(10, 10, status=1), shape(10, 5), shape(10, 5), shape(4, 4)]
    both = metrics.compute_pharmacophores(records, linker, shapes)
    assert tuple(both) == metrics.PHARM_NAMES + metrics.PHARM_SC_NAMES
    sc = [0.5 * 1.0 + 0.5 * (7 / 10), 0.5 * 0.25 + 0.5 * (4 / 4)]          # the pairs that both scored
    assert both['sc_similarity'] == sum(sc) / 2
    assert (both['sc_similarity_7'], both['sc_similarity_8'], both['sc_similarity_9']) == (50.0, 50.0, 0.0)
    nothing = metrics.compute_pharmacophores([], [], [])
    assert nothing == {'feature_molecules': 0, 'feature_flagged': 0, 'feature_similarity': None, 'feature_similarity_linker': None,
                       'sc_similarity': None, 'sc_similarity_7': None, 'sc_similarity_8': None, 'sc_similarity_9': None}
    with pytest.raises(ValueError, match='shape records'):
        metrics.compute_pharmacophores(records, linker, shapes[:2])
    assert 'inflated' in metrics.compute_pharmacophores.__doc__ and 'linker' in metrics.compute_pharmacophores.__doc__
