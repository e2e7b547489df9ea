"""Fingerprints without a GPU: the pinned values and invariances of ``tests/fingerprint_ref.py``, its tie to
``mol_keys_ref``, the ABI of ``dl_fingerprints`` and ``dl_tanimoto_nearest`` (struct layout, exports, constants, every argument
check - they all come before any device work) and ``metrics.compute_diversity`` on hand-made records."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fingerprint_ref as fr
import mol_keys_ref
from difflinker_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h


# ---- the reference itself -----------------------------------------------------------------------------------------------------

def test_pinned_fingerprints():
    """Computed on the CPU from the definition in the header: n_bits 2048, radius 2, type index 0 = C."""
    assert fr.on_bits(*fr.BENZENE) == {92, 1852, 2031}
    toluene = fr.on_bits(*fr.TOLUENE)
    assert len(toluene) == 9 and {7, 92, 380, 1098, 1852, 2031} <= toluene
    assert fr.on_bits(*fr.TOLUENE, centres=[0] * 6 + [1]) == {380, 1098, 2031}
    hexane = fr.on_bits(*fr.HEXANE)
    assert len(hexane) == 6 and {1098, 2031} <= hexane
    assert [len(fr.on_bits(*fr.TOLUENE, radius=r, n_bits=512)) for r in range(5)] == [1, 4, 9, 16, 23]
    assert fr.on_bits(*fr.PYRIDINE) != fr.on_bits(*fr.BENZENE)
    assert fr.pack_bits({0, 31, 32, 2047}, 2048) == [0x80000001, 1] + [0] * 61 + [1 << 31]


def random_molecule(rng, n, degree=2.2):
    pairs = set()
    while len(pairs) < min(int(round(degree * n / 2)), n * (n - 1) // 2):
        i, j = (int(v) for v in rng.choice(n, 2, replace=False))
        pairs.add((min(i, j), max(i, j)))
    return [int(t) for t in rng.integers(0, 4, n)], [(i, j, int(rng.integers(1, 4))) for i, j in sorted(pairs)]


def test_the_reference_does_not_depend_on_numbering_or_list_order():
    rng = np.random.default_rng(0)
    for n in (2, 7, 30):
        types, bonds = random_molecule(rng, n)
        keep = [bool(v) for v in rng.random(n) < 0.8]
        centres = [bool(v) for v in rng.random(n) < 0.5]
        want = fr.on_bits(types, bonds, keep, centres, radius=3, n_bits=1024)
        assert want or not any(k and c for k, c in zip(keep, centres))
        perm = rng.permutation(n)                                        # old atom k becomes atom perm[k]
        moved = lambda values: [values[int(np.argwhere(perm == k)[0, 0])] for k in range(n)]      # noqa: E731
        shuffled = [bonds[k] for k in rng.permutation(len(bonds))]
        renumbered = [(int(perm[j]), int(perm[i]), o) if rng.random() < 0.5 else (int(perm[i]), int(perm[j]), o)
                      for i, j, o in shuffled]
        assert fr.on_bits(moved(types), renumbered, moved(keep), moved(centres), radius=3, n_bits=1024) == want


@pytest.mark.parametrize('radius', [1, 2, 3, 4])
def test_the_colours_are_those_of_the_molecule_keys(radius):
    """A molecule of exactly ``radius`` atoms is refined for ``radius`` rounds by ``colours_and_key``: the same colours."""
    rng = np.random.default_rng(radius)
    types = [int(t) for t in rng.integers(0, 3, radius)]
    bonds = [(k, k + 1, int(rng.integers(1, 4))) for k in range(radius - 1)]
    want = mol_keys_ref.colours_and_key(types, bonds)[0]
    assert fr.colours(types, bonds, radius) == want
    assert fr.on_bits(types, bonds, radius=radius, n_bits=2048) >= {c % 2048 for c in want}


def test_the_reference_of_the_similarity():
    a = np.array([[0b1011, 0], [0, 0], [0xFFFFFFFF, 0xFFFFFFFF]], np.uint32)
    b = np.array([[0b0011, 0], [0b1011, 0], [0b1011, 0], [0, 0]], np.uint32)
    got = fr.tanimoto_nearest(a, b)
    assert got['nn_index'].tolist() == [1, 3, 1] and got['nn_common'].tolist() == [3, 0, 3] and got['nn_union'].tolist() == [3, 0, 64]
    assert got['n_pairs'].tolist() == [4, 4, 4]
    assert got['sum_q20'].tolist() == [((2 << 20) // 3) + 2 * (1 << 20), 1 << 20, (2 << 20) // 64 + 2 * ((3 << 20) // 64)]
    alone = fr.tanimoto_nearest(a, a, [0, 2, 2, 3], [0, 2, 3, 9], exclude_diagonal=True, want_sum=False)
    assert alone['nn_index'].tolist() == [1, 0, -1] and alone['n_pairs'].tolist() == [1, 1, 0] and alone['sum_q20'] is None


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_aromatic_rings')
    assert _lib.EXPORTS[at + 1:at + 3] == ('dl_fingerprints', 'dl_tanimoto_nearest') and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_fingerprints(const dl_fingerprint_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert 'int32_t dl_tanimoto_nearest(const dl_tanimoto_args* args);' in header
    opening = header.split('#ifndef DIFFLINKER_HIP_H')[0]
    assert ' *   dl_fingerprints ' in opening and ' *   dl_tanimoto_nearest ' in opening, 'listed in the opening comment'
    assert "NOT RDKit's" in opening and 'What this is NOT: RDKit' in header
    for name, value in (('DL_FP_MAX_ATOMS', 256), ('DL_FP_MAX_RADIUS', 4), ('DL_FP_TOO_LARGE', 4), ('DL_FP_BAD_BOND', 8),
                        ('DL_TANIMOTO_TILE', _lib.DL_TANIMOTO_TILE)):
        assert re.search(rf'#define {name} {value}\s', header) and getattr(_lib, name) == value
    assert (fr.MAX_ATOMS, fr.MAX_RADIUS, fr.TOO_LARGE, fr.BAD_BOND, fr.BONDS_OVERFLOW) == \
        (_lib.DL_FP_MAX_ATOMS, _lib.DL_FP_MAX_RADIUS, _lib.DL_FP_TOO_LARGE, _lib.DL_FP_BAD_BOND, _lib.DL_BONDS_OVERFLOW)
    assert _lib.DL_FP_BITS == (512, 1024, 2048) and _lib.DL_TANIMOTO_TILE >= 64
    lib = _lib.load()
    assert hasattr(lib, 'dl_fingerprints') and hasattr(lib, 'dl_tanimoto_nearest') and lib.dl_abi_version() == 7
    # the structs' fields in the header's order, the stream last
    for struct, args in (('dl_fingerprint_args', _lib.DLFingerprintArgs), ('dl_tanimoto_args', _lib.DLTanimotoArgs)):
        body = header.split('typedef struct %s {' % struct)[1].split('} %s;' % struct)[0]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = [n for line in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', line.strip().split('*')[-1])]
        assert names == [n for n, _ in args._fields_], struct
        assert names[-1] == 'stream' and args._fields_[-1] == ('stream', ctypes.c_void_p)
        assert 'void* stream;                   /* hipStream_t; NULL: the default stream */' in header


def test_struct_sizes_are_the_compilers(tmp_path):
    """``sizeof`` and the offsets of the first pointer and of the last field of both structs, from the C compiler."""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'a C compiler is needed to read include/difflinker_hip.h'
    source, program = os.path.join(tmp_path, 'size.c'), os.path.join(tmp_path, 'size')
    with open(source, 'w') as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "difflinker_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dl_fingerprint_args), '
                'offsetof(dl_fingerprint_args, one_hot), offsetof(dl_fingerprint_args, radius), '
                'offsetof(dl_fingerprint_args, stream), sizeof(dl_tanimoto_args), offsetof(dl_tanimoto_args, a_bits), '
                'offsetof(dl_tanimoto_args, exclude_diagonal), offsetof(dl_tanimoto_args, stream)); return 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), source, '-o', program], check=True)
    sizes = [int(v) for v in subprocess.run([program], check=True, capture_output=True, text=True).stdout.split()]
    F, T = _lib.DLFingerprintArgs, _lib.DLTanimotoArgs
    assert sizes == [ctypes.sizeof(F), F.one_hot.offset, F.radius.offset, F.stream.offset,
                     ctypes.sizeof(T), T.a_bits.offset, T.exclude_diagonal.offset, T.stream.offset]
    assert F.stream.offset + 8 == ctypes.sizeof(F) and T.stream.offset + 8 == ctypes.sizeof(T), 'the stream is the last field'


ONE = 16                                         # a pointer that is never dereferenced (and 16-byte aligned)


def fingerprint_args(**kw):
    fields = dict(B=1, N=8, nf=4, capacity=4, radius=2, n_bits=2048,
                  **{name: ONE for name in ('one_hot', 'node_mask', 'n_bonds_in', 'bonds', 'status_in', 'bits', 'n_on', 'n_atoms',
                                            'n_centres', 'status')})
    fields.update(kw)
    return _lib.DLFingerprintArgs(**fields)


def tanimoto_args(**kw):
    fields = dict(Ma=4, Mb=4, W=64, G=1, **{name: ONE for name in ('a_bits', 'b_bits', 'a_offsets', 'b_offsets', 'nn_index',
                                                                  'nn_common', 'nn_union', 'n_pairs', 'sum_q20')})
    fields.update(kw)
    return _lib.DLTanimotoArgs(**fields)


def test_fingerprint_argument_checks_come_before_device_work():
    call = _lib.load().dl_fingerprints
    assert call(None) == BAD_ARG
    for bad in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(nf=17), dict(capacity=-1), dict(radius=-1), dict(radius=5),
                dict(n_bits=0), dict(n_bits=256), dict(n_bits=2047), dict(n_bits=4096), dict(n_bits=1536)):
        assert call(ctypes.byref(fingerprint_args(**bad))) == BAD_ARG, bad
        assert call(ctypes.byref(fingerprint_args(B=0, **{k: v for k, v in bad.items() if k != 'B'}))) == (0 if 'B' in bad else BAD_ARG)
    for name in ('one_hot', 'node_mask', 'n_bonds_in', 'bonds', 'status_in', 'bits', 'n_on', 'n_atoms', 'n_centres', 'status'):
        assert call(ctypes.byref(fingerprint_args(**{name: None}))) == BAD_ARG, name
    assert call(ctypes.byref(fingerprint_args(B=0, one_hot=None, bits=None))) == 0, 'an empty batch has nothing to point at'


def test_tanimoto_argument_checks_come_before_device_work():
    call = _lib.load().dl_tanimoto_nearest
    assert call(None) == BAD_ARG
    for bad in (dict(Ma=-1), dict(Mb=-1), dict(G=-1), dict(W=0), dict(W=8), dict(W=48), dict(W=128), dict(a_bits=None),
                dict(b_bits=None), dict(a_offsets=None), dict(b_offsets=None), dict(nn_index=None), dict(nn_common=None),
                dict(nn_union=None), dict(n_pairs=None), dict(a_bits=ONE + 4), dict(b_bits=ONE + 8)):
        assert call(ctypes.byref(tanimoto_args(**bad))) == BAD_ARG, bad
    assert call(ctypes.byref(tanimoto_args(Ma=0, a_bits=None, nn_index=None))) == 0, 'no rows: no launch'
    assert call(ctypes.byref(tanimoto_args(Ma=0, W=24))) == BAD_ARG, 'the width is checked first'


def test_python_layer_refuses_host_tensors_and_bad_parameters():
    import torch
    from difflinker_amd.molecule_builder import Bonds
    one_hot, mask = torch.zeros(1, 4, 3), torch.ones(1, 4)
    found = Bonds(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 3, dtype=torch.int32), None, None, None,
                  torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.fingerprints(one_hot, mask, found)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.tanimoto_nearest(torch.zeros(2, 64, dtype=torch.int32), torch.zeros(2, 64, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.analyze_fingerprints(one_hot, torch.zeros(1, 4, 3), mask, False, mask)
    defaults = inspect.signature(metrics.fingerprints).parameters
    assert defaults['radius'].default == 2 and defaults['n_bits'].default == 2048 and defaults['centre_mask'].default is None
    assert metrics.Fingerprints._fields == ('bits', 'n_on', 'n_atoms', 'n_centres', 'status')
    assert metrics.Nearest._fields == ('index', 'common', 'union', 'sum_q20', 'n_pairs')


def test_flags_are_off_by_default():
    from difflinker_amd import generate, sample
    from difflinker_amd.lightning import DDPM
    parameters = inspect.signature(sample.sample).parameters
    assert parameters['diversity'].default is False and parameters['diversity_reference'].default is None
    assert inspect.signature(generate.generate).parameters['diversity'].default is False
    assert 'diversity_metrics = False' in inspect.getsource(DDPM.__init__)


# ---- compute_diversity ----------------------------------------------------------------------------------------------------------

def record(input, status=0, sim=None, pairs=0, sim_linker=None, true=None, true_linker=None, ref=None):
    """A ``DiversityRecord`` by hand: ``sim`` the similarities to the other samples of the input as ``(c, u)`` fractions."""
    q = lambda fractions: sum((c << 20) // u if u else 1 << 20 for c, u in fractions or [])      # noqa: E731
    pair = lambda f: (None, None) if f is None else f                                           # noqa: E731
    return metrics.DiversityRecord(input, status, q(sim), pairs, q(sim if sim_linker is None else sim_linker), pairs,
                                   *pair(true), *pair(true_linker), *pair(ref))


def test_diversity_of_identical_and_of_disjoint_samples():
    same = [record('a', sim=[(9, 9)], pairs=1), record('a', sim=[(9, 9)], pairs=1)]
    got = metrics.compute_diversity(same)
    assert got == {'diversity_molecules': 2, 'internal_diversity': 0.0, 'internal_diversity_linker': 0.0}
    apart = [record('a', sim=[(0, 18), (0, 20)], pairs=2), record('a', sim=[(0, 18), (0, 15)], pairs=2),
             record('a', sim=[(0, 20), (0, 15)], pairs=2)]
    assert metrics.compute_diversity(apart)['internal_diversity'] == 1.0
    empty = [record('a', sim=[(0, 0)], pairs=1), record('a', sim=[(0, 0)], pairs=1)]
    assert metrics.compute_diversity(empty)['internal_diversity'] == 0.0, 'two empty fingerprints are equal'


def test_diversity_is_a_mean_over_inputs_and_leaves_single_samples_out():
    records = [record('a', sim=[(1, 2)], pairs=1, sim_linker=[(1, 4)]), record('a', sim=[(1, 2)], pairs=1, sim_linker=[(1, 4)]),
               record('b', sim=[(9, 9)], pairs=1), record('b', sim=[(9, 9)], pairs=1),
               record('c')]                                                # one sample: no pair, no part in the mean
    got = metrics.compute_diversity(records)
    assert got['diversity_molecules'] == 5
    assert got['internal_diversity'] == (0.5 + 0.0) / 2 and got['internal_diversity_linker'] == (0.75 + 0.0) / 2
    assert metrics.compute_diversity([record('c')]) == {'diversity_molecules': 1, 'internal_diversity': None,
                                                       'internal_diversity_linker': None}
    assert metrics.compute_diversity([])['diversity_molecules'] == 0


def test_a_flagged_molecule_is_not_scored():
    records = [record('a', sim=[(1, 2)], pairs=1, true=(1, 4), true_linker=(0, 0), ref=(3, 3)),
               record('a', sim=[(1, 2)], pairs=1, true=(3, 4), true_linker=(1, 2), ref=(1, 2)),
               record('a', status=_lib.DL_FP_TOO_LARGE, sim=[(9, 9), (9, 9)], pairs=2, true=(9, 9), true_linker=(9, 9), ref=(9, 9)),
               record('b', status=_lib.DL_BONDS_OVERFLOW)]
    got = metrics.compute_diversity(records)
    assert got == {'diversity_molecules': 2, 'internal_diversity': 0.5, 'internal_diversity_linker': 0.5,
                   'similarity_to_true': 0.5, 'similarity_to_true_linker': 0.75,
                   'nearest_reference_similarity': 0.75, 'nearest_reference_identical': 0.5}
    assert set(got) == set(metrics.DIVERSITY_NAMES + metrics.DIVERSITY_TRUE_NAMES + metrics.DIVERSITY_REFERENCE_NAMES)
    # the keys that are asked for are there even when nothing carries them; those that are not asked for are not
    bare = metrics.compute_diversity([record('a')], with_true=True, with_reference=True)
    assert bare['similarity_to_true'] is None and bare['nearest_reference_identical'] is None
    assert set(metrics.compute_diversity(records, with_true=False, with_reference=False)) == set(metrics.DIVERSITY_NAMES)
