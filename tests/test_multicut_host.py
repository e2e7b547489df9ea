"""Cuts at three to five bonds without a GPU: the plain-Python rule of ``tests/multicut_ref.py`` on molecules whose answer is
known by hand, ``fragment.multi_examples`` on a made-up result, the command line of ``prepare``, and the argument checks of
``dl_fragment_multicuts``, which come before any device work."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import fragment_ref
import multicut_ref
from difflinker_amd import _lib, const, prepare
from difflinker_amd.datasets import collate
from difflinker_amd.fragment import MULTI_ANCHOR, MULTI_E, MULTI_EXIT, MULTI_N_FRAG, MultiCuts, multi_all, multi_cuts, multi_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h
OFF = multicut_ref.GATES_OFF
SMALL = {'min_linker': 1, 'min_fragment': 1}


def test_hand_counts():
    """Three tails of five carbons on one carbon: a 3-star takes one bond of every tail, 5 * 5 * 5 ways; the fragments are the
    ends of the tails, a..c atoms, the linker the rest.  With at least three atoms in each: a, b, c in 3..5 and
    16 - a - b - c >= 3, which leaves 23 of the 27."""
    got = multicut_ref.hand('star', R=130, **SMALL)
    assert got['n_cuts_k'] == [125, 0, 0] and got['n_cuts'] == 125 and got['status'] == 0 and got['n_cuttable'] == 15
    got = multicut_ref.hand('star', R=30, min_linker=3, min_fragment=3)
    assert got['n_cuts_k'] == [23, 0, 0] == [sum(16 - a - b - c >= 3 for a in (3, 4, 5) for b in (3, 4, 5) for c in (3, 4, 5)), 0, 0]
    first = got['cuts'][0]                       # the entries 0, 5 and 12: the bonds 0-1 and 0-6 at the centre, 12-13 in the third tail
    assert first == [3, 3, 0, 5, 12, -1, -1, 1, 6, 13, -1, -1, 0, 0, 12, -1, -1, 5, 5, 3, -1, -1]
    assert got['labels'][0] == [5] + [0] * 5 + [1] * 5 + [5, 5, 2, 2, 2]
    assert got['cuts'][23] == [0] * 22 and got['labels'][23] == [255] * 16
    for name in fragment_ref.HAND:
        if name.startswith('chain'):
            assert multicut_ref.hand(name, **SMALL)['n_cuts_k'] == [0, 0, 0], 'the middle one of three bonds on a path lies between the others'
    # a ring linker: fragments beyond 4-5, 9-10 and 7-11 around the five-ring
    got = multicut_ref.hand('ring_linker', R=30, **SMALL)
    assert got['n_cuts_k'] == [25, 0, 0], 'one of five bonds on either chain, and the branch atom'


@pytest.mark.parametrize('m', [2, 3, 5, 7])
def test_a_centre_with_one_atom_arms(m):
    got = multicut_ref.of_types(*multicut_ref.arms(m), 200, **OFF, **SMALL)
    assert got['n_cuts_k'] == [math.comb(m, k) for k in (3, 4, 5)] and got['n_cuts'] == sum(math.comb(m, k) for k in (3, 4, 5))
    for rec, row in zip(got['cuts'][:got['n_cuts']], got['labels']):
        k = rec[0]
        chosen = rec[MULTI_E:MULTI_E + k]
        assert rec[1] == m + 1 - k and rec[MULTI_ANCHOR:MULTI_ANCHOR + k] == [1 + c for c in chosen]
        assert rec[MULTI_EXIT:MULTI_EXIT + k] == [0] * k and rec[MULTI_N_FRAG:MULTI_N_FRAG + k] == [1] * k
        assert all(rec[at + k:at + 5] == [-1] * (5 - k) for at in (MULTI_E, MULTI_ANCHOR, MULTI_EXIT, MULTI_N_FRAG))
        assert [row[1 + c] for c in chosen] == list(range(k)) and row.count(5) == m + 1 - k
    ks = [rec[0] for rec in got['cuts'][:got['n_cuts']]]
    assert ks == sorted(ks), 'k ascending'
    es = [tuple(rec[MULTI_E:MULTI_E + rec[0]]) for rec in got['cuts'][:got['n_cuts']]]
    assert all(a < b for a, b in zip(es, es[1:]) if len(a) == len(b)), 'lexicographic within a k'
    only = multicut_ref.of_types(*multicut_ref.arms(m), 2, min_cuts=4, max_cuts=4, **OFF, **SMALL)
    assert only['n_cuts_k'] == [0, math.comb(m, 4), 0] and (only['status'] == multicut_ref.TRUNCATED) == (math.comb(m, 4) > 2)


def test_gates():
    types, entries = multicut_ref.arms(5)
    rings = entries + [(1, 2, 1), (3, 4, 1)]                            # two three-rings: arms 1..4 are no longer cuttable
    assert multicut_ref.of_types(types, entries, 4, **SMALL)['n_cuts'] == 0, 'no ring: behind the default gate'
    assert multicut_ref.of_types(types, entries, 4, **SMALL)['status'] == 0, 'and a gate sets no bit'
    assert multicut_ref.of_types(types, entries, 4, min_rings=0, **SMALL)['n_cuts'] == 16
    assert multicut_ref.of_types(types, entries, 4, min_rings=0, max_atoms=6, **SMALL)['n_cuts'] == 16
    gated = multicut_ref.of_types(types, entries, 4, min_rings=0, max_atoms=5, **SMALL)
    assert (gated['n_cuts'], gated['status'], gated['n_cuttable'], gated['n_atoms']) == (0, 0, 5, 6)
    three = multicut_ref.arms(3, 2)
    tri = (three[0] + [0, 0, 0, 0], three[1] + [(0, 7, 1), (7, 8, 1), (8, 0, 1), (0, 9, 1), (9, 10, 1), (10, 0, 1)])
    assert multicut_ref.of_types(*tri, 4, min_rings=2, **SMALL)['n_cuts_k'] == [8, 0, 0]
    assert multicut_ref.of_types(*tri, 4, min_rings=3, **SMALL)['n_cuts_k'] == [0, 0, 0]
    assert multicut_ref.of_types(types, rings, 4, min_rings=2, **SMALL)['n_cuttable'] == 1


def test_the_64_bond_boundary():
    rule = dict(OFF, min_cuts=3, max_cuts=3, **SMALL)
    got = multicut_ref.of_types(*multicut_ref.arms(64), 2, **rule)
    assert got['n_cuts_k'] == [math.comb(64, 3), 0, 0] and got['status'] == multicut_ref.TRUNCATED and got['n_cuttable'] == 64
    assert got['cuts'][1][:5] == [3, 62, 0, 1, 3]
    got = multicut_ref.of_types(*multicut_ref.arms(65), 2, **rule)
    assert (got['n_cuts'], got['n_cuttable'], got['status']) == (0, 65, multicut_ref.MANY_CUTTABLE)
    assert got['cuts'] == [[0] * 22] * 2 and got['labels'] == [[255] * 66] * 2
    gated = multicut_ref.of_types(*multicut_ref.arms(65), 2, **dict(rule, max_atoms=65))
    assert (gated['n_cuts'], gated['n_cuttable'], gated['status']) == (0, 65, 0), 'behind a gate: no bit at all'
    big = multicut_ref.molecule([1.0] * 257, [[1.0]] * 257, [(k, k + 1, 1) for k in range(256)], 256, 1, status_in=2, **rule)
    assert big['status'] == 2 | multicut_ref.TOO_LARGE and (big['n_cuttable'], big['n_cuts']) == (0, 0)


def test_batch_helper_shapes():
    types, entries = multicut_ref.arms(4)
    one_hot = np.zeros((2, 6, 3), np.float32)
    one_hot[:, :, 0] = 1
    mask = np.ones((2, 6), np.float32)
    mask[:, 5] = 0
    got = multicut_ref.multicuts(mask, one_hot, np.array([entries, entries]), [4, 3], 6, **OFF, **SMALL)
    assert got['n_cuts'].tolist() == [5, 0] and got['n_cuts_k'].tolist() == [[4, 1, 0], [0, 0, 0]]
    assert got['cuts'].shape == (2, 6, 22) and got['labels'].shape == (2, 6, 6) and got['labels'].dtype == np.uint8
    assert all(got[k].dtype == np.int32 for k in multicut_ref.FIELDS if k != 'labels')
    assert got['status'].tolist() == [0, multicut_ref.DISCONNECTED], 'the last entry left out: atom 4 is on its own'
    assert got['labels'][0, 4].tolist() == [5, 0, 1, 2, 3, 255]


def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_pocket_select')
    assert _lib.EXPORTS[at + 1] == 'dl_fragment_multicuts' and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_fragment_multicuts(const dl_fragment_multi_args* args, void* stream);' in header
    for name, value in (('DL_FRAG_MULTI_FIELDS', 22), ('DL_FRAG_MULTI_MIN_CUTS', 3), ('DL_FRAG_MULTI_MAX_CUTS', 5),
                        ('DL_FRAG_MULTI_MAX_CUTTABLE', 64), ('DL_FRAG_MULTI_LINKER', 5), ('DL_FRAG_MANY_CUTTABLE', 64)):
        assert re.search(rf'#define {name} {value}\s', header) and getattr(_lib, name) == value
    assert (multicut_ref.FIELDS_PER_CUT, multicut_ref.MIN_CUTS, multicut_ref.MAX_CUTS, multicut_ref.MAX_CUTTABLE, multicut_ref.LINKER,
            multicut_ref.MANY_CUTTABLE) == (_lib.DL_FRAG_MULTI_FIELDS, _lib.DL_FRAG_MULTI_MIN_CUTS, _lib.DL_FRAG_MULTI_MAX_CUTS,
                                            _lib.DL_FRAG_MULTI_MAX_CUTTABLE, _lib.DL_FRAG_MULTI_LINKER, _lib.DL_FRAG_MANY_CUTTABLE)
    lib = _lib.load()
    assert lib.dl_abi_version() == 7 and hasattr(lib, 'dl_fragment_multicuts')
    # the ctypes struct against the header's field list, names and kinds in order
    body = header[header.index('typedef struct dl_fragment_multi_args {'):header.index('} dl_fragment_multi_args;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S).split('{', 1)[1]
    declared = []
    for statement in body.split(';'):
        statement = statement.strip()
        if statement:
            pointer = '*' in statement
            for name in statement.replace('*', ' ').split(',') if not pointer else [statement.replace('*', ' ')]:
                declared.append((name.split()[-1], ctypes.c_void_p if pointer else ctypes.c_int32))
    assert declared == list(_lib.DLFragmentMultiArgs._fields_)
    assert MultiCuts._fields == multicut_ref.FIELDS and (MULTI_E, MULTI_ANCHOR, MULTI_EXIT, MULTI_N_FRAG) == (2, 7, 12, 17)


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    fine = dict(N=40, nf=8, capacity=8, R=4, min_cuts=3, max_cuts=5)
    call = lambda **kw: int(lib.dl_fragment_multicuts(ctypes.byref(_lib.DLFragmentMultiArgs(**dict(fine, **kw))), None))  # noqa: E731
    assert int(lib.dl_fragment_multicuts(None, None)) == BAD_ARG
    assert call(B=2) == BAD_ARG                                         # null pointers
    assert call(B=2, capacity=0, R=0) == BAD_ARG                        # also when the lists may be null
    assert call(B=-1) == BAD_ARG
    # an empty batch is looked at no further than its sizes
    assert call(B=0) == _lib.DL_OK and call(B=0, min_cuts=4, max_cuts=4) == _lib.DL_OK and call(B=0, min_cuts=5) == _lib.DL_OK
    assert call(B=0, N=1, nf=1, capacity=0, R=0) == _lib.DL_OK and call(B=0, N=1024, nf=9, carbon_type=8) == _lib.DL_OK
    assert call(B=0, max_atoms=-3, min_rings=-3) == _lib.DL_OK, 'the gates are any integers'
    for bad in (dict(min_cuts=2), dict(max_cuts=6), dict(min_cuts=5, max_cuts=4), dict(min_cuts=0, max_cuts=0), dict(N=0), dict(N=1025),
                dict(nf=0), dict(carbon_type=8), dict(carbon_type=-1), dict(capacity=-1), dict(R=-1)):
        assert call(B=0, **bad) == BAD_ARG, bad


def test_cpu_tensors_raise():
    B, N = 2, 6
    args = (torch.zeros(B, N, 8), torch.ones(B, N), torch.zeros(B, 5, 3, dtype=torch.int32), torch.zeros(B, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        multi_cuts(*args, is_geom=False, capacity=4)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        multi_all(*args, is_geom=False)


def made_up_result():
    """Two molecules: a centre (atom 2) with four arms of two, by the reference rule with fragments of two, and one without cuts."""
    types = [0] * 9
    entries = [(2, 0, 1), (0, 1, 1), (3, 2, 1), (3, 4, 1), (2, 5, 1), (5, 6, 1), (7, 2, 1), (7, 8, 1)]
    one_hot = np.tile([1.0, 0, 0, 0, 0, 0, 0, 0], (2, 9, 1))
    got = multicut_ref.multicuts(np.ones((2, 9), np.float32), one_hot, np.array([entries, entries]), [8, 2], 5,
                                 min_linker=1, min_fragment=2, **OFF)
    del types
    return MultiCuts(*(torch.as_tensor(got[name]) for name in multicut_ref.FIELDS))


def test_multi_examples():
    result = made_up_result()
    assert result.n_cuts.tolist() == [5, 0] and result.n_cuts_k.tolist() == [[4, 1, 0], [0, 0, 0]]
    symbols = [['C', 'N', 'C', 'C', 'O', 'C', 'F', 'C', 'S'], ['C'] * 9]
    positions = [np.arange(27, dtype=np.float64).reshape(9, 3) / 7, np.zeros((9, 3))]
    data, rows = multi_examples(result, symbols, positions, ['first', 'second'], False, with_rows=True)
    assert multi_examples(result, symbols, positions, ['first', 'second'], False)[0].keys() == data[0].keys()
    assert len(data) == 5 and [item['uuid'] for item in data] == list(range(5))
    assert rows[0] == (0, 3, (0, 2, 4), (2, 2, 2), 3) and rows[4] == (0, 4, (0, 2, 4, 6), (2, 2, 2, 2), 1)
    item = data[0]                               # the arms 0-1, 3-4 and 5-6; the linker is 2, 7, 8
    assert list(item) == ['uuid', 'name', 'positions', 'one_hot', 'charges', 'anchors', 'fragment_mask', 'linker_mask', 'num_atoms']
    assert (item['uuid'], item['name'], item['num_atoms']) == (0, 'first', 9)
    order = [0, 1, 3, 4, 5, 6, 2, 7, 8]
    assert torch.equal(item['positions'], torch.tensor(positions[0][order], dtype=torch.float32))
    assert item['charges'].tolist() == [{'C': 6.0, 'N': 7.0, 'O': 8.0, 'F': 9.0, 'S': 16.0}[symbols[0][k]] for k in order]
    assert item['one_hot'].argmax(1).tolist() == [const.ATOM2IDX[symbols[0][k]] for k in order]
    assert item['anchors'].tolist() == [1.0, 0, 1.0, 0, 1.0, 0, 0, 0, 0], 'the atoms 0, 3 and 5'
    assert item['fragment_mask'].tolist() == [1.0] * 6 + [0.0] * 3 and item['linker_mask'].tolist() == [0.0] * 6 + [1.0] * 3
    assert all(item[k].dtype == torch.float32 for k in list(item)[2:8])
    last = data[4]                               # all four arms: the fragments in the order of their bonds, the linker is atom 2
    assert last['anchors'].nonzero().flatten().tolist() == [0, 2, 4, 6] and last['linker_mask'].tolist() == [0.0] * 8 + [1.0]
    assert torch.equal(last['positions'], torch.tensor(positions[0][[0, 1, 3, 4, 5, 6, 7, 8, 2]], dtype=torch.float32))
    assert multi_examples(result, symbols, positions, ['first', 'second'], True)[0]['one_hot'].shape == (9, const.GEOM_NUMBER_OF_ATOM_TYPES)
    batch = collate([item, last])
    assert batch['positions'].shape == (2, 9, 3) and batch['anchors'].sum(1).flatten().tolist() == [3.0, 4.0]
    truncated = result._replace(n_cuts=torch.tensor([7, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match='multi_all'):
        multi_examples(truncated, symbols, positions, ['first', 'second'], False)


def test_prepare_command_line(capsys):
    assert prepare.MULTI_TABLE_COLUMNS == ('uuid', 'molecule', 'n_cuts', 'anchors', 'n_frags', 'n_linker')
    assert prepare.TABLE_COLUMNS == ('uuid', 'molecule', 'anchor_1', 'anchor_2', 'n_frag_1', 'n_frag_2', 'n_linker')
    assert prepare.SKIP_REASONS == ('malformed', 'unknown_element', 'too_large', 'not_one_piece', 'no_3d')
    base = ['--sdf', 'none.sdf', '--out', 'x', '--prefix', 'y']
    for extra, says in ((['--multi_cuts', '3', '5', '--proteins', 'dir'], '--proteins'), (['--multi_cuts', '2', '5'], 'MIN <= MAX'),
                        (['--multi_cuts', '3', '6'], 'MIN <= MAX'), (['--multi_cuts', '5', '4'], 'MIN <= MAX'),
                        (['--multi_cuts', '3'], 'expected 2 arguments'), (['--multi_cuts', 'a', 'b'], 'invalid int')):
        with pytest.raises(SystemExit) as done:
            prepare.main(base + extra)
        assert done.value.code == 2 and says in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as done:
        prepare.main(['--help'])
    assert done.value.code == 0 and '--multi_min_rings' in capsys.readouterr().out
