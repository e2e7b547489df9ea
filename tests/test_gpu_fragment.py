"""Double cuts on the GPU (``dl_fragment_cuts``, ``csrc/fragment.hip``) against the plain-Python rule of
``tests/fragment_ref.py``.  Every output is an integer and every comparison is exact: counts, order of records, labels, status.
Every launch of ``launch`` writes into outputs pre-filled with 0x5a bytes, so no result may depend on stale memory.  The public
path (``fragment_all``, ``python -m difflinker_amd.prepare``, training on what it wrote) comes last."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import fragment_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = fragment_ref.FIELDS
NF = 8
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read
LOOSE = {'min_linker': 1, 'min_fragment': 1, 'min_path_atoms': 1, 'linker_leq_frags': 0}


def pack(rng, molecules, width, capacity=None):
    """``molecules``: dicts with ``types`` (by atom), ``entries`` and optionally ``charges`` (by atom), ``n_in``, ``status``.
    Real rows are scattered over ``width``; rows that are not real carry garbage types and charges."""
    B = len(molecules)
    capacity = max(len(m['entries']) for m in molecules) + 3 if capacity is None else capacity
    out = {'mask': np.zeros((B, width), np.float32), 'one_hot': rng.random((B, width, NF)).astype(np.float32),
           'charge': rng.integers(-1, 2, (B, width)).astype(np.int32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_in': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32)}
    out['bonds'][:] = GARBAGE
    for b, m in enumerate(molecules):
        n = len(m['types'])
        real = np.sort(rng.choice(width, n, replace=False))
        out['mask'][b, real] = 1
        out['one_hot'][b, real] = np.eye(NF, dtype=np.float32)[np.asarray(m['types'], dtype=int)] if n else 0
        out['charge'][b, real] = m.get('charges', [0] * n)
        if m['entries']:
            out['bonds'][b, :len(m['entries'])] = m['entries']
        out['n_in'][b] = m.get('n_in', len(m['entries']))
        out['status'][b] = m.get('status', 0)
    return out


def dev(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def launch(batch, R, charge=True, status=True, carbon_type=fragment_ref.CARBON, **rule):
    """``dl_fragment_cuts`` itself, into outputs full of 0x5a bytes.  Returns a dict of numpy arrays."""
    from difflinker_amd import _lib
    rule = dict(fragment_ref.DEFAULTS, **rule)
    B, N = batch['mask'].shape
    E = batch['bonds'].shape[1]
    ins = {'one_hot': dev(batch['one_hot'], torch.float32), 'node_mask': dev(batch['mask'], torch.float32),
           'charge': dev(batch['charge'], torch.int32) if charge else None, 'n_bonds_in': dev(batch['n_in'], torch.int32),
           'bonds': dev(batch['bonds'], torch.int32) if E else None, 'status_in': dev(batch['status'], torch.int32) if status else None}
    shapes = {'n_atoms': (B,), 'n_bonds': (B,), 'n_cuttable': (B,), 'n_cuts': (B,), 'status': (B,), 'bond_side': (B, E),
              'cuts': (B, R, 10), 'labels': (B, R, N)}
    outs = {k: torch.full(s, 0x5a, dtype=torch.uint8, device=DEV) if k == 'labels' else
            torch.full(s, 0x5a5a5a5a, dtype=torch.int32, device=DEV) for k, s in shapes.items()}
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()                          # noqa: E731
    args = _lib.DLFragmentArgs(B=B, N=N, nf=NF, carbon_type=carbon_type, capacity=E, R=R, **rule,
                               **{k: ptr(t) for k, t in ins.items()}, **{k: ptr(t) for k, t in outs.items()})
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(_lib.load().dl_fragment_cuts(ctypes.byref(args), stream), 'dl_fragment_cuts')
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in outs.items()}


def reference(batch, R, charge=True, status=True, carbon_type=fragment_ref.CARBON, **rule):
    return fragment_ref.fragment_cuts(batch['mask'], batch['one_hot'], batch['bonds'], batch['n_in'], R,
                                      batch['charge'] if charge else None, batch['status'] if status else None, carbon_type, **rule)


def assert_exact(got, want, what=''):
    if not isinstance(got, dict):
        got = {name: getattr(got, name).cpu().numpy() for name in FIELDS}
    for name in FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def hand_batch():
    rng = np.random.default_rng(5)
    names = sorted(fragment_ref.HAND)
    molecules = []
    for k, name in enumerate(names):
        types, entries, charged = fragment_ref.HAND[name]
        molecules.append({'types': types, 'entries': entries, 'charges': [charged.get(a, 0) for a in range(len(types))],
                          'status': 2 if k == 1 else 0})
    return names, pack(rng, molecules, 40)


@pytest.mark.parametrize('rule', [{}, {'linker_leq_frags': 0}, {'linker_leq_frags': 0, 'min_path_atoms': 1}, LOOSE],
                         ids=['defaults', 'any_linker', 'any_path', 'loose'])
def test_hand_molecules_in_one_batch(rule):
    names, batch = hand_batch()
    R = 150 if rule is LOOSE else 8
    got = launch(batch, R, **rule)
    assert_exact(got, reference(batch, R, **rule))
    cuts = dict(zip(names, got['n_cuts'].tolist()))
    if not rule:
        assert cuts == dict.fromkeys(names, 0) | {'chain13': 1, 'chain14': 3, 'amide': 1, 'ester': 1, 'orders': 1}
        assert got['cuts'][names.index('chain13'), 0].tolist() == [4, 7, 4, 5, 8, 7, 5, 5, 3, 3]
    if rule == {'linker_leq_frags': 0}:
        assert (cuts['biphenyl_tails'], cuts['ring_linker'], cuts['star']) == (3, 1, 0)
    if rule == {'linker_leq_frags': 0, 'min_path_atoms': 1}:
        assert cuts['star'] == 3
    again = launch(batch, R, **rule)
    assert all(got[name].tobytes() == again[name].tobytes() for name in FIELDS), 'the same batch twice: the same bytes'


def random_molecule(rng, n):
    """A random tree plus 0..4 ring closures; random orders, types and charges; entries in both orientations and random order,
    a few of them repeated (with an order of their own) or out of range."""
    pairs = [(k, int(rng.integers(0, k))) for k in range(1, n)]
    have = {(min(p), max(p)) for p in pairs}
    for _ in range(int(rng.integers(0, 5))):
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if i != j and (min(i, j), max(i, j)) not in have:
            have.add((min(i, j), max(i, j)))
            pairs.append((i, j))
    entries = [(i, j) if rng.random() < 0.5 else (j, i) for i, j in pairs]
    entries = [(i, j, 1 if rng.random() < 0.7 else int(rng.integers(2, 5))) for i, j in entries]
    entries = [entries[k] for k in rng.permutation(len(entries))]
    if entries and rng.random() < 0.25:
        for _ in range(int(rng.integers(1, 3))):
            i, j, _ = entries[int(rng.integers(0, len(entries)))]
            entries.insert(int(rng.integers(0, len(entries) + 1)), (j, i, int(rng.integers(1, 5))))
    if rng.random() < 0.15:
        entries.insert(int(rng.integers(0, len(entries) + 1)),
                       [(n, 0, 1), (0, 0, 1), (-1, 0, 1), (0, n - 1, 0), (0, n - 1, 5)][int(rng.integers(0, 5))])
    types = np.where(rng.random(n) < 0.6, 0, rng.integers(1, NF, n)).tolist()
    charges = np.where(rng.random(n) < 0.9, 0, rng.integers(-1, 2, n)).tolist()
    n_in = len(entries) - int(rng.random() < 0.1 and len(entries) > 0)      # the last entry left out: often two pieces
    return {'types': types, 'entries': entries, 'charges': charges, 'n_in': n_in}


@pytest.mark.parametrize('seed, rule', [(0, {}), (1, LOOSE), (2, {'min_linker': 2, 'min_fragment': 3, 'min_path_atoms': 3, 'linker_leq_frags': 0}),
                                        (3, {'linker_leq_frags': 0})])
def test_random_molecules(seed, rule):
    rng = np.random.default_rng(seed)
    molecules = [random_molecule(rng, int(rng.integers(1, 61))) for _ in range(50)]
    batch = pack(rng, molecules, 64)
    want = reference(batch, 48, **rule)
    got = launch(batch, 48, **rule)
    assert_exact(got, want, seed)
    assert want['n_cuts'].max() > 0 and (want['status'] & fragment_ref.BAD_BOND).any()
    assert (want['status'] & fragment_ref.DISCONNECTED).any()
    if rule is LOOSE:
        assert (want['status'] & fragment_ref.TRUNCATED).any() and (want['n_cuttable'] > 20).any()


def chain_with_rings(n, rings=3):
    """A chain of ``n`` atoms with ``rings`` six-rings closed along it (k, k + 5), the last one at the very end."""
    entries = fragment_ref.chain(n)
    for k in [n - 6, n // 2, 3][:rings]:
        if 0 <= k and k + 5 < n:
            entries.append((k + 5, k, 1))
    return {'types': [0] * n, 'entries': entries}


def test_word_boundaries_of_the_bit_sets():
    rng = np.random.default_rng(7)
    small = pack(rng, [chain_with_rings(n) for n in (63, 64, 65, 66)], 80)
    assert_exact(launch(small, 256, min_fragment=20), reference(small, 256, min_fragment=20), 'small')
    big = pack(rng, [chain_with_rings(n) for n in (255, 256, 257, 129)], 300)
    rule = {'min_fragment': 110}
    want = reference(big, 700, **rule)
    got = launch(big, 700, **rule)
    assert_exact(got, want, 'big')
    assert want['n_atoms'].tolist() == [255, 256, 257, 129] and want['status'].tolist() == [0, 0, fragment_ref.TOO_LARGE, 0]
    assert want['n_cuttable'][1] == 255 - 3 * 5 and want['n_cuts'][0] > 256 and want['n_cuts'][1] > want['n_cuts'][0]
    assert (got['labels'][2] == 255).all() and not got['cuts'][2].any(), 'nothing but the atom count of a molecule too large'


def test_truncation_and_fragment_all():
    from difflinker_amd.fragment import fragment_all, fragment_cuts
    rng = np.random.default_rng(9)
    molecules = [{'types': [0] * n, 'entries': fragment_ref.chain(n)} for n in (14, 12, 20, 13)]
    batch = pack(rng, molecules, 24)
    full = reference(batch, 40)
    assert full['n_cuts'].tolist() == [3, 0, 24, 1]
    got = launch(batch, 2)
    assert_exact(got, reference(batch, 2))
    assert got['n_cuts'].tolist() == [3, 0, 24, 1], 'the count is complete'
    assert (got['status'] & fragment_ref.TRUNCATED != 0).tolist() == [True, False, True, False]
    assert np.array_equal(got['cuts'], full['cuts'][:, :2]) and np.array_equal(got['labels'], full['labels'][:, :2])
    tensors = (dev(batch['one_hot'], torch.float32), dev(batch['mask'], torch.float32), dev(batch['bonds'], torch.int32),
               dev(batch['n_in'], torch.int32))
    extra = {'charge': dev(batch['charge'], torch.int32), 'status': dev(batch['status'], torch.int32)}
    assert_exact(fragment_cuts(*tensors, is_geom=False, capacity=2, **extra), reference(batch, 2), 'the wrapper')
    assert_exact(fragment_all(*tensors, is_geom=False, capacity=2, **extra), reference(batch, 24), 'widened once')
    assert_exact(fragment_all(*tensors, is_geom=False, **extra), reference(batch, 64), 'wide enough from the start')


def test_edge_cases():
    rng = np.random.default_rng(11)
    chain14 = {'types': [0] * 14, 'entries': fragment_ref.chain(14)}
    two_pieces = {'types': [0] * 14, 'entries': fragment_ref.chain(7) + fragment_ref.chain(7, 7)}
    molecules = [chain14, two_pieces, {'types': [0], 'entries': []}, {'types': [], 'entries': []},
                 {'types': [0] * 14, 'entries': fragment_ref.chain(14), 'n_in': -4},
                 {'types': [0] * 14, 'entries': fragment_ref.chain(14), 'n_in': 40, 'status': 2}]
    batch = pack(rng, molecules, 20)
    for R in (0, 1, 5):                                                 # R = 0: cuts and labels are NULL
        want = reference(batch, R)
        assert_exact(launch(batch, R), want, R)
    assert want['n_cuts'].tolist() == [3, 0, 0, 0, 0, 3] and want['n_cuttable'].tolist() == [13, 12, 0, 0, 0, 13]
    assert want['status'].tolist() == [0, fragment_ref.DISCONNECTED, 0, 0, fragment_ref.DISCONNECTED,
                                       2 | fragment_ref.BONDS_OVERFLOW | fragment_ref.BAD_BOND], 'the list is read to its capacity'
    for optional in ({'charge': False}, {'status': False}, {'carbon_type': 3}):
        assert_exact(launch(batch, 3, **optional), reference(batch, 3, **optional), optional)
    # an empty bond list: capacity 0, `bonds` and `bond_side` NULL
    bare = pack(rng, [{'types': [0], 'entries': []}, {'types': [0, 1], 'entries': []}], 5, capacity=0)
    got = launch(bare, 2)
    assert_exact(got, reference(bare, 2), 'no list')
    assert got['status'].tolist() == [0, fragment_ref.DISCONNECTED] and got['bond_side'].shape == (2, 0)
    # an empty batch
    none = {k: v[:0] for k, v in batch.items()}
    got = launch(none, 4)
    assert got['cuts'].shape == (0, 4, 10) and got['n_cuts'].shape == (0,)
    # N = 1024 rows, a list of more than 256 entries with the bonds at its end
    wide = pack(rng, [{'types': [0] * 13, 'entries': [(0, 0, 0)] * 300 + fragment_ref.chain(13)}], 1024)
    got = launch(wide, 2)
    assert_exact(got, reference(wide, 2), 'wide')
    assert got['n_cuts'].tolist() == [1] and got['cuts'][0, 0, :2].tolist() == [304, 307]


ZIGZAG = np.array([[1.25, 0.0, 0.0], [0.0, 0.75, 0.5]])


def write_sdf(path, molecules):
    """V2000 records of hand molecules (``fragment_ref.HAND`` names), atoms along a zigzag line."""
    symbol = {fragment_ref.C: 'C', fragment_ref.N_: 'N', fragment_ref.O: 'O'}
    with open(path, 'w') as f:
        for name in molecules:
            types, entries, charged = fragment_ref.HAND[name]
            f.write(f'{name}\n  by hand                 3D\n\n%3d%3d  0  0  0  0  0  0  0  0999 V2000\n' % (len(types), len(entries)))
            for k, t in enumerate(types):
                x, y, z = k * ZIGZAG[0] + (k % 2) * ZIGZAG[1]
                f.write('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0\n' % (x, y, z, symbol[t]))
            for i, j, order in entries:
                f.write('%3d%3d%3d  0  0  0  0\n' % (i + 1, j + 1, order))
            for atom, charge in charged.items():
                f.write('M  CHG  1 %3d %3d\n' % (atom + 1, charge))
            f.write('M  END\n$$$$\n')


def test_prepare_then_train_and_evaluate(tmp_path, capsys):
    from difflinker_amd import DDPM, const, prepare, train
    from difflinker_amd.datasets import ZincDataset, collate, get_dataloader
    from difflinker_amd.evaluate import evaluate
    names = ['chain13', 'chain14', 'amide', 'orders', 'charged', 'chain14', 'ester']
    sdf = os.path.join(tmp_path, 'mols.sdf')
    write_sdf(sdf, names)
    counts = {name: fragment_ref.hand(name)['n_cuts'] for name in names}
    assert sum(counts[name] for name in names) == 10

    summary = prepare.main(['--sdf', sdf, '--out', str(tmp_path), '--prefix', 'mine', '--device', DEV])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary['molecules_read'] == 7 and summary['examples'] == 10 and summary['files'] == {'mine': 10}
    assert not any(summary['molecules_skipped'].values())
    data = ZincDataset(str(tmp_path), 'mine', 'cpu')
    assert len(data) == 10 and [item['name'] for item in data] == [n for n in names for _ in range(counts[n])]
    assert [item['uuid'] for item in data] == list(range(10))
    amide = next(item for item in data if item['name'] == 'amide')
    o, n_, c = (const.ATOM2IDX[s] for s in 'ONC')
    assert amide['one_hot'].argmax(1).tolist() == [c] * 10 + [c, o, n_] and amide['linker_mask'].tolist() == [0.0] * 10 + [1.0] * 3
    assert amide['anchors'].nonzero().flatten().tolist() == [4, 5] and amide['charges'].tolist() == [6.0] * 11 + [8.0, 7.0]
    assert torch.equal(amide['positions'][10], torch.tensor(5 * ZIGZAG[0] + ZIGZAG[1], dtype=torch.float32))
    batches = list(get_dataloader(data, 4, collate_fn=collate))
    assert [b['positions'].shape[0] for b in batches] == [4, 4, 2] and batches[0]['positions'].shape[1:] == (14, 3)
    with open(os.path.join(tmp_path, 'mine_table.csv')) as f:
        table = f.read().splitlines()
    assert table[0] == 'uuid,molecule,anchor_1,anchor_2,n_frag_1,n_frag_2,n_linker' and len(table) == 11
    assert table[1] == '0,chain13,4,5,5,5,3'

    # split by molecule, then two optimiser steps and the held-out loss on what was written
    split = prepare.main(['--sdf', sdf, '--out', str(tmp_path), '--prefix', 'zinc_final', '--val_fraction', '0.3', '--seed', '1',
                          '--device', DEV])
    files = split['files']
    assert files['zinc_final_train'] + files['zinc_final_val'] == 10 and min(files.values()) > 0
    held_out = ZincDataset(str(tmp_path), 'zinc_final_val', 'cpu')
    assert len(held_out) == files['zinc_final_val'] and [item['uuid'] for item in held_out] == list(range(len(held_out)))
    cfg = os.path.join(tmp_path, 'cfg.yml')
    with open(cfg, 'w') as f:
        f.write('nf: 128\nn_layers: 1\ninv_sublayers: 1\ntanh: False\nattention: False\nnorm_constant: 0.000001\n'
                'normalization_factor: 100\ninclude_charges: False\nbatch_size: 3\nlr: 0.0002\nnormalize_factors: [1, 4, 10]\n'
                'train_data_prefix: zinc_final_train\nval_data_prefix: zinc_final_val\ndiffusion_steps: 20\n')
    capsys.readouterr()
    ckpt = train.main(['--config', cfg, '--data', str(tmp_path), '--checkpoints', os.path.join(tmp_path, 'ck'), '--max_steps', '2',
                       '--no_validation', '--device', DEV])
    steps = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines() if '"loss"' in ln]
    assert [s['step'] for s in steps] == [1, 2] and all(math.isfinite(s['loss']) for s in steps)
    model = DDPM.load_from_checkpoint(ckpt, map_location='cpu', torch_device=DEV).to(DEV).eval()
    model.data_path = str(tmp_path)
    model.setup('val')
    scores = evaluate(model, model.val_dataloader())
    assert math.isfinite(scores['loss']) and math.isfinite(scores['l2_loss'])
