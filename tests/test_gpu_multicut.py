"""Cuts at three to five bonds on the GPU (``dl_fragment_multicuts``, ``csrc/fragment.hip``) against the plain-Python rule of
``tests/multicut_ref.py``.  Every output is an integer and every comparison is exact: counts, order of records, labels, status.
Every launch of ``launch`` writes into outputs pre-filled with 0x5a bytes, so no result may depend on stale memory.  The public
path (``python -m difflinker_amd.prepare --multi_cuts``, training and sampling on what it wrote) comes last."""
import ctypes
import hashlib
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

import fragment_ref
import multicut_ref
import test_gpu_fragment as double
from test_gpu_fragment import DEV, NF, dev, pack

pytestmark = pytest.mark.gpu
FIELDS = multicut_ref.FIELDS
OFF = multicut_ref.GATES_OFF
SMALL = {'min_linker': 1, 'min_fragment': 1}


def launch(batch, R, charge=True, status=True, carbon_type=fragment_ref.CARBON, **rule):
    """``dl_fragment_multicuts`` itself, into outputs full of 0x5a bytes.  Returns a dict of numpy arrays."""
    from difflinker_amd import _lib
    rule = dict(multicut_ref.DEFAULTS, **rule)
    B, N = batch['mask'].shape
    E = batch['bonds'].shape[1]
    ins = {'one_hot': dev(batch['one_hot'], torch.float32), 'node_mask': dev(batch['mask'], torch.float32),
           'charge': dev(batch['charge'], torch.int32) if charge else None, 'n_bonds_in': dev(batch['n_in'], torch.int32),
           'bonds': dev(batch['bonds'], torch.int32) if E else None, 'status_in': dev(batch['status'], torch.int32) if status else None}
    shapes = {'n_atoms': (B,), 'n_bonds': (B,), 'n_cuttable': (B,), 'n_cuts': (B,), 'status': (B,), 'n_cuts_k': (B, 3),
              'cuts': (B, R, 22), 'labels': (B, R, N)}
    outs = {k: torch.full(s, 0x5a, dtype=torch.uint8, device=DEV) if k == 'labels' else
            torch.full(s, 0x5a5a5a5a, dtype=torch.int32, device=DEV) for k, s in shapes.items()}
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()                          # noqa: E731
    args = _lib.DLFragmentMultiArgs(B=B, N=N, nf=NF, carbon_type=carbon_type, capacity=E, R=R, **rule,
                                    **{k: ptr(t) for k, t in ins.items()}, **{k: ptr(t) for k, t in outs.items()})
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(_lib.load().dl_fragment_multicuts(ctypes.byref(args), stream), 'dl_fragment_multicuts')
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in outs.items()}


def reference(batch, R, charge=True, status=True, carbon_type=fragment_ref.CARBON, **rule):
    return multicut_ref.multicuts(batch['mask'], batch['one_hot'], batch['bonds'], batch['n_in'], R,
                                  batch['charge'] if charge else None, batch['status'] if status else None, carbon_type, **rule)


def assert_exact(got, want, what=''):
    if not isinstance(got, dict):
        got = {name: getattr(got, name).cpu().numpy() for name in FIELDS}
    for name in FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


@pytest.mark.parametrize('sizes', [3, 1])
def test_hand_molecules_in_one_batch(sizes):
    names, batch = double.hand_batch()
    rule = dict(OFF, min_linker=sizes, min_fragment=sizes)
    want = reference(batch, 130, **rule)
    got = launch(batch, 130, **rule)
    assert_exact(got, want)
    kept = dict(zip(names, got['n_cuts_k'].tolist()))
    assert kept['star'] == [{3: 23, 1: 125}[sizes], 0, 0] and all(kept[name] == [0, 0, 0] for name in names if 'chain' in name)
    assert got['status'].tolist() == [0, 2] + [0] * (len(names) - 2), 'the status of the bond list is carried forward'
    again = launch(batch, 130, **rule)
    assert all(got[name].tobytes() == again[name].tobytes() for name in FIELDS), 'the same batch twice: the same bytes'


RANDOM_CASES = [(0, dict(OFF, **SMALL), 40),
                (1, {'min_cuts': 3, 'max_cuts': 3, 'min_linker': 1, 'min_fragment': 2, 'max_atoms': 24, 'min_rings': 1}, 8),
                (6, {'min_cuts': 4, 'max_cuts': 4, 'max_atoms': 26, 'min_rings': 2, **SMALL}, 40),
                (3, dict(OFF, min_cuts=5, max_cuts=5, min_linker=2, min_fragment=1), 40)]


def random_batch(seed):
    rng = np.random.default_rng(seed)
    molecules = [double.random_molecule(rng, int(rng.integers(1, 31))) for _ in range(50)]
    return pack(rng, molecules, 32)


def shows(want, rule):
    """What the reference alone must show of a random batch for the comparison to mean something."""
    ks = range(rule.get('min_cuts', 3), rule.get('max_cuts', 5) + 1)
    seen = {f'kept stars of {k} bonds': want['n_cuts_k'][:, k - 3].any() for k in ks}
    seen.update({f'no stars of {k} bonds': not want['n_cuts_k'][:, k - 3].any() for k in (3, 4, 5) if k not in ks})
    seen.update(truncated=(want['status'] & multicut_ref.TRUNCATED).any(), bad_bond=(want['status'] & multicut_ref.BAD_BOND).any(),
                disconnected=(want['status'] & multicut_ref.DISCONNECTED).any())
    if rule['max_atoms'] < 256:
        loose = {k: v for k, v in rule.items() if k not in ('max_atoms', 'min_rings')}
        rings = want['n_bonds'] - want['n_atoms'] + 1
        seen['stopped by max_atoms'] = (want['n_atoms'] > rule['max_atoms']).any()
        seen['stopped by min_rings'] = ((rings < rule['min_rings']) & (want['n_atoms'] <= rule['max_atoms'])).any()
        seen['_loose'] = loose
    return seen


@pytest.mark.parametrize('seed, rule, R', RANDOM_CASES)
def test_random_molecules(seed, rule, R):
    batch = random_batch(seed)
    want = reference(batch, R, **rule)
    seen = shows(want, rule)
    loose = seen.pop('_loose', None)
    assert all(seen.values()), seen
    if loose is not None:                                               # each gate took cuts away that were there without it
        free = reference(batch, 0, **dict(OFF, **loose))
        rings = want['n_bonds'] - want['n_atoms'] + 1
        assert (free['n_cuts'][want['n_atoms'] > rule['max_atoms']] > 0).any()
        assert (free['n_cuts'][(rings < rule['min_rings']) & (want['n_atoms'] <= rule['max_atoms'])] > 0).any()
    assert_exact(launch(batch, R, **rule), want, seed)


def centre_with_arms(m):
    types, entries = multicut_ref.arms(m)
    return {'types': types, 'entries': entries}


def test_mask_boundaries():
    rng = np.random.default_rng(13)
    R = 300
    chain = lambda n: {'types': [0] * n, 'entries': fragment_ref.chain(n)}                       # noqa: E731
    batch = pack(rng, [centre_with_arms(63), centre_with_arms(64), centre_with_arms(65), chain(256), chain(257)], 260)
    got = launch(batch, R, **OFF, **SMALL)
    assert got['n_atoms'].tolist() == [64, 65, 66, 256, 257] and got['n_cuttable'].tolist() == [63, 64, 65, 255, 0]
    assert got['n_bonds'].tolist() == [63, 64, 65, 255, 0]
    assert got['status'].tolist() == [multicut_ref.TRUNCATED, multicut_ref.TRUNCATED, multicut_ref.MANY_CUTTABLE,
                                      multicut_ref.MANY_CUTTABLE, multicut_ref.TOO_LARGE]
    assert got['n_cuts_k'].tolist() == [[math.comb(63, k) for k in (3, 4, 5)], [math.comb(64, k) for k in (3, 4, 5)]] + [[0] * 3] * 3
    assert got['n_cuts'].tolist() == [sum(math.comb(m, k) for k in (3, 4, 5)) for m in (63, 64)] + [0, 0, 0]
    for b, m in enumerate((63, 64)):
        # arm a is the bond (0, 1 + a), entry a: fragment q is the atom 1 + c_q alone, the linker everything else
        for r, chosen in enumerate(itertools.islice(itertools.combinations(range(m), 3), R)):
            pad = [-1, -1]
            assert got['cuts'][b, r].tolist() == [3, m + 1 - 3] + list(chosen) + pad + [1 + c for c in chosen] + pad + \
                [0, 0, 0] + pad + [1, 1, 1] + pad, (m, r)
            row = np.full(260, 255)
            row[:m + 1] = 5
            row[[1 + c for c in chosen]] = [0, 1, 2]
            assert np.array_equal(got['labels'][b, r], row), (m, r)
    assert not got['cuts'][2:].any() and (got['labels'][2:] == 255).all(), 'nothing else of 65 arms, 255 bonds, 257 atoms'
    # all four and five cuts of 64 arms, counted alone, and the last records of each k through a window at the end
    only = pack(rng, [centre_with_arms(64)], 65)
    for k in (4, 5):
        got = launch(only, 2, **OFF, **SMALL, min_cuts=k, max_cuts=k)
        assert got['n_cuts_k'][0].tolist() == [math.comb(64, k) if q == k else 0 for q in (3, 4, 5)]
        assert got['cuts'][0, 1, :7].tolist() == [k, 65 - k] + list(range(k - 1)) + [k] + [-1] * (5 - k)


def test_edge_cases():
    rng = np.random.default_rng(11)
    star = {'types': [0] * 16, 'entries': fragment_ref.HAND['star'][1]}
    two_pieces = {'types': [0] * 16, 'entries': star['entries'][:7] + star['entries'][8:]}
    molecules = [star, two_pieces, {'types': [0], 'entries': []}, {'types': [], 'entries': []}, dict(star, n_in=-4),
                 dict(star, n_in=40, status=2)]
    batch = pack(rng, molecules, 20)
    rule = dict(OFF, **SMALL)
    for R in (0, 1, 130):                                               # R = 0: cuts and labels are NULL
        want = reference(batch, R, **rule)
        assert_exact(launch(batch, R, **rule), want, R)
    assert want['n_cuts'].tolist() == [125, 0, 0, 0, 0, 125] and want['n_cuttable'].tolist() == [15, 14, 0, 0, 0, 15]
    assert want['status'].tolist() == [0, multicut_ref.DISCONNECTED, 0, 0, multicut_ref.DISCONNECTED,
                                       2 | multicut_ref.BONDS_OVERFLOW | multicut_ref.BAD_BOND], 'the list is read to its capacity'
    for optional in ({'charge': False}, {'status': False}, {'carbon_type': 3}):
        assert_exact(launch(batch, 3, **optional, **rule), reference(batch, 3, **optional, **rule), optional)
    # an empty bond list: capacity 0, `bonds` NULL
    bare = pack(rng, [{'types': [0], 'entries': []}, {'types': [0, 1], 'entries': []}], 5, capacity=0)
    got = launch(bare, 2, **rule)
    assert_exact(got, reference(bare, 2, **rule), 'no list')
    assert got['status'].tolist() == [0, multicut_ref.DISCONNECTED]
    # an empty batch
    none = {k: v[:0] for k, v in batch.items()}
    got = launch(none, 4, **rule)
    assert got['cuts'].shape == (0, 4, 22) and got['n_cuts_k'].shape == (0, 3)
    # N = 1024 rows, a list of more than 256 entries with the bonds at its end
    wide = pack(rng, [{'types': [0] * 16, 'entries': [(0, 0, 0)] * 300 + star['entries']}], 1024)
    got = launch(wide, 30, min_linker=3, min_fragment=3, **OFF)
    assert_exact(got, reference(wide, 30, min_linker=3, min_fragment=3, **OFF), 'wide')
    assert got['n_cuts'].tolist() == [23] and got['cuts'][0, 0, 2:5].min() >= 300


def test_double_cuts_are_what_they_were():
    names, batch = double.hand_batch()
    for rule in ({}, double.LOOSE):
        double.assert_exact(double.launch(batch, 150, **rule), double.reference(batch, 150, **rule))


# ---- the public path ----------------------------------------------------------------------------------------------------------
def ringed_star(arm):
    """A six-ring 0-5 with a three-ring 6-7 on its bond 0-1 closing two more rings (cyclomatic number 3), and tails of ``arm``
    carbons on the ring atoms 2, 3, 4 and 5: ``(types, entries)``."""
    entries = fragment_ref.ring(6) + [(0, 6, 1), (6, 1, 1), (0, 7, 1), (7, 1, 1)]
    for a, root in enumerate((2, 3, 4, 5)):
        entries += fragment_ref.tail(root, 8 + a * arm, arm)
    return [fragment_ref.C] * (8 + 4 * arm), entries


def sha(path):
    with open(path, 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_prepare_multi_then_train_evaluate_and_sample(tmp_path, capsys):
    from difflinker_amd import DDPM, prepare, train
    from difflinker_amd.datasets import ZincDataset, collate, get_dataloader
    from difflinker_amd.evaluate import evaluate
    hand = {'ringed3': ringed_star(3), 'ringed4': ringed_star(4), 'ringed5': ringed_star(5), 'ringed3_again': ringed_star(3)}
    names = ['ringed3', 'ringed4', 'star', 'ringed5', 'ringed3_again']
    fragment_ref.HAND.update({name: (types, entries, {}) for name, (types, entries) in hand.items()})
    try:
        sdf = os.path.join(tmp_path, 'mols.sdf')
        double.write_sdf(sdf, names)
        counts = {name: multicut_ref.hand(name, **multicut_ref.DEFAULTS) for name in set(names)}
    finally:
        for name in hand:
            del fragment_ref.HAND[name]
    per_k = [sum(counts[name]['n_cuts_k'][q] for name in names) for q in range(3)]
    total = sum(per_k)
    assert counts['star']['n_cuts'] == 0 and counts['ringed3']['n_cuts_k'] == [4, 1, 0] and per_k[1] >= 3 and total > 20

    out = str(tmp_path)
    summary = prepare.main(['--sdf', sdf, '--out', out, '--prefix', 'multi', '--multi_cuts', '3', '5', '--geom', '--device', DEV])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary['examples'] == total and summary['files'] == {'multi': total} and not any(summary['molecules_skipped'].values())
    assert summary['examples_by_cuts'] == {'3': per_k[0], '4': per_k[1], '5': per_k[2]} and summary['molecules_with_examples'] == 4
    data = ZincDataset(out, 'multi', 'cpu')
    assert len(data) == total and [item['uuid'] for item in data] == list(range(total))
    assert [item['name'] for item in data] == [name for name in names for _ in range(counts[name]['n_cuts'])]
    first = data[0]                                                     # ringed3, the tails on 2, 3 and 4 cut at the ring
    assert first['num_atoms'] == 20 and first['anchors'].nonzero().flatten().tolist() == [0, 3, 6]
    assert first['fragment_mask'].tolist() == [1.0] * 9 + [0.0] * 11 and first['linker_mask'].tolist() == [0.0] * 9 + [1.0] * 11
    assert torch.equal(first['positions'][0], torch.tensor(8 * double.ZIGZAG[0], dtype=torch.float32)), 'atom 8 comes first'
    four = data[4]
    assert four['anchors'].sum() == 4 and four['linker_mask'].sum() == 8 and four['anchors'].nonzero().flatten().tolist() == [0, 3, 6, 9]
    with open(os.path.join(out, 'multi_table.csv')) as f:
        table = f.read().splitlines()
    assert table[0] == ','.join(prepare.MULTI_TABLE_COLUMNS) and len(table) == total + 1
    assert table[1] == '0,ringed3,3,0-3-6,3-3-3,11' and table[5] == '4,ringed3,4,0-3-6-9,3-3-3-3,8'

    # split by molecule, then two optimiser steps and the held-out loss on what was written
    split = prepare.main(['--sdf', sdf, '--out', out, '--prefix', 'geom_multi', '--multi_cuts', '3', '5', '--geom',
                          '--val_fraction', '0.3', '--seed', '1', '--max_per_molecule', '6', '--device', DEV])
    files = split['files']
    assert files['geom_multi_train'] + files['geom_multi_val'] == split['examples'] and min(files.values()) > 0
    assert split['examples'] == sum(min(counts[name]['n_cuts'], 6) for name in names)
    held_out = ZincDataset(out, 'geom_multi_val', 'cpu')
    assert [item['uuid'] for item in held_out] == list(range(len(held_out)))
    assert not {item['name'] for item in held_out} & {item['name'] for item in ZincDataset(out, 'geom_multi_train', 'cpu')}
    cfg = os.path.join(tmp_path, 'cfg.yml')
    with open(cfg, 'w') as f:
        f.write('nf: 128\nn_layers: 1\ninv_sublayers: 1\ntanh: False\nattention: False\nnorm_constant: 0.000001\n'
                'normalization_factor: 100\ninclude_charges: False\nbatch_size: 3\nlr: 0.0002\nnormalize_factors: [1, 4, 10]\n'
                'train_data_prefix: geom_multi_train\nval_data_prefix: geom_multi_val\ndiffusion_steps: 20\n'
                'center_of_mass: anchors\nremove_anchors_context: False\n')
    capsys.readouterr()
    ckpt = train.main(['--config', cfg, '--data', out, '--checkpoints', os.path.join(tmp_path, 'ck'), '--max_steps', '2',
                       '--no_validation', '--device', DEV])
    steps = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines() if '"loss"' in ln]
    assert [s['step'] for s in steps] == [1, 2] and all(math.isfinite(s['loss']) for s in steps)
    model = DDPM.load_from_checkpoint(ckpt, map_location='cpu', torch_device=DEV).to(DEV).eval()
    model.data_path = out
    model.setup('val')
    scores = evaluate(model, model.val_dataloader())
    assert math.isfinite(scores['loss']) and math.isfinite(scores['l2_loss'])
    batch = next(iter(get_dataloader(held_out, 2, collate_fn=collate)))
    batch = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in batch.items()}
    chain, node_mask = model.sample_chain(batch, keep_frames=1)
    x = chain[0][:, :, :3]
    assert torch.isfinite(chain).all()
    centre = (batch['positions'] * batch['anchors']).sum(1, keepdim=True) / batch['anchors'].sum(1, keepdim=True)
    still = batch['fragment_mask'].bool().squeeze(-1)
    # coordinates reach 40 A, where an fp32 ulp is 3.8e-6: a few roundings of the centring on either side
    assert torch.allclose(x[still], (batch['positions'] - centre)[still], atol=1e-4), 'every fragment atom stays where it was'

    # without --multi_cuts: what the double-cut run has always written
    double_names = ['chain13', 'chain14', 'amide', 'orders', 'charged', 'chain14', 'ester']
    double.write_sdf(sdf, double_names)
    prepare.main(['--sdf', sdf, '--out', out, '--prefix', 'mine', '--device', DEV])
    with open(os.path.join(out, 'mine_table.csv'), newline='') as f:
        text = f.read()
    assert hashlib.sha256(text.encode()).hexdigest() == DOUBLE_TABLE_SHA256
    items = torch.load(os.path.join(out, 'mine.pt'), map_location='cpu')
    digest = hashlib.sha256()
    for item in items:
        assert list(item) == ['uuid', 'name', 'positions', 'one_hot', 'charges', 'anchors', 'fragment_mask', 'linker_mask', 'num_atoms']
        for key, value in item.items():
            digest.update(value.numpy().tobytes() if torch.is_tensor(value) else repr(value).encode())
    assert digest.hexdigest() == DOUBLE_ITEMS_SHA256


# sha256 of what `prepare.main --sdf <the seven hand molecules> --prefix mine` wrote on the commit before --multi_cuts existed:
# the text of mine_table.csv, and the contents of mine.pt item by item (tensors as bytes, everything else by repr).  Recorded
# from that commit's prepare.py and fragment.examples, with tests/fragment_ref.py in the kernel's place (its tests pin the two
# to the same integers)
DOUBLE_TABLE_SHA256 = 'b141067e7fcd973fc7a7de80f79843289314580e4f17b0b9ca45a79534054202'
DOUBLE_ITEMS_SHA256 = 'cd1966984ae0faff3331db165ba27ad7dbd3293d777124a01b75d2b8c0407f77'
