"""Molecule keys and scores on the GPU (csrc/mol_keys.hip) against the plain Python restatement ``mol_keys_ref``, bit for
bit, and ``DDPM.sample_and_analyze`` / the training loop's end-of-epoch scoring on toy data sets."""
import json
import os

import numpy as np
import pytest
import torch

import mol_keys_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def torch_scores(types, bonds, keep, limits):
    """n_over and the number of pieces from a bond list, in torch on the CPU: dropped atoms and their bonds go first."""
    n = len(types)
    keep = torch.tensor(keep, dtype=torch.bool)
    rows = torch.tensor(bonds, dtype=torch.long).reshape(-1, 3)
    rows = rows[keep[rows[:, 0]] & keep[rows[:, 1]]]
    valence = torch.zeros(n, dtype=torch.long)
    valence.index_add_(0, rows[:, 0], rows[:, 2])
    valence.index_add_(0, rows[:, 1], rows[:, 2])
    n_over = int(((valence > limits[torch.tensor(types, dtype=torch.long)]) & keep).sum()) if n else 0
    label = torch.arange(n)
    for _ in range(n):
        low = torch.minimum(label[rows[:, 0]], label[rows[:, 1]])
        new = label.clone()
        new.scatter_reduce_(0, rows[:, 0], low, 'amin')
        new.scatter_reduce_(0, rows[:, 1], low, 'amin')
        if torch.equal(new, label):
            break
        label = new
    return n_over, int(label[keep].unique().numel())


def check_against_restatement(one_hot, x, mask, is_geom, drop=None):
    """Every output of ``analyze`` against the restatement (key, colour: the same 64 bits) and the torch scores."""
    from difflinker_amd import const
    from difflinker_amd.metrics import analyze
    dev = lambda t: None if t is None else t.to(DEV)                  # noqa: E731
    got = analyze(dev(one_hot), dev(x), dev(mask), is_geom, drop_mask=dev(drop))
    again = analyze(dev(one_hot), dev(x), dev(mask), is_geom, drop_mask=dev(drop))
    for name in ('n_atoms', 'n_over', 'n_components', 'n_bonds', 'key', 'colour', 'status'):
        assert torch.equal(getattr(got, name), getattr(again, name)), f'{name} differs between two launches'
    B, N = mask.shape[:2]
    assert got.key.dtype == torch.int64 and got.colour.shape == (B, N) and got.n_over.dtype == torch.int32
    limits = const.max_valence_table(is_geom).long()
    n_list, lists = got.bonds.n_bonds.cpu().tolist(), got.bonds.bonds.cpu().tolist()
    assert int(got.bonds.status.max()) == 0 and max(n_list) <= got.bonds.bonds.shape[1], 'analyze never cuts the list'
    real = mask.reshape(B, N) != 0
    keys = []
    for b in range(B):
        types = one_hot[b][real[b]].argmax(1).tolist()
        keep = [True] * len(types) if drop is None else (drop.reshape(B, N)[b][real[b]] == 0).tolist()
        bonds = [tuple(r) for r in lists[b][:n_list[b]]]
        colours, key, n_atoms, n_bonds = ref.colours_and_key(types, bonds, keep)
        n_over, pieces = torch_scores(types, bonds, keep, limits)
        print(f'mol {b}: atoms {n_atoms} bonds {n_bonds} over {n_over} pieces {pieces} key {key:016x} '
              f'got {int(got.key[b]) & ref.M:016x}')
        assert int(got.key[b]) == ref.signed(key), b
        assert got.colour[b].cpu().tolist() == [ref.signed(c) for c in colours] + [0] * (N - len(types)), b
        assert (int(got.n_atoms[b]), int(got.n_bonds[b])) == (n_atoms, n_bonds), b
        assert (int(got.n_over[b]), int(got.n_components[b])) == (n_over, pieces), b
        assert int(got.status[b]) == 0
        keys.append(key)
    return got, keys


def fixture_batch(golden_dir):
    """The 96 molecules of bond_orders.npz in ONE batch: padded to the widest batch and to the GEOM vocabulary, whose
    leading 8 x 8 block of thresholds is the ZINC table, so every molecule keeps its bonds."""
    g = np.load(os.path.join(golden_dir, 'bond_orders.npz'))
    parts = [(g[f'b{k}_one_hot'], g[f'b{k}_x'], g[f'b{k}_mask']) for k in range(int(g['n_batches']))]
    N = max(p[2].shape[1] for p in parts)
    B = sum(len(p[2]) for p in parts)
    one_hot, x, mask = torch.zeros(B, N, 9), torch.zeros(B, N, 3), torch.zeros(B, N, 1)
    at = 0
    for h, pos, m in parts:
        b, n, nf = h.shape
        one_hot[at:at + b, :n, :nf], x[at:at + b, :n], mask[at:at + b, :n, 0] = (torch.from_numpy(a) for a in (h, pos, m))
        at += b
    assert B == 96
    return one_hot, x, mask


def chains(B, N, sizes, nf, seed, spread_rows=True):
    """Random chains with 1.1 .. 1.7 A steps, one time in four from an earlier atom; real rows spread over the N rows."""
    rng = np.random.default_rng(seed)
    one_hot, x, mask = np.zeros((B, N, nf), np.float32), np.zeros((B, N, 3), np.float32), np.zeros((B, N, 1), np.float32)
    for b in range(B):
        n = int(sizes[b])
        pos = np.zeros((n, 3))
        for k in range(1, n):
            parent = k - 1 if rng.random() < 0.75 else rng.integers(0, k)
            step = rng.normal(size=3)
            pos[k] = pos[parent] + step / np.linalg.norm(step) * rng.uniform(1.1, 1.7)
        rows = np.sort(rng.choice(N, size=n, replace=False)) if spread_rows else np.arange(n)
        x[b, rows] = pos
        mask[b, rows] = 1
        one_hot[b, np.arange(N), rng.choice(nf, size=N, p=np.array([6, 3, 3] + [1] * (nf - 3)) / (12 + nf - 3))] = 1
    return torch.from_numpy(one_hot), torch.from_numpy(x), torch.from_numpy(mask)


def test_fixture_molecules_in_one_batch(golden_dir):
    got, keys = check_against_restatement(*fixture_batch(golden_dir), True)
    assert int((got.n_components > 1).sum()) >= 4, 'the fixture holds molecules in several pieces'
    assert len(set(keys)) == 96


def test_ragged_chains_at_50_and_row_permutations():
    rng = np.random.default_rng(4)
    sizes = rng.integers(2, 51, size=64)
    sizes[:2] = (50, 2)
    one_hot, x, mask = chains(64, 50, sizes, 8, seed=50)
    got, keys = check_against_restatement(one_hot, x, mask, False)
    # the same molecules with their rows permuted inside each molecule: the same keys, the colours move with the atoms
    g = torch.Generator().manual_seed(1)
    perm = torch.stack([torch.randperm(50, generator=g) for _ in range(64)])
    take = lambda t: torch.gather(t, 1, perm[:, :, None].expand(-1, -1, t.shape[2]))     # noqa: E731
    moved, moved_keys = check_against_restatement(take(one_hot), take(x), take(mask), False)
    assert moved_keys == keys and torch.equal(moved.key, got.key)
    for name in ('n_atoms', 'n_over', 'n_components', 'n_bonds'):
        assert torch.equal(getattr(moved, name), getattr(got, name))
    assert torch.equal(moved.colour.sort(1).values, got.colour.sort(1).values)


def test_pocket_width_with_250_atoms_dropped():
    B, N = 8, 292
    one_hot, x, mask = chains(B, N, [N] * B, 9, seed=292)
    drop = torch.zeros(B, N, 1)
    g = torch.Generator().manual_seed(2)
    for b in range(B):
        rows = torch.arange(42, N) if b % 2 == 0 else torch.randperm(N, generator=g)[:250]
        drop[b, rows] = 1
    got, _ = check_against_restatement(one_hot, x, mask, True, drop)
    assert got.n_atoms.tolist() == [42] * B
    whole, _ = check_against_restatement(one_hot, x, mask, True)
    assert whole.n_atoms.tolist() == [N] * B
    # dropping atoms is the same as never having had them: the first 42 atoms alone, in a batch of their own
    alone, _ = check_against_restatement(one_hot[::2, :42], x[::2, :42], mask[::2, :42], True)
    assert torch.equal(alone.key, got.key[::2]) and torch.equal(alone.colour, got.colour[::2, :42])
    assert torch.equal(alone.n_over, got.n_over[::2]) and torch.equal(alone.n_components, got.n_components[::2])


def test_one_atom_empty_row_and_no_bond():
    one_hot = torch.zeros(3, 4, 8)
    one_hot[:, :, 0] = 1
    x = torch.zeros(3, 4, 3)
    x[2, :, 0] = torch.arange(4) * 5.0                                 # four carbons 5 A apart: no bond
    mask = torch.zeros(3, 4, 1)
    mask[0, 2] = 1                                                     # one atom, in the third row
    mask[2] = 1                                                        # molecule 1 stays empty
    got, keys = check_against_restatement(one_hot, x, mask, False)
    assert got.n_atoms.tolist() == [1, 0, 4] and got.n_bonds.tolist() == [0, 0, 0] and got.n_components.tolist() == [1, 0, 4]
    assert got.n_over.tolist() == [0, 0, 0] and len(set(keys)) == 3
    assert got.colour[0, 0] != 0 and got.colour[0, 1:].tolist() == [0, 0, 0] and got.colour[1].tolist() == [0] * 4
    # everything dropped
    gone, _ = check_against_restatement(one_hot, x, mask, False, torch.ones(3, 4, 1))
    assert gone.n_atoms.tolist() == [0, 0, 0] and torch.equal(gone.key, got.key[1].expand(3))


def test_cut_list_and_foreign_entries_set_their_bits():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import analyze, molecule_keys
    from difflinker_amd.molecule_builder import Bonds, perceive_bonds
    one_hot = torch.zeros(2, 12, 8, device=DEV)
    one_hot[:, :, 0] = 1
    x = torch.zeros(2, 12, 3, device=DEV)
    x[0, :, 0] = torch.arange(12, device=DEV) * 0.01                   # twelve carbons within 0.11 A: 66 triple bonds
    x[1, :, 0] = torch.arange(12, device=DEV) * 1.5                    # a chain: 11 single bonds
    mask = torch.ones(2, 12, 1, device=DEV)
    cut = perceive_bonds(one_hot, x, mask, False)                      # default capacity 4 * 12 = 48 < 66
    assert cut.status.tolist() == [_lib.DL_BONDS_OVERFLOW, 0]
    keys = molecule_keys(one_hot, mask, cut, False)
    assert keys.status.tolist() == [_lib.DL_BONDS_OVERFLOW, 0], 'the bit is carried forward: this key is of a cut list'
    assert keys.n_over.tolist() == [12, 0] and keys.n_components.tolist() == [1, 1], 'valences and pieces are still whole'
    full = analyze(one_hot, x, mask, False)                            # goes through perceive_all_bonds: never cut
    assert full.status.tolist() == [0, 0] and full.n_bonds.tolist() == [66, 11] and full.n_over.tolist() == [12, 0]
    assert int(full.key[0]) != int(keys.key[0]) and int(full.key[1]) == int(keys.key[1])
    # entries that are not bonds of the molecule (an atom beyond the count, a self bond, order 0) are skipped and flagged
    rows = full.bonds.bonds.clone()
    rows[1, 11] = torch.tensor([12, 0, 1])
    rows[1, 12] = torch.tensor([3, 3, 1])
    rows[1, 13] = torch.tensor([5, -1, 1])
    rows[1, 14] = torch.tensor([4, 2, 0])
    n_bonds = full.bonds.n_bonds.clone()
    n_bonds[1] = 15
    odd = molecule_keys(one_hot, mask, Bonds(n_bonds, rows, *full.bonds[2:]), False)
    assert odd.status.tolist() == [0, _lib.DL_KEYS_BAD_BOND] and torch.equal(odd.key, full.key)
    assert torch.equal(odd.colour, full.colour) and odd.n_bonds.tolist() == [66, 11]
    # a non-finite coordinate is flagged, its atom bonds to nothing
    x[1, 3, 1] = float('nan')
    nan = analyze(one_hot, x, mask, False)
    assert nan.status.tolist() == [0, _lib.DL_BONDS_NONFINITE] and nan.n_components.tolist() == [1, 3]


def test_negative_count_too_many_rows_and_an_empty_batch():
    """What ``dl_molecule_keys`` shares with the other list kernels and no test above reaches: ``n_bonds_in`` below zero reads
    no entry, more than 1024 real rows give DL_KEYS_TOO_LARGE and zeros, and an empty batch launches nothing.  N = 1100 is no
    multiple of 256 and molecule 1 sits in the last rows, in the last threads' ranges."""
    from difflinker_amd import _lib
    from difflinker_amd.metrics import molecule_keys
    from difflinker_amd.molecule_builder import Bonds
    B, N, nf = 2, 1100, 8
    one_hot = torch.zeros(B, N, nf, device=DEV)
    one_hot[0, :, 0] = 1
    one_hot[1, :, 2] = 1
    mask = torch.zeros(B, N, 1, device=DEV)
    mask[0, :1025] = 1
    mask[1, 1093:] = 1                                                  # seven atoms
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)     # noqa: E731
    chain = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 2)]
    found = Bonds(i32([4, -7]), i32([chain, chain]), torch.zeros(B, N, dtype=torch.int32, device=DEV), i32([1022, 7]), None,
                  i32([0, 2]))
    got = molecule_keys(one_hot, mask, found, False)
    colours, key, n_atoms, n_bonds = ref.colours_and_key([2] * 7, [])
    assert got.status.tolist() == [_lib.DL_KEYS_TOO_LARGE, 2]
    assert got.n_atoms.tolist() == [1025, n_atoms] and got.n_bonds.tolist() == [0, n_bonds] and got.n_over.tolist() == [0, 0]
    assert got.n_components.tolist() == [0, 7] and got.key.tolist() == [0, ref.signed(key)]
    assert not got.colour[0].any() and got.colour[1].tolist() == [ref.signed(c) for c in colours] + [0] * (N - 7)
    none = molecule_keys(one_hot[:0], mask[:0], Bonds(i32([]), found.bonds[:0], found.valence[:0], i32([]), None, i32([])), False)
    assert none.key.shape == (0,) and none.colour.shape == (0, N) and none.status.shape == (0,)


# ---- DDPM.sample_and_analyze and the training loop ---------------------------------------------------------------------

def zigzag(n, shift=0.0):
    """A planar zigzag chain with 1.48 A steps: single bonds between neighbours of any of C, O, N and nothing else."""
    k = torch.arange(n, dtype=torch.float32)
    return torch.stack([1.25 * k, 0.8 * (k % 2) + shift, torch.zeros(n)], 1)


def toy_dataset(n_mols, nf, pockets=False, seed=0):
    """Molecules that are valid and in one piece (a zigzag chain over fragment and linker atoms; the pocket is a chain of its
    own 30 A away), in the layout of the preprocessed data sets: fragment, pocket, linker."""
    g = torch.Generator().manual_seed(seed)
    data = []
    for k in range(n_mols):
        n_frag, n_link, n_pock = 6 + k % 4, 3, (5 if pockets else 0)
        n = n_frag + n_pock + n_link
        frag_only, pock, link = torch.zeros(n), torch.zeros(n), torch.zeros(n)
        frag_only[:n_frag] = 1
        pock[n_frag:n_frag + n_pock] = 1
        link[n_frag + n_pock:] = 1
        chain = zigzag(n_frag + n_link)
        pos = torch.cat([chain[:n_frag], zigzag(n_pock, shift=30.0), chain[n_frag:]])
        item = {'uuid': k, 'name': f'mol{k}', 'positions': pos,
                'one_hot': torch.nn.functional.one_hot(torch.randint(0, 3, (n,), generator=g), nf).float(),
                'charges': torch.zeros(n), 'anchors': torch.zeros(n), 'fragment_mask': frag_only + pock,
                'linker_mask': link, 'num_atoms': n}
        if pockets:
            item['fragment_only_mask'] = frag_only
            item['pocket_mask'] = pock
        data.append(item)
    return data


def toy_model(tmp_path, pockets):
    from difflinker_amd import DDPM
    nf = 9 if pockets else 8
    prefix = 'MOAD_test.full' if pockets else 'zinc_final_test'
    torch.save(toy_dataset(5, nf, pockets=pockets), os.path.join(tmp_path, ('MOAD_test_full' if pockets else prefix) + '.pt'))
    hp = dict(in_node_nf=nf, n_dims=3, context_node_nf=2 if pockets else 1, hidden_nf=128, activation='silu', tanh=False,
              n_layers=2, attention=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
              normalization_factor=100, aggregation_method='sum', diffusion_steps=500,
              diffusion_noise_schedule='polynomial_2', diffusion_noise_precision=1e-5, diffusion_loss_type='l2',
              normalize_factors=[1, 4, 10], include_charges=False, model='egnn_dynamics', data_path=str(tmp_path),
              train_data_prefix='MOAD_train.full' if pockets else 'zinc_final_train', val_data_prefix=prefix,
              batch_size=2, lr=2e-4, torch_device=DEV, test_epochs=1, n_stability_samples=3,
              normalization='batch_norm', anchors_context=False, graph_type='FC-10A-4A' if pockets else None)
    torch.manual_seed(0)
    m = DDPM(**hp).to(DEV).eval()
    m.setup('val')
    m.edm.T = 5
    m.edm.noise_source = 'philox'
    return m


def by_hand(m, fails=()):
    """``sample_and_analyze`` spelled out: the same chains in the same order, scored through the public functions."""
    from difflinker_amd.metrics import analyze, compute_metrics, to_host
    pred, true, index, calls, first = [], [], [], 0, 0
    for data in m.val_dataloader():
        drop = data['pocket_mask'] if m.pockets else None
        n = len(data['positions'])
        true_batch = to_host(analyze(data['one_hot'], data['positions'], data['atom_mask'], m.is_geom, drop_mask=drop),
                             data['one_hot'], data['atom_mask'], drop)
        for _ in range(m.n_stability_samples):
            calls += 1
            if calls in fails:
                continue
            chain, node_mask = DDPM_sample_chain(m, data)
            x, one_hot = chain[0][:, :, :3], chain[0][:, :, 3:]
            pred += to_host(analyze(one_hot, x, node_mask, m.is_geom, drop_mask=drop), one_hot, node_mask, drop)
            true += true_batch
            index += range(first, first + n)
        first += n
    return compute_metrics(pred, true, index), pred, true


def DDPM_sample_chain(m, data):
    return type(m).sample_chain(m, data, keep_frames=1)


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_equals_the_metrics_by_hand(tmp_path, pockets, monkeypatch, capsys):
    from difflinker_amd import utils
    from difflinker_amd.metrics import METRIC_NAMES
    m = toy_model(tmp_path, pockets)
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES)
    assert all(type(v) is float and 0.0 <= v <= 1.0 for v in got.values()), got
    m.edm.noise_seed = 5
    want, pred, true = by_hand(m)
    print('sample_and_analyze', got, 'by hand', want)
    assert got == want
    assert len(pred) == 5 * 3 and all(t.n_over == 0 and t.n_components == 1 and t.status == 0 for t in true), \
        'the toy molecules are valid and in one piece, so no prediction is dropped'
    assert all(len(p.graph.types) == len(t.graph.types) for p, t in zip(pred, true)), 'pocket atoms are not in the graphs'

    # a NaN in the second chain: printed in the reference's formats, that sample is skipped, nothing is raised
    calls = {'n': 0}

    def flaky(data, sample_fn=None, keep_frames=None):
        calls['n'] += 1
        if calls['n'] == 2:
            raise utils.FoundNaNException(x_nan_idx={0}, h_nan_idx={0, 1})
        return type(m).sample_chain(m, data, sample_fn=sample_fn, keep_frames=keep_frames)
    monkeypatch.setattr(m, 'sample_chain', flaky, raising=False)
    m.edm.noise_seed = 5
    capsys.readouterr()
    got = m.sample_and_analyze(m.val_dataloader())
    out = capsys.readouterr().out
    assert 'FoundNaNException: [xh], e=0, b=0, i=0: mol0' in out and 'FoundNaNException: [ h], e=0, b=0, i=1: mol1' in out
    monkeypatch.undo()
    m.edm.noise_seed = 5
    want, pred, _ = by_hand(m, fails=(2,))
    assert len(pred) == 5 * 3 - 2 and got == want

    # validation_epoch_end: step metrics and sampling metrics under '<name>/val', the best epoch by validity_and_connectivity
    m.edm.noise_seed = 5
    now = m.validation_epoch_end([{'loss': torch.tensor(2.0)}, {'loss': torch.tensor(4.0)}])
    assert now['loss/val'] == 3.0 and now['best_epoch'] == 0 and now['best_loss/val'] == 3.0
    assert {f'{k}/val' for k in METRIC_NAMES} <= set(now) and m.metrics['validity_and_connectivity/val'] == [now['validity_and_connectivity/val']]
    m.metrics['validity_and_connectivity/val'] += [2.0, 2.0]
    m.metrics['loss/val'] += [7.0, 8.0]
    best, epoch = m.compute_best_validation_metrics()
    assert epoch == 1 and best['loss/val'] == 7.0 and best['validity_and_connectivity/val'] == 2.0
    m.test_dataset = m.val_dataset
    m.current_epoch, m.test_epochs = 0, 2
    assert m.test_epoch_end([{'loss': torch.tensor(1.0)}]) == {'loss/test': 1.0}, 'no sampling before the second epoch'


def test_training_loop_scores_epochs_and_keeps_the_best_checkpoint(tmp_path, capsys):
    from difflinker_amd import DDPM, train
    from difflinker_amd.const import NUMBER_OF_ATOM_TYPES
    torch.save(toy_dataset(6, NUMBER_OF_ATOM_TYPES, seed=0), os.path.join(tmp_path, 'zinc_final_train.pt'))
    torch.save(toy_dataset(3, NUMBER_OF_ATOM_TYPES, seed=1), os.path.join(tmp_path, 'zinc_final_val.pt'))
    cfg = os.path.join(tmp_path, 'cfg.yml')
    with open(cfg, 'w') as f:
        f.write('nf: 128\nn_layers: 1\ninv_sublayers: 1\ntanh: False\nattention: False\nnorm_constant: 0.000001\n'
                'normalization_factor: 100\ninclude_charges: False\nbatch_size: 3\nlr: 0.0002\nnormalize_factors: [1, 4, 10]\n'
                'train_data_prefix: zinc_final_train\nval_data_prefix: zinc_final_val\ndiffusion_steps: 20\n'
                'n_stability_samples: 2\n')
    ck = os.path.join(tmp_path, 'ck')
    # two steps make an epoch: epoch 0 is scored after step 2, the run stops inside epoch 1
    train.main(['--config', cfg, '--data', str(tmp_path), '--checkpoints', ck, '--sample_every_epochs', '1', '--max_steps', '3'])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines()]
    scored = [ln for ln in lines if 'val_epoch' in ln]
    assert len(scored) == 1 and scored[0]['epoch'] == 0 and scored[0]['step'] == 2
    score = scored[0]['val_epoch']['validity_and_connectivity/val']
    assert 0.0 <= score <= 1.0 and 'loss/val' in scored[0]['val_epoch'] and scored[0]['val_epoch']['best_epoch'] == 0
    best = os.path.join(ck, 'best.ckpt')
    assert os.path.exists(best) and os.path.exists(os.path.join(ck, 'last.ckpt'))
    ckpt = torch.load(best, map_location='cpu', weights_only=False)
    assert ckpt['global_step'] == 2 and ckpt['best_validity_and_connectivity'] == score
    assert torch.load(os.path.join(ck, 'last.ckpt'), map_location='cpu', weights_only=False)['global_step'] == 3
    model = DDPM.load_from_checkpoint(best, map_location='cpu', torch_device=DEV).to(DEV).eval()
    model.data_path = str(tmp_path)
    model.setup('val')
    model.edm.T = 5
    chain, _ = model.sample_chain(next(iter(model.val_dataloader())), keep_frames=1)
    assert torch.isfinite(chain).all()


def test_drivers_write_metrics_json_only_when_asked(tmp_path):
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import METRIC_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_generate import IO_DIR, ddpm_hparams
    m = toy_model(tmp_path, False)
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5)
    assert not os.path.exists(os.path.join(plain, 'metrics.json'))
    out = sample(m, str(tmp_path / 'scored'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} and got['molecules'] == 5 * 2
    assert all(0.0 <= got[k] <= 1.0 for k in METRIC_NAMES)
    assert sorted(f for f in os.listdir(os.path.join(out, '0')) if f[0].isdigit()) == ['0_.xyz', '1_.xyz'], 'the files are as without it'
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    files = generate(frag, ddpm, str(tmp_path / 'gen'), n_samples=3, n_steps=5, linker_size='4', metrics=True)
    assert len(files) == 3 and all(f.endswith('.xyz') for f in files)
    got = json.load(open(tmp_path / 'gen' / 'metrics.json'))
    assert set(got) == set(METRIC_NAMES[:4]) | {'molecules'} and got['molecules'] == 3, 'no true molecule: no novelty, no recovery'
    generate(frag, ddpm, str(tmp_path / 'gen_plain'), n_samples=3, n_steps=5, linker_size='4')
    assert 'metrics.json' not in os.listdir(tmp_path / 'gen_plain')
