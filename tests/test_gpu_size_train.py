"""Training of the linker-size predictor on the GPU (csrc/size_gnn_train.hip): gradients, logits and BatchNorm statistics
against fp64 autograd of a train-mode restatement (tests/size_train_ref.py) and against the unmodified reference's
``loss.backward()`` (tests/golden/size_grad.npz), bitwise repeatability, the edge cases of the row layout, re-folding after
an optimiser step, an AdamW trajectory, a short overfit and the ``python -m difflinker_amd.train_size_gnn`` loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import rel_l2, seeded_size_state_dict
from size_train_ref import size_batch, train_logits, true_labels

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_ALL, BAR_TENSOR = 2e-6, 1e-5       # the FC backward's bars
IN_NF, OUT_NF = 8, 10


def make_clf(L, bn, seed, loss_weights=None):
    from difflinker_amd.linker_size import SizeClassifier
    clf = SizeClassifier(in_node_nf=IN_NF, hidden_nf=128, out_node_nf=OUT_NF, n_layers=L,
                         normalization='batch_norm' if bn else None, loss_weights=loss_weights)
    sd = seeded_size_state_dict(IN_NF, 128, OUT_NF, L, seed=seed, batch_norm=bn, prefix='gnn.')
    clf.load_state_dict(sd, strict=True)
    return clf.to(DEV).train(), sd


def to_dev(d):
    out = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}
    out.pop('edges', None)
    return out


def ref_run(sd, data, L, bn, weights=None):
    """fp64 logits, loss, gradients (state_dict keys) and batch statistics of the restatement."""
    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    d = lambda k: data[k].detach().cpu().double()       # noqa: E731
    out, stats = train_logits(p, d('one_hot'), d('positions'), d('fragment_mask'), d('edge_mask'), L, bn)
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    loss = torch.nn.functional.cross_entropy(out, true_labels(data['linker_mask'].cpu()), weight=w)
    loss.backward()
    return out.detach(), loss.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}, stats


def hip_run(clf, data):
    clf.zero_grad(set_to_none=True)
    logits, loss = clf.training_forward(to_dev(data))
    loss.backward()
    return logits.detach().cpu(), loss.detach().cpu(), {'gnn.' + k: p.grad.detach().cpu() for k, p in clf.gnn.named_parameters()}


def pre_bn_bias(key):
    """Biases right before a train-mode BatchNorm: their true gradient is exactly 0 (the batch mean cancels them)."""
    return key.endswith('node_mlp.0.bias') or key.endswith('node_mlp.3.bias')


def compare(hip, ref, bn):
    keys = [k for k in ref if k in hip]
    a = torch.cat([hip[k].double().reshape(-1) for k in keys])
    b = torch.cat([ref[k].double().reshape(-1) for k in keys])
    per = {k: rel_l2(hip[k], ref[k]) for k in keys if not (bn and pre_bn_bias(k))}
    zeros = max([float(hip[k].double().norm()) / float(b.norm()) for k in keys if bn and pre_bn_bias(k)] + [0.0])
    return rel_l2(a, b), max(per.values()), zeros


CASES = {   # sizes, linkers, n_layers, BatchNorm, loss weights
    'bn1_ragged': ([12, 20, 7, 30], [4, 6, 2, 8], 1, True, False),
    'bn2_weights': ([15, 9, 26, 11, 5], [5, 3, 9, 4, 0], 2, True, True),
    'plain3': ([18, 25, 9], [6, 8, 3], 3, False, False),
    'plain4_weights': ([10, 33, 21], [3, 10, 4], 4, False, True),
    'bn5': ([22, 14, 35, 17, 28, 12], [7, 4, 12, 5, 9, 3], 5, True, False),
}


@pytest.mark.parametrize('case', list(CASES))
def test_grad_matches_fp64_restatement(case):
    sizes, linkers, L, bn, weighted = CASES[case]
    weights = torch.linspace(0.3, 3.0, OUT_NF).tolist() if weighted else None
    clf, sd = make_clf(L, bn, seed=700 + L, loss_weights=weights)
    # chain-like molecules: a few kept edges per atom.  (In a dense cloud, fp32 and fp64 put some of the millions of ReLU
    # inputs on different sides of the kink, and the gradient is not continuous there.)
    data = size_batch(sizes, linkers, IN_NF, seed=sum(sizes), scale=0.9, chain=True)
    ref_out, ref_loss, ref_g, ref_stats = ref_run(sd, data, L, bn, weights)
    out, loss, g = hip_run(clf, data)
    assert rel_l2(out, ref_out) <= 1e-5 and abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    overall, worst, zeros = compare(g, ref_g, bn)
    print(f'[size grad {case}] rel-L2 all {overall:.3e}, worst tensor {worst:.3e}, pre-BN biases {zeros:.1e}')
    assert overall <= BAR_ALL and worst <= BAR_TENSOR and zeros <= 1e-5
    if bn:                                          # running statistics after one step (momentum 0.1, unbiased var)
        n = data['positions'].shape[0] * data['positions'].shape[1]
        for key, (mean, var) in ref_stats.items():
            rm = 0.9 * sd[key + '.running_mean'].double() + 0.1 * mean
            rv = 0.9 * sd[key + '.running_var'].double() + 0.1 * var * n / (n - 1)
            mod = clf.get_submodule(key)
            assert rel_l2(mod.running_mean.cpu(), rm) <= 1e-5 and rel_l2(mod.running_var.cpu(), rv) <= 1e-5
            assert int(mod.num_batches_tracked) == 8


@pytest.mark.parametrize('tag', ['bn2', 'plain3', 'bn1_full'])
def test_grad_matches_reference_fixture(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, 'size_grad.npz'))
    L, bn, weighted, seed = [int(v) for v in z[f'{tag}.params']]
    weights = z['loss_weights'].tolist() if weighted else None
    clf, _ = make_clf(L, bool(bn), seed, loss_weights=weights)
    data = {k: torch.from_numpy(z[f'{tag}.{k}']) for k in ('one_hot', 'positions', 'fragment_mask', 'linker_mask', 'edge_mask')}
    out, loss, g = hip_run(clf, data)
    assert rel_l2(out, torch.from_numpy(z[f'{tag}.logits'])) <= 1e-5
    assert abs(float(loss) - float(z[f'{tag}.loss'])) <= 1e-5 * abs(float(z[f'{tag}.loss']))
    hip, ref = {}, {}
    for k in z.files:
        if not k.startswith(tag + '.grad.'):
            continue
        key = 'gnn.' + k[len(tag) + 6:]
        v = g[key].reshape(-1)
        if f'{tag}.idx.{key[4:]}' in z.files:
            v = v[torch.from_numpy(z[f'{tag}.idx.{key[4:]}']).long()]
        hip[key], ref[key] = v, torch.from_numpy(z[k])
    overall, worst, zeros = compare(hip, ref, bool(bn))
    print(f'[size grad fixture {tag}] rel-L2 all {overall:.3e}, worst tensor {worst:.3e}, pre-BN biases {zeros:.1e}')
    assert overall <= BAR_ALL and worst <= BAR_TENSOR and zeros <= 1e-5
    for k in z.files:
        if k.startswith(tag + '.stat.'):
            key = k[len(tag) + 6:]
            mod, attr = key.rsplit('.', 1)
            assert rel_l2(getattr(clf.gnn.get_submodule(mod), attr).cpu(), torch.from_numpy(z[k])) <= 1e-5


def test_gradient_is_bitwise_repeatable():
    clf, _ = make_clf(3, True, seed=711)
    data = size_batch([17, 30, 9, 24], [5, 9, 2, 7], IN_NF, seed=5)
    _, _, g1 = hip_run(clf, data)
    _, _, g2 = hip_run(clf, data)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)


def test_two_forwards_before_their_backwards():
    clf, _ = make_clf(2, False, seed=712)
    d1 = to_dev(size_batch([12, 8], [3, 2], IN_NF, seed=6))
    d2 = to_dev(size_batch([20, 15, 9], [5, 4, 3], IN_NF, seed=7))
    _, l1 = clf.training_forward(d1)
    _, l2 = clf.training_forward(d2)
    (l1 + l2).backward()
    both = {k: p.grad.clone() for k, p in clf.gnn.named_parameters()}
    ref = None
    for d in (d1, d2):
        clf.zero_grad(set_to_none=True)
        clf.training_forward(d)[1].backward()
        g = {k: p.grad.clone() for k, p in clf.gnn.named_parameters()}
        ref = g if ref is None else {k: ref[k] + g[k] for k in g}
    assert max(rel_l2(both[k].cpu(), ref[k].cpu()) for k in ref if ref[k].norm() > 0) <= 1e-6


def test_molecule_without_kept_edge_and_full_molecule():
    """Fragment atoms 10 apart (no kept edge but the self loops) beside a 64-fragment-atom molecule; 65 raises."""
    from difflinker_amd.datasets import collate_with_fragment_edges
    data = size_batch([64, 6], [0, 2], IN_NF, seed=8, scale=0.9, chain=True)
    sparse = size_batch([4], [0], IN_NF, seed=9)
    sparse['positions'][0, :4] = torch.tensor([[0.0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]])
    mols = []
    for d in (data, sparse):
        for b in range(d['positions'].shape[0]):
            n = int(d['atom_mask'][b].sum())
            mols.append({'positions': d['positions'][b, :n], 'one_hot': d['one_hot'][b, :n], 'anchors': torch.zeros(n),
                         'fragment_mask': d['fragment_mask'][b, :n, 0], 'linker_mask': d['linker_mask'][b, :n, 0],
                         'num_atoms': n, 'uuid': 0, 'name': 'm'})
    batch = collate_with_fragment_edges(mols)
    for bn in (True, False):
        clf, sd = make_clf(2, bn, seed=713)
        ref_out, _, ref_g, _ = ref_run(sd, batch, 2, bn)
        out, _, g = hip_run(clf, batch)
        overall, worst, _ = compare(g, ref_g, bn)
        print(f'[size grad 64 + edgeless bn={bn}] rel-L2 all {overall:.3e}, worst tensor {worst:.3e}')
        if worst > BAR_TENSOR:
            print({k: f'{rel_l2(g[k], ref_g[k]):.1e}' for k in ref_g if k in g})
        assert rel_l2(out, ref_out) <= 1e-5 and overall <= BAR_ALL and worst <= BAR_TENSOR
    big = size_batch([70], [5], IN_NF, seed=10)
    clf, _ = make_clf(1, True, seed=714)
    with pytest.raises(ValueError, match='fragment atoms'):
        clf.training_forward(to_dev(big))


def test_one_row_with_batch_norm_raises():
    clf, _ = make_clf(1, True, seed=715)
    with pytest.raises(ValueError, match='more than 1 value'):
        clf.training_forward(to_dev(size_batch([1], [0], IN_NF, seed=11)))
    clf0, _ = make_clf(1, False, seed=715)              # without BatchNorm one row is fine
    clf0.training_forward(to_dev(size_batch([1], [0], IN_NF, seed=11)))[1].backward()


def test_eval_forward_refolds_after_optimizer_step():
    clf, _ = make_clf(2, True, seed=716)
    data = to_dev(size_batch([14, 22, 9], [4, 6, 3], IN_NF, seed=12))
    clf.eval()
    before, _ = clf.forward(data, return_loss=False)
    clf.train()
    opt = clf.configure_optimizers()
    clf.training_step(data)['loss'].backward()
    opt.step()
    clf.eval()
    after, _ = clf.forward(data, return_loss=False)
    assert not torch.equal(before, after)
    fresh, _ = make_clf(2, True, seed=716)
    fresh.load_state_dict(clf.state_dict())
    again, _ = fresh.eval().forward(data, return_loss=False)
    assert torch.equal(after, again)


def test_adamw_trajectory_matches_fp64():
    L = 2
    clf, sd = make_clf(L, True, seed=717)
    data = size_batch([16, 11, 25, 8], [5, 3, 8, 2], IN_NF, seed=13)
    opt = clf.configure_optimizers()
    p = {k: v.detach().double().clone().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    leaves = [p['gnn.' + k] for k, _ in clf.gnn.named_parameters()]
    ref_opt = torch.optim.AdamW(leaves, lr=clf.lr, amsgrad=True, weight_decay=1e-12)
    d = lambda k: data[k].double()       # noqa: E731
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        clf.training_step(to_dev(data))['loss'].backward()
        opt.step()
        ref_opt.zero_grad(set_to_none=True)
        out, _ = train_logits(p, d('one_hot'), d('positions'), d('fragment_mask'), d('edge_mask'), L, True)
        torch.nn.functional.cross_entropy(out, true_labels(data['linker_mask'])).backward()
        ref_opt.step()
    # biases right before a BatchNorm have a true gradient of 0: AdamW turns their rounding noise into steps of size lr
    errs = [rel_l2(q.detach().cpu(), p['gnn.' + k].detach()) for k, q in clf.gnn.named_parameters() if not pre_bn_bias(k)]
    print(f'[size adamw] worst parameter rel-L2 after 3 steps {max(errs):.3e}')
    assert max(errs) <= 1e-4


def test_overfit_eight_molecules():
    torch.manual_seed(0)
    clf, _ = make_clf(3, True, seed=718)
    sizes = [12, 18, 9, 22, 15, 27, 11, 20]
    data = to_dev(size_batch(sizes, [3, 4, 5, 6, 7, 8, 9, 10], IN_NF, seed=14))
    opt = clf.configure_optimizers()
    for _ in range(200):
        opt.zero_grad(set_to_none=True)
        clf.training_step(data)['loss'].backward()
        opt.step()
    clf.train()
    logits, _ = clf.training_forward(data)
    acc = float((logits.argmax(-1) == clf.get_true_labels(data['linker_mask'])).float().mean())
    print(f'[size overfit] training accuracy {acc:.3f}')
    assert acc == 1.0


def test_cli_trains_and_generate_uses_checkpoint(tmp_path):
    def mols(k, seed):
        """A learnable task: every atom of a molecule has one type t, and its linker has 3 + t atoms."""
        g = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(k):
            t = int(torch.randint(0, 4, (1,), generator=g))
            nfrag, nl = int(torch.randint(12, 25, (1,), generator=g)), 3 + t
            n = nfrag + nl
            frag = torch.zeros(n)
            frag[:nfrag] = 1
            out.append({'positions': torch.cumsum(0.9 * torch.randn((n, 3), generator=g), 0),
                        'one_hot': torch.nn.functional.one_hot(torch.full((n,), t), 8).float(), 'anchors': torch.zeros(n),
                        'fragment_mask': frag, 'linker_mask': 1 - frag, 'num_atoms': n, 'uuid': 0, 'name': 'm'})
        return out
    torch.save(mols(48, 16), tmp_path / 'zinc_syn_train.pt')
    torch.save(mols(16, 17), tmp_path / 'zinc_syn_val.pt')
    ck = tmp_path / 'ck'
    cmd = [sys.executable, '-m', 'difflinker_amd.train_size_gnn', '--data', str(tmp_path), '--train_data_prefix',
           'zinc_syn_train', '--val_data_prefix', 'zinc_syn_val', '--checkpoints', str(ck), '--max_steps', '50',
           '--batch_size', '16', '--normalization', 'batch_norm', '--loss_weights', '--val_every', '1000']
    proc = subprocess.run(cmd + ['--max_steps', '1'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    first = [json.loads(l) for l in proc.stdout.splitlines() if '"val"' in l][-1]['val']['loss/val']
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    last = [json.loads(l) for l in proc.stdout.splitlines() if '"val"' in l][-1]['val']['loss/val']
    print(f'[size cli] val loss after 1 step {first:.4f}, after 50 {last:.4f}')
    assert last < first
    from difflinker_amd.linker_size import SizeClassifier
    path = str(ck / 'last.ckpt')
    clf = SizeClassifier.load_from_checkpoint(path)
    assert clf.gnn.normalization == 'batch_norm' and clf.loss_weights is not None
    from difflinker_amd.generate import make_sample_fn
    from difflinker_amd.datasets import collate_with_fragment_edges
    batch = to_dev(collate_with_fragment_edges(mols(4, 18)))
    sizes = make_sample_fn(path, DEV)(batch)
    assert sizes.shape == (4,) and int(sizes.min()) >= 3
