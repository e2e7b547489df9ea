"""Milliseconds per training step of the linker-size predictor (``SizeClassifier.training_forward`` + ``backward`` +
``AdamW.step``) on ZINC-like synthetic batches (fragments of 15..35 atoms, linkers of 3..12, BatchNorm), and the same step
with an eager fp32 restatement (the oracle's GCL with train-mode ``F.batch_norm``) under PyTorch autograd on the same device.

    python scripts/time_size_train_step.py [--steps 10] [--warmup 3] [--configs 64x3,256x5] [--no_eager]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflinker_amd import const                                              # noqa: E402
from difflinker_amd.datasets import collate_with_fragment_edges                # noqa: E402
from difflinker_amd.linker_size import SizeClassifier                          # noqa: E402
from oracle.egnn_oracle import coord2diff, fc_edges, segment_sum               # noqa: E402


def batch(B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    mols = []
    for _ in range(B):
        nfrag = int(torch.randint(15, 36, (1,), generator=g))
        nl = int(torch.randint(3, 13, (1,), generator=g))
        n = nfrag + nl
        frag = torch.zeros(n)
        frag[:nfrag] = 1
        types = torch.randint(0, const.NUMBER_OF_ATOM_TYPES, (n,), generator=g)
        pos = torch.cumsum(torch.randn((n, 3), generator=g) * 0.9, 0)        # chain-like: a few kept edges per atom
        mols.append({'positions': pos, 'one_hot': F.one_hot(types, const.NUMBER_OF_ATOM_TYPES).float(),
                     'anchors': torch.zeros(n), 'fragment_mask': frag, 'linker_mask': 1 - frag, 'num_atoms': n,
                     'uuid': 0, 'name': 'm'})
    d = collate_with_fragment_edges(mols)
    d.pop('edges')
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def eager_loss(gnn, data, labels):
    """SizeClassifier.forward in training mode, eager fp32 (linker_size_lightning.py:83-117)."""
    bs, n = data['positions'].shape[:2]
    fm = data['fragment_mask'].float()
    x = (data['positions'] * fm).reshape(bs * n, -1)
    h = (data['one_hot'] * fm).reshape(bs * n, -1)
    row, col = fc_edges(n, bs, device=x.device)
    dist, _ = coord2diff(x, row, col)
    em = (data['edge_mask'].reshape(-1, 1).bool() & (dist < 6)).float()
    h = gnn.embedding_in(h)
    for gcl in [gnn.gcl1] + list(gnn.gcl_layers):
        m = F.relu(gcl.edge_mlp[0](torch.cat([h[row], h[col], dist], 1)))
        m = F.relu(gcl.edge_mlp[2](m)) * em
        t = torch.cat([h, segment_sum(m, row, h.size(0), 1.0)], 1)
        t = F.relu(gcl.node_mlp[1](gcl.node_mlp[0](t)))
        h = (h + gcl.node_mlp[4](gcl.node_mlp[3](t))) * fm.reshape(-1, 1)
    out = gnn.embedding_out(h).view(bs, n, -1).mean(1)
    return F.cross_entropy(out, labels)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--configs', default='64x3,256x5')
    p.add_argument('--no_eager', action='store_true')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    for cfg in a.configs.split(','):
        B, L = [int(v) for v in cfg.split('x')]
        torch.manual_seed(0)
        clf = SizeClassifier(in_node_nf=const.NUMBER_OF_ATOM_TYPES, hidden_nf=128,
                             out_node_nf=len(const.ZINC_TRAIN_LINKER_ID2SIZE), n_layers=L,
                             normalization='batch_norm').to(dev).train()
        data = batch(B, 1, dev)
        labels = clf.get_true_labels(data['linker_mask'])
        opt = clf.configure_optimizers()

        def hip_step():
            opt.zero_grad(set_to_none=True)
            clf.training_step(data)['loss'].backward()
            opt.step()
        res = {'batch': B, 'n_layers': L, 'n_padded': int(data['positions'].shape[1]),
               'hip_ms_per_step': timed(hip_step, a.steps, a.warmup)}
        if not a.no_eager:
            opt2 = torch.optim.AdamW(clf.gnn.parameters(), lr=clf.lr, amsgrad=True, weight_decay=1e-12)

            def eager_step():
                opt2.zero_grad(set_to_none=True)
                eager_loss(clf.gnn, data, labels).backward()
                opt2.step()
            res['eager_autograd_ms_per_step'] = timed(eager_step, a.steps, a.warmup)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
