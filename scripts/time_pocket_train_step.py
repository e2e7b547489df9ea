"""Milliseconds per training step of the pocket-conditioned model (``training_forward`` + ``backward`` + ``AdamW.step``) at
the C4 geometry (``synthetic.CONFIGS['C4']``: 30 fragment, 250 pocket, 6..12 linker atoms, graph FC-10A-4A, 6 blocks x 2
sublayers, hidden 128) on a synthetic batch of B complexes (16: the batch of pockets_difflinker_full_no_anchors_fc.yml), and
two baselines on the same device:
  (a) the same parameter gradient through ``dl_egnn_backward_fc`` with the radius graph handed over as a dense 0/1 int8
      mask (what the tree could do before the edge-list backward): every one of the N^2 pairs, one compute unit per molecule;
  (b) the same step with the oracle port (``oracle.egnn_oracle``) under eager PyTorch fp32 autograd.

    python scripts/time_pocket_train_step.py [--batch 16] [--steps 5] [--warmup 2] [--no_dense] [--no_eager]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflinker_amd import Dynamics, DynamicsWithPockets, EDM, synthetic      # noqa: E402
from oracle import egnn_oracle                                                 # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--layers', type=int, default=6)
    p.add_argument('--no_dense', action='store_true')
    p.add_argument('--no_eager', action='store_true')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    data, c = synthetic.make_batch('C4', seed=0, batch=a.batch)
    inp = synthetic.sampler_inputs(data, pockets=True)
    nf, ctx, L, S, graph = c['nf'], c['ctx'], a.layers, 2, c['graph_type']
    B, N = inp['x'].shape[:2]
    g = {k: v.to(dev) for k, v in inp.items()}
    torch.manual_seed(0)
    kw = dict(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, inv_sublayers=S, norm_constant=1e-6,
              normalization_factor=100)
    dyn = DynamicsWithPockets(graph_type=graph, **kw).to(dev)
    edm = EDM(dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(dev)
    opt = torch.optim.AdamW(edm.parameters(), lr=2e-4, amsgrad=True, weight_decay=1e-12)
    args = (g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'])

    def hip_step():
        out = edm.training_forward(*args)
        opt.zero_grad(set_to_none=True)
        out[4].backward()
        opt.step()

    def timed(fn, steps=a.steps, warmup=a.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    # the graph of one z_t: its edge count, and the dense mask of baseline (a)
    cfg = egnn_oracle.EGNNConfig(in_node_nf=nf, context_node_nf=ctx, n_layers=L, inv_sublayers=S, norm_constant=1e-6,
                                 normalization_factor=100, graph_type=graph)
    gen = torch.Generator().manual_seed(1)
    z = (torch.cat([inp['x'], inp['h'] / 4], -1) * inp['fragment_mask']
         + torch.randn(B, N, 3 + nf, generator=gen) * inp['linker_mask'])
    t = torch.rand(B, 1, generator=gen)
    G = torch.randn(B, N, 3 + nf, generator=gen)
    flat = lambda v: v.reshape(B * N, -1)                                                   # noqa: E731
    row, col = egnn_oracle.pocket_edges(cfg, flat(z[..., :3] * inp['node_mask']), flat(inp['node_mask']), inp['edge_mask'].view(-1),
                                        flat(inp['linker_mask']), flat(inp['context'][..., -2]), flat(inp['context'][..., -1]))
    res = {'batch': B, 'n_padded': N, 'layers': L, 'edges': int(row.numel()), 'pairs_dense': B * N * N,
           'hip_ms_per_step': timed(hip_step)}
    with torch.no_grad():
        res['hip_loss_forward_ms'] = timed(lambda: edm(*args))
    on = lambda v: v.to(dev)                                                                # noqa: E731
    bargs = (on(t), on(z), g['node_mask'], g['linker_mask'])
    res['hip_backward_ms'] = timed(lambda: dyn.parameter_grad(*bargs, g['edge_mask'], g['context'], on(G)))
    if not a.no_dense:
        mask = torch.zeros(B * N, B * N, dtype=torch.int8)
        mask[row, col] = 1
        dense = torch.stack([mask[b * N:(b + 1) * N, b * N:(b + 1) * N] for b in range(B)]).to(dev)
        fc = Dynamics(**kw).to(dev)
        fc.load_state_dict(dyn.state_dict())
        res['dense_mask_fc_backward_ms'] = timed(lambda: fc.parameter_grad(*bargs, dense, g['context'], on(G)), steps=2, warmup=1)
        res['speedup_over_dense_mask'] = res['dense_mask_fc_backward_ms'] / res['hip_backward_ms']
        a_, b_ = dyn.parameter_grad(*bargs, g['edge_mask'], g['context'], on(G)), fc.parameter_grad(*bargs, dense, g['context'], on(G))
        num = sum(float(((u.double() - v.double()) ** 2).sum()) for u, v in zip(a_, b_))
        den = sum(float((v.double() ** 2).sum()) for v in b_)
        res['rel_l2_against_dense_mask'] = (num / den) ** 0.5
    if not a.no_eager:
        params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in dyn.state_dict().items()}
        eopt = torch.optim.AdamW(params.values(), lr=2e-4, amsgrad=True, weight_decay=1e-12)
        lm = g['linker_mask']

        def eager_step():
            tt = torch.rand(B, 1, device=dev)
            eps = torch.randn(B, N, 3 + nf, device=dev) * lm
            zz = torch.cat([g['x'], g['h'] / 4], -1) * g['fragment_mask'] + eps
            eps_hat = egnn_oracle.dynamics_forward_pockets(params, cfg, tt, zz, g['node_mask'], lm, g['edge_mask'],
                                                           g['context']) * lm
            loss = (((eps - eps_hat) ** 2).sum((1, 2)) / ((3 + nf) * lm.sum((1, 2)))).mean()
            eopt.zero_grad(set_to_none=True)
            loss.backward()
            eopt.step()
        res['eager_autograd_ms_per_step'] = timed(eager_step)
        res['hip_over_eager'] = res['hip_ms_per_step'] / res['eager_autograd_ms_per_step']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
