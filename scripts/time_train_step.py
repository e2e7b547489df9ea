"""Milliseconds per training step (``training_forward`` + ``backward`` + ``AdamW.step``) at the GEOM configuration
(configs/geom_difflinker.yml: 6 blocks, 2 sublayers, hidden 128, one context channel) on a synthetic ragged batch of
B molecules of about N atoms, and the same step with the oracle port (``oracle.egnn_oracle``, the eager baseline of
``bench.py --full``) under eager PyTorch autograd on the same device.

    python scripts/time_train_step.py [--batch 64] [--atoms 50] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflinker_amd import Dynamics, EDM                                       # noqa: E402
from difflinker_amd.const import GEOM_NUMBER_OF_ATOM_TYPES                     # noqa: E402
from difflinker_amd.datasets import collate                                    # noqa: E402
from oracle import egnn_oracle                                                 # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--atoms', type=int, default=50)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--no_eager', action='store_true')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    nf, ctx, L, S = GEOM_NUMBER_OF_ATOM_TYPES, 1, 6, 2
    g = torch.Generator().manual_seed(0)
    mols = []
    for _ in range(a.batch):
        n = int(torch.randint(a.atoms - 15, a.atoms + 16, (1,), generator=g))
        nl = max(2, n // 5)
        frag = torch.zeros(n)
        frag[:n - nl] = 1
        mols.append({'positions': 2.0 * torch.randn((n, 3), generator=g),
                     'one_hot': torch.nn.functional.one_hot(torch.randint(0, nf, (n,), generator=g), nf).float(),
                     'anchors': torch.zeros(n), 'fragment_mask': frag, 'linker_mask': 1 - frag, 'num_atoms': n})
    b = {k: v.to(dev) for k, v in collate(mols).items() if torch.is_tensor(v)}
    torch.manual_seed(0)
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, inv_sublayers=S,
                   norm_constant=1e-6, normalization_factor=100).to(dev)
    edm = EDM(dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(dev)
    opt = torch.optim.AdamW(edm.parameters(), lr=2e-4, amsgrad=True, weight_decay=1e-12)
    args = (b['positions'], b['one_hot'], b['atom_mask'], b['fragment_mask'], b['linker_mask'], b['edge_mask'],
            b['fragment_mask'])

    def hip_step():
        out = edm.training_forward(*args)
        opt.zero_grad(set_to_none=True)
        out[4].backward()
        opt.step()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    res = {'batch': a.batch, 'n_padded': int(b['positions'].shape[1]), 'hip_ms_per_step': timed(hip_step)}
    # the pieces: forward-only loss, and the weight re-pack the next forward pays after a step
    with torch.no_grad():
        res['hip_loss_forward_ms'] = timed(lambda: edm(*args))
    res['repack_ms'] = timed(lambda: (dyn.invalidate_packed(), dyn.hip_model(dev)))
    if not a.no_eager:
        cfg = egnn_oracle.EGNNConfig(in_node_nf=nf, context_node_nf=ctx, n_layers=L, inv_sublayers=S, norm_constant=1e-6,
                                     normalization_factor=100)
        params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in dyn.state_dict().items()}
        eopt = torch.optim.AdamW(params.values(), lr=2e-4, amsgrad=True, weight_decay=1e-12)
        B, N = b['positions'].shape[:2]
        lm = b['linker_mask']

        def eager_step():
            t = torch.rand(B, 1, device=dev)
            eps = torch.randn(B, N, 3 + nf, device=dev) * lm
            z = torch.cat([b['positions'], b['one_hot'] / 4], -1) * b['fragment_mask'] + eps
            eps_hat = egnn_oracle.dynamics_forward(params, cfg, t, z, b['atom_mask'], lm, b['edge_mask'],
                                                   b['fragment_mask']) * lm
            loss = (((eps - eps_hat) ** 2).sum((1, 2)) / ((3 + nf) * lm.sum((1, 2)))).mean()
            eopt.zero_grad(set_to_none=True)
            loss.backward()
            eopt.step()
        res['eager_autograd_ms_per_step'] = timed(eager_step)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
