"""Timing (GPU box): molecules/s of EDM.forward (the loss / VLB of held-out data) on the C2 geometry (GEOM hparams, 35..50
atoms, synthetic.make_batch) at B = 256 and B = 64.  Per-kernel times of the prologue, the denoiser forward and the
epilogue come from a kernel trace of this script (no counter collection in the same run):

    rocprofv3 --kernel-trace --stats -d OUT -o loss -- python scripts/time_loss.py
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='256,64')
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--noise_source', choices=('philox', 'torch'), default='philox')
a = ap.parse_args()

from difflinker_amd import Dynamics, EDM, synthetic     # noqa: E402

dev = torch.device('cuda:0')
for bs in (int(b) for b in a.batches.split(',')):
    data, cfg = synthetic.make_batch('C2', seed=1, batch=bs, device=dev)
    torch.manual_seed(0)
    dyn = Dynamics(3, cfg['nf'], cfg['ctx'], hidden_nf=128, n_layers=cfg['n_layers'], norm_constant=1e-6).to(dev)
    edm = EDM(dyn, in_node_nf=cfg['nf'], n_dims=3, timesteps=cfg['T'], noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(dev)
    edm.noise_source = a.noise_source
    args = (data['positions'], data['one_hot'], data['atom_mask'], data['fragment_mask'], data['linker_mask'],
            data['edge_mask'], data['fragment_mask'])
    with torch.no_grad():
        for _ in range(a.warmup):
            out = edm(*args)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.iters):
            out = edm(*args)
        ev1.record()
        torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / a.iters
    # the denoiser call alone on the same z_t / t (what EDM.forward adds around it: the two loss kernels + host glue)
    with torch.no_grad():
        x, h = edm.normalize(data['positions'], data['one_hot'])
        z = torch.cat([x, h], 2)
        t = torch.rand((bs, 1), device=dev)
        fwd = dict(xh=z, t=t, node_mask=data['atom_mask'], linker_mask=data['linker_mask'], edge_mask=data['edge_mask'],
                   context=data['fragment_mask'])
        for _ in range(a.warmup):
            dyn.forward(**fwd)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(a.iters):
            dyn.forward(**fwd)
        ev1.record()
        torch.cuda.synchronize()
    ms_fwd = ev0.elapsed_time(ev1) / a.iters
    print(json.dumps({'batch': bs, 'noise_source': a.noise_source, 'ms_per_call': round(ms, 4),
                      'molecules_per_s': round(bs / ms * 1e3, 1), 'forward_only_ms': round(ms_fwd, 4),
                      'added_share': round((ms - ms_fwd) / ms_fwd, 4), 'l2_loss': float(out[4])}))
