"""Launch time of dl_add_hydrogens at B = 256, N = 50: device events around back-to-back launches, after a warm-up."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import hydrogens_ref as hr                      # noqa: E402
import test_gpu_hydrogens as t                  # noqa: E402
from difflinker_amd import _lib                 # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--launches', type=int, default=20000)
p.add_argument('--repeats', type=int, default=5)
a = p.parse_args()
rng = np.random.default_rng(1)
molecules, _ = hr.random_molecules(rng, 256, max_atoms=50, with_drop=lambda b: False)
batch = t.pack(molecules, 50, rng=rng)
B, N = batch['mask'].shape
capacity, Hcap = batch['bonds'].shape[1], 4 * N
valence, length = hr.tables()
held = [t.dev(batch['x']), t.dev(batch['one_hot']), t.dev(batch['mask']), t.dev(batch['planar'], torch.int32),
        t.dev(valence, torch.int32), t.dev(length, torch.float64), t.dev(batch['n_in'], torch.int32),
        t.dev(batch['bonds'], torch.int32), t.dev(batch['status'], torch.int32)]
x, one_hot, mask, planar, valence_t, length_t, n_in, bonds, status_in = held
i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=t.DEV)      # noqa: E731
n_h, h_count, h_parent, status = i32(B), i32(B, N), i32(B, Hcap), i32(B)
h_x = torch.zeros((B, Hcap, 3), dtype=torch.float64, device=t.DEV)
args = _lib.DLHydrogensArgs(
    B=B, N=N, nf=8, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(), drop_mask=None,
    atom_planar=planar.data_ptr(), default_valence=valence_t.data_ptr(), xh_length=length_t.data_ptr(), capacity=capacity,
    n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr(), status_in=status_in.data_ptr(), Hcap=Hcap, n_h=n_h.data_ptr(),
    h_count=h_count.data_ptr(), h_parent=h_parent.data_ptr(), h_x=h_x.data_ptr(), status=status.data_ptr())
lib = _lib.load()
args.stream = torch.cuda.current_stream(torch.device(t.DEV)).cuda_stream
ref = ctypes.byref(args)
for _ in range(200):
    _lib.check(lib.dl_add_hydrogens(ref), 'dl_add_hydrogens')
torch.cuda.synchronize()
print('atoms per molecule: mean %.1f; hydrogens per molecule: mean %.1f' % (batch['mask'].sum() / B, float(n_h.float().mean())))
times = []
for _ in range(a.repeats):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.launches):
        lib.dl_add_hydrogens(ref)
    end.record()
    torch.cuda.synchronize()
    times.append(start.elapsed_time(end) * 1e3 / a.launches)
print('B = %d, N = %d: microseconds per launch over %d back-to-back launches, %d repeats: %s; median %.2f' % (
    B, N, a.launches, a.repeats, ' '.join('%.2f' % v for v in times), float(np.median(times))))
