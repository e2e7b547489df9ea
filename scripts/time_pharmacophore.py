"""Launch time of dl_pharmacophore_features: device events around back-to-back launches, after a warm-up.  B = 256 fuzz
molecules of tests/test_gpu_pharmacophore.py (two to four hand-built molecules joined, at most 44 atoms, a few of them
pocket atoms that drop_mask removes) on N = 50 rows, the linker half marked."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import pharmacophore_ref as pr                  # noqa: E402
import test_gpu_pharmacophore as t              # noqa: E402
from difflinker_amd import _lib                 # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--launches', type=int, default=20000)
p.add_argument('--repeats', type=int, default=5)
a = p.parse_args()
B, N, Fcap = 256, 50, 96
batch, drop, mark, _ = t.build_fuzz(seed=1, B=B, N=N)
capacity = batch['bonds'].shape[1]
held = [t.dev(batch['x']), t.dev(batch['one_hot']), t.dev(batch['node_mask']), t.dev(drop), t.dev(mark),
        t.dev(batch['n_bonds_in'], torch.int32), t.dev(batch['bonds'], torch.int32), t.dev(batch['bond_aromatic'], torch.int32),
        t.dev(batch['status_in'], torch.int32), *t.tables()]
x, one_hot, mask, drop_d, mark_d, n_in, bonds, aromatic, status_in, classes, valences = held
i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=t.DEV)      # noqa: E731
family, anchor, marked, n_features, family_count, status = i32(B, Fcap), i32(B, Fcap), i32(B, Fcap), i32(B), i32(B, pr.FAMILIES), i32(B)
position = torch.zeros((B, Fcap, 3), dtype=torch.float32, device=t.DEV)
args = _lib.DLPharmArgs(
    B=B, N=N, nf=batch['one_hot'].shape[2], x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
    drop_mask=drop_d.data_ptr(), mark_mask=mark_d.data_ptr(), feature_class=classes.data_ptr(), default_valence=valences.data_ptr(),
    capacity=capacity, n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr(), bond_aromatic=aromatic.data_ptr(),
    status_in=status_in.data_ptr(), Fcap=Fcap, family=family.data_ptr(), anchor=anchor.data_ptr(), position=position.data_ptr(),
    marked=marked.data_ptr(), n_features=n_features.data_ptr(), family_count=family_count.data_ptr(), status=status.data_ptr())
lib = _lib.load()
args.stream = torch.cuda.current_stream(torch.device(t.DEV)).cuda_stream
ref = ctypes.byref(args)
for _ in range(200):
    _lib.check(lib.dl_pharmacophore_features(ref), 'dl_pharmacophore_features')
torch.cuda.synchronize()
kept = (batch['node_mask'] * (1 - drop)).sum() / B
print('kept atoms per molecule: mean %.1f; features per molecule: mean %.1f; by family: %s; molecules with a status bit: %d' % (
    kept, n_features.float().mean(), ' '.join('%.1f' % v for v in family_count.float().mean(dim=0).tolist()), int((status != 0).sum())))
times = []
for _ in range(a.repeats):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.launches):
        lib.dl_pharmacophore_features(ref)
    end.record()
    torch.cuda.synchronize()
    times.append(start.elapsed_time(end) * 1e3 / a.launches)
print('B = %d, N = %d: microseconds per launch over %d back-to-back launches, %d repeats: %s; median %.2f' % (
    B, N, a.launches, a.repeats, ' '.join('%.2f' % v for v in times), float(np.median(times))))
