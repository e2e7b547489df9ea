"""Launch time of dl_pose_checks: device events around back-to-back launches, after a warm-up.  By default B = 256 random
molecules of at most 50 atoms on N = 50 rows; --pocket times a pocket batch instead: B = 64, N = 292, of which 250 rows are
pocket atoms that drop_mask removes and up to 42 are a ligand."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import pose_checks_ref as pr                    # noqa: E402
import test_gpu_pose_checks as t                # noqa: E402
from difflinker_amd import _lib, const          # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--launches', type=int, default=20000)
p.add_argument('--repeats', type=int, default=5)
p.add_argument('--pocket', action='store_true')
a = p.parse_args()
rng = np.random.default_rng(1)
if a.pocket:
    B, N, n_pocket = 64, 292, 250
    molecules = []
    for _ in range(B):                           # pocket atoms first, unbonded and dropped; the ligand after them
        m = pr.random_molecule(rng, max_atoms=N - n_pocket, min_atoms=20)
        shift = lambda e: (e[0] + n_pocket, e[1] + n_pocket, e[2])      # noqa: E731
        molecules.append(dict(types=[pr.C] * n_pocket + m['types'],
                              points=[tuple(v) for v in rng.normal(0, 8, (n_pocket, 3)).tolist()] + m['points'],
                              entries=[shift(e) for e in m['entries']], planar=[k + n_pocket for k in m['planar']],
                              marked=[k + n_pocket for k in m['marked']], dropped=list(range(n_pocket))))
else:
    B, N = 256, 50
    molecules = [dict(pr.random_molecule(rng, max_atoms=N, min_atoms=10), dropped=[]) for _ in range(B)]
batch = t.batch_of(molecules, N, seed=2)
capacity = batch['bonds'].shape[1]
tables = (const.length_bounds_table(False), const.angle_cos_table(), const.internal_clash_table(False))
held = [t.dev(batch['x']), t.dev(batch['one_hot']), t.dev(batch['node_mask']), t.dev(batch['drop_mask']), t.dev(batch['mark_mask']),
        t.dev(batch['atom_planar'], torch.int32), t.dev(batch['n_bonds_in'], torch.int32), t.dev(batch['bonds'], torch.int32),
        t.dev(batch['status_in'], torch.int32)] + [t.dev(table, torch.float64) for table in tables]
x, one_hot, mask, drop, mark, planar, n_in, bonds, status_in, bounds, cosines, clash = held
i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=t.DEV)      # noqa: E731
counts, flags, status = i32(B, 2, 8), i32(B, N), i32(B)
args = _lib.DLPoseArgs(
    B=B, N=N, nf=8, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(), drop_mask=drop.data_ptr(),
    mark_mask=mark.data_ptr(), atom_planar=planar.data_ptr(), length_bounds2=bounds.data_ptr(), angle_cos=cosines.data_ptr(),
    clash2=clash.data_ptr(), capacity=capacity, n_bonds_in=n_in.data_ptr(), bonds=bonds.data_ptr(), status_in=status_in.data_ptr(),
    counts=counts.data_ptr(), atom_flags=flags.data_ptr(), status=status.data_ptr())
lib = _lib.load()
args.stream = torch.cuda.current_stream(torch.device(t.DEV)).cuda_stream
ref = ctypes.byref(args)
for _ in range(200):
    _lib.check(lib.dl_pose_checks(ref), 'dl_pose_checks')
torch.cuda.synchronize()
kept = (batch['node_mask'] * (1 - batch['drop_mask'])).sum() / B
print('kept atoms per molecule: mean %.1f; per molecule: %s' % (kept, ', '.join(
    '%s %.1f' % (name, v) for name, v in zip(('bonds', 'untabled', 'short', 'long', 'angles', 'bad angles', 'far pairs', 'clashes'),
                                             counts[:, 0].float().mean(dim=0).tolist()))))
times = []
for _ in range(a.repeats):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.launches):
        lib.dl_pose_checks(ref)
    end.record()
    torch.cuda.synchronize()
    times.append(start.elapsed_time(end) * 1e3 / a.launches)
print('B = %d, N = %d: microseconds per launch over %d back-to-back launches, %d repeats: %s; median %.2f' % (
    B, N, a.launches, a.repeats, ' '.join('%.2f' % v for v in times), float(np.median(times))))
