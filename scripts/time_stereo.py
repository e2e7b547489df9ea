"""Time of one dl_stereo_perceive launch beside the numpy restatement of the same batch (tests/stereo_ref.py): device events
around back-to-back calls, after a warm-up.  The benchmark's batch shape: B = 256 molecules of 35..50 atoms on N = 50 rows, the
random 3D molecules of tests/stereo_ref.py with their bond lists handed over."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import stereo_ref as sr                         # noqa: E402
from difflinker_amd import metrics              # noqa: E402
from difflinker_amd.molecule_builder import Bonds   # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--calls', type=int, default=50)
p.add_argument('--repeats', type=int, default=5)
a = p.parse_args()
DEV = 'cuda:0'
rng = np.random.default_rng(1)
B, N = 256, 50
molecules = [sr.random_molecule(rng, max_atoms=N, min_atoms=35) for _ in range(B)]
batch = sr.as_batch(molecules, N, rng=np.random.default_rng(2))
t = lambda name, dtype=torch.float32: torch.as_tensor(batch[name]).to(device=DEV, dtype=dtype).contiguous()      # noqa: E731
one_hot, x, mask, drop, mark = t('one_hot'), t('x'), t('node_mask'), t('drop_mask'), t('mark_mask')
planar, aromatic = t('atom_planar', torch.int32), t('bond_aromatic', torch.int32)
found = Bonds(t('n_bonds_in', torch.int32), t('bonds', torch.int32), None, None, None, torch.zeros(B, dtype=torch.int32, device=DEV))


def stereo():
    return metrics.stereo(one_hot, x, mask, found, True, drop, mark, planar, aromatic)


for _ in range(5):
    out = stereo()
torch.cuda.synchronize()
start = time.perf_counter()
want = sr.perceive(batch['x'], batch['one_hot'], batch['node_mask'], batch['bonds'], batch['n_bonds_in'], drop_mask=batch['drop_mask'],
                   mark_mask=batch['mark_mask'], atom_planar=batch['atom_planar'], bond_aromatic=batch['bond_aromatic'])
host_ms = 1000 * (time.perf_counter() - start)
same = all(out[name].cpu().numpy().tobytes() == want[name].tobytes() for name in sr.FIELDS)
counts = out['counts'][:, 0].sum(dim=0).tolist()
print('B = %d, N = %d: kept atoms per molecule %.1f, list entries per molecule %.1f; centres %d + %d undetermined, double bonds '
      '%d + %d undetermined; every output bit equal to the restatement: %s' % (
          B, N, float((out['atom_class'] >= 0).sum(dim=1).float().mean()), float(batch['n_bonds_in'].mean()), counts[0], counts[1],
          counts[2], counts[3], same))
times = []
for _ in range(a.repeats):
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(a.calls):
        stereo()
    end.record()
    torch.cuda.synchronize()
    times.append(begin.elapsed_time(end) / a.calls)
print('dl_stereo_perceive (through metrics.stereo): milliseconds per call over %d back-to-back calls, %d repeats: %s; median %.3f' % (
    a.calls, a.repeats, ' '.join('%.3f' % v for v in times), float(np.median(times))))
print('tests/stereo_ref.py on the same batch, one pass on the host: %.0f ms' % host_ms)
