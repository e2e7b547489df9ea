"""Time of one dl_canonical_ranks launch against one dl_molecule_keys launch on the same batch (the same refinement, run
once): device events around back-to-back calls, after a warm-up.  The benchmark's batch shape: B = 256 molecules of 35..50
atoms on N = 50 rows.  By default connected molecule-like graphs (tests/canon_cases.random_graph: a random tree with up to
three ring bonds) handed over as a bond list; --geometry takes the random 3D molecules of tests/pose_checks_ref.py instead and
perceives their bonds on the device: atoms piled on one another, about eight pieces per molecule, many of them single atoms
of one element - the case the leaf budget is for."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import canon_cases as cc                        # noqa: E402
import pose_checks_ref as pr                    # noqa: E402
import relax_ref as rr                          # noqa: E402
import test_gpu_canon as tc                     # noqa: E402
from difflinker_amd import _lib, metrics, molecule_builder as mb   # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--calls', type=int, default=50)
p.add_argument('--repeats', type=int, default=5)
p.add_argument('--max_leaves', type=int, default=256)
p.add_argument('--geometry', action='store_true')
a = p.parse_args()
DEV = 'cuda:0'
rng = np.random.default_rng(1)
B, N = 256, 50
if a.geometry:
    molecules = [dict(pr.random_molecule(rng, max_atoms=N, min_atoms=35), dropped=[], entries=[]) for _ in range(B)]
    batch = rr.batch_of(molecules, N, seed=2)
    one_hot, x, mask = (torch.as_tensor(batch[k]).to(DEV) for k in ('one_hot', 'x', 'node_mask'))
    found = mb.perceive_all_bonds(one_hot, x, mask, False)
else:
    graphs = [tc.molecule(*cc.random_graph(seed, 35, 50)) for seed in range(B)]
    one_hot, mask, _, found = tc.batch_of(graphs, N)
    one_hot, mask, found = one_hot.to(DEV), mask.to(DEV), tc.on_device(found)
    pieces = torch.ones(B, dtype=torch.int32, device=DEV)                    # connected by construction; valences are not read
    found = found._replace(n_components=pieces)


def keys():
    return metrics.molecule_keys(one_hot, mask, found, False)


def canon():
    return metrics.canonical_ranks(one_hot, mask, found, False, max_leaves=a.max_leaves)


for _ in range(5):
    k, c = keys(), canon()
torch.cuda.synchronize()
leaves = c['n_leaves'].float()
budget = float(((c['status'] & _lib.DL_CANON_BUDGET) != 0).float().mean())
print('B = %d, N = %d: atoms per molecule %.1f (min %d, max %d), bonds per molecule %.1f, pieces per molecule %.2f' % (
    B, N, float(k.n_atoms.float().mean()), int(k.n_atoms.min()), int(k.n_atoms.max()), float(k.n_bonds.float().mean()),
    float(k.n_components.float().mean())))
print('n_leaves mean %.2f, max %d; DL_CANON_BUDGET share %.4f; status other than the budget bit != 0: %d; distinct codes %d, distinct keys %d' % (
    float(leaves.mean()), int(leaves.max()), budget, int(((c['status'] & ~_lib.DL_CANON_BUDGET) != 0).sum()),
    len(set(c['code'].tolist())), len(set(k.key.tolist()))))
medians = {}
for name, call in (('dl_molecule_keys', keys), ('dl_canonical_ranks', canon)):
    times = []
    for _ in range(a.repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            call()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / a.calls)
    medians[name] = float(np.median(times))
    print('%s: milliseconds per call over %d back-to-back calls, %d repeats: %s; median %.3f' % (
        name, a.calls, a.repeats, ' '.join('%.3f' % v for v in times), medians[name]))
print('ratio %.1f; per leaf of the slowest molecule (max n_leaves): %.1f microseconds' % (
    medians['dl_canonical_ranks'] / medians['dl_molecule_keys'], 1000 * medians['dl_canonical_ranks'] / float(leaves.max())))
