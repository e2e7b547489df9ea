"""Time of one molecule_builder.relax_samples call (perceive_bonds, refine_bond_orders, dl_relax_molecules) and of the relax
launch alone: device events around back-to-back calls, after a warm-up.  By default the benchmark's shape: B = 256 random
molecules of at most 50 atoms on N = 50 rows, about a third of the atoms marked as the linker; --pocket times a pocket batch
instead: B = 64, N = 292, of which 250 rows are pocket atoms (dropped: the wall) and up to 42 are a ligand."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import pose_checks_ref as pr                    # noqa: E402
import relax_ref as rr                          # noqa: E402
from difflinker_amd import molecule_builder as mb   # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--calls', type=int, default=50)
p.add_argument('--repeats', type=int, default=5)
p.add_argument('--steps', type=int, default=200)
p.add_argument('--pocket', action='store_true')
a = p.parse_args()
DEV = 'cuda:0'
rng = np.random.default_rng(1)
if a.pocket:
    B, N, n_pocket = 64, 292, 250
    molecules = []
    for _ in range(B):                           # pocket atoms first, unbonded and dropped; the ligand after them
        m = pr.random_molecule(rng, max_atoms=N - n_pocket, min_atoms=20)
        molecules.append(dict(types=[pr.C] * n_pocket + m['types'],
                              points=[tuple(v) for v in rng.normal(0, 8, (n_pocket, 3)).tolist()] + m['points'], entries=[],
                              planar=[], marked=[k + n_pocket for k in m['marked']], dropped=list(range(n_pocket))))
else:
    B, N = 256, 50
    molecules = [dict(pr.random_molecule(rng, max_atoms=N, min_atoms=10), dropped=[], entries=[]) for _ in range(B)]
batch = rr.batch_of(molecules, N, seed=2)
one_hot, x, mask, mark, drop = (torch.as_tensor(batch[k]).to(DEV) for k in ('one_hot', 'x', 'node_mask', 'mark_mask', 'drop_mask'))


def whole():
    return mb.relax_samples(one_hot, x, mask, False, mark, drop_mask=drop, steps=a.steps)


found = mb.perceive_bonds(one_hot, x, mask, False)
refined, aromatic = mb.refine_bond_orders(found, one_hot, x, mask, False, drop, mark)
refined = refined._replace(status=aromatic.status)


def alone():
    return mb.relax(refined, one_hot, x, mask, False, mark, drop, aromatic.atom_aromatic, aromatic.bond_aromatic, steps=a.steps)


for _ in range(5):
    out = whole()
    alone()
torch.cuda.synchronize()
movable = float((batch['node_mask'] * (1 - batch['drop_mask']) * batch['mark_mask']).sum() / B)
print('B = %d, N = %d, %d steps asked: movable atoms per molecule %.1f, steps done mean %.1f (min %d, max %d), status != 0: %d' % (
    B, N, a.steps, movable, float(out.steps_done.float().mean()), int(out.steps_done.min()), int(out.steps_done.max()),
    int((out.status != 0).sum())))
for name, call in (('relax_samples (three launches)', whole), ('relax alone (one launch)', alone)):
    times = []
    for _ in range(a.repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            call()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / a.calls)
    print('%s: milliseconds per call over %d back-to-back calls, %d repeats: %s; median %.3f' % (
        name, a.calls, a.repeats, ' '.join('%.3f' % v for v in times), float(np.median(times))))
