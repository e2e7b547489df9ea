"""Launch time of aromatic-ring perception (csrc/aromatic.hip) at its use: after ``dl_perceive_bonds`` on a batch of
molecules, beside the two launches the metrics path already makes for them - bonds and rings; and the same outputs as
``tests/aromatic_ref.py`` computes them in plain Python on the host.

    python scripts/time_aromatic.py
    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_aromatic.py --reps 50 --host 0

256 molecules of 20 to 40 heavy atoms, laid out as drug-like molecules are: one to three fused systems of planar five- and
six-rings (1.39 A sides, C with some N, O and S, 0.03 A of jitter per atom) with substituents, strung along x 1.5 A apart
and filled up with a zigzag chain, a random rotation each.  The bonds are perceived on the GPU from the geometry; the timed
calls are ``perceive_bonds``, ``metrics.ring_scores`` and ``molecule_builder.refine_bond_orders`` on that result (launch +
output allocation each); the kernels' own times are the profiler's rows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import aromatic_ref                                                         # noqa: E402
from difflinker_amd import const                                            # noqa: E402
from difflinker_amd.metrics import ring_scores                              # noqa: E402
from difflinker_amd.molecule_builder import perceive_bonds, refine_bond_orders    # noqa: E402

B, N_MIN, N_MAX, LINK = 256, 20, 40, 1.5
NF = const.NUMBER_OF_ATOM_TYPES


def molecule(rng):
    """``(types, points)`` of ``N_MIN`` to ``N_MAX`` atoms: fused systems along x, then a chain."""
    n = int(rng.integers(N_MIN, N_MAX + 1))
    units = int(rng.integers(1, 4))
    types, points, right = [], [], 0.0
    for _ in range(units):
        t, p, _ = aromatic_ref.random_fused(rng, max_atoms=max(n // units, 8))
        if len(types) + len(t) > n:
            break
        p = np.asarray(p)
        p[:, 0] += right - p[:, 0].min() + (LINK if types else 0.0)
        p[:, 1] -= p[np.argmin(p[:, 0]), 1]                                 # the leftmost atom on the x axis, where the link ends
        types += t
        points += list(p)
        right = max(q[0] for q in points)
    while len(types) < n:                                                   # a zigzag chain of carbons
        k = len(types)
        right += 1.3
        points.append(np.array([right, 0.75 * (k % 2), 0.0]) + rng.normal(0, 0.03, 3))
        types.append(aromatic_ref.C)
    x = np.asarray(points)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return types, (x - x.mean(0)) @ q.T


def batch(seed=0):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, N_MAX, 3), np.float32)
    types = np.zeros((B, N_MAX), np.int64)
    mask = np.zeros((B, N_MAX), np.float32)
    for b in range(B):
        t, p = molecule(rng)
        x[b, :len(t)], types[b, :len(t)], mask[b, :len(t)] = p, t, 1
    linker = mask * (np.arange(N_MAX)[None, :] < 12)
    return x, np.eye(NF, dtype=np.float32)[types] * mask[:, :, None], mask, linker.astype(np.float32)


def timed(fn, reps):
    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1) / reps * 1e3


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--host', type=int, default=1, help='0: skip the plain-Python run on the host')
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    x, one_hot, mask, linker = batch()
    dx, dh, dm, dl = (torch.from_numpy(v).cuda() for v in (x, one_hot, mask, linker))
    found, t_bonds = timed(lambda: perceive_bonds(dh, dx, dm, False), a.reps)
    assert int(found.status.max()) == 0
    rings, t_rings = timed(lambda: ring_scores(dm, found, None, dl), a.reps)
    (refined, aromatic), t_arom = timed(lambda: refine_bond_orders(found, dh, dx, dm, False, mark_mask=dl), a.reps)
    both, t_both = timed(lambda: refine_bond_orders(perceive_bonds(dh, dx, dm, False), dh, dx, dm, False, mark_mask=dl), a.reps)
    old, t_old = timed(lambda: ring_scores(dm, perceive_bonds(dh, dx, dm, False), None, dl), a.reps)
    print(f'B={B} molecules of {mask.sum(1).mean():.1f} atoms, {found.n_bonds.double().mean().item():.1f} bonds, '
          f'{rings.n_rings.double().mean().item():.2f} rings, {aromatic.n_planar_rings.double().mean().item():.2f} planar and '
          f'{aromatic.n_aromatic_rings.double().mean().item():.2f} aromatic rings each (capacity {found.bonds.shape[1]}; status bits '
          f'{int(aromatic.status.max())})', flush=True)
    print(f'per call (device events, {a.reps} calls): perceive_bonds {t_bonds:.1f} us, ring_scores {t_rings:.1f} us, '
          f'refine_bond_orders {t_arom:.1f} us; bonds + aromatic {t_both:.1f} us against bonds + rings {t_old:.1f} us', flush=True)
    if a.host:
        lists = (x, one_hot, mask, found.bonds.cpu().numpy(), found.n_bonds.cpu().numpy(),
                 aromatic_ref.ring_class_table(const.ATOM2IDX), found.status.cpu().numpy())
        t0 = time.perf_counter()
        want = aromatic_ref.aromatic_rings(*lists, mark_mask=linker)
        t_host = time.perf_counter() - t0
        got = dict(aromatic._asdict(), order_out=refined.bonds[:, :, 2], valence_out=refined.valence)
        same = all(np.array_equal(got[name].cpu().numpy(), want[name]) for name in aromatic_ref.FIELDS)
        print(f'tests/aromatic_ref.py on the host: {t_host * 1e3:.1f} ms for the batch ({t_host / B * 1e6:.0f} us per molecule); '
              f'outputs agree: {same}', flush=True)


if __name__ == '__main__':
    main()
