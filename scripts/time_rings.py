"""Launch time of ring perception (csrc/rings.hip) at its use: the bond lists ``dl_perceive_bonds`` leaves on the device for a
batch of molecules; beside it, the same outputs as ``tests/rings_ref.py`` computes them in plain Python on the host.

    python scripts/time_rings.py
    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_rings.py --reps 50 --host 0

256 molecules of 50 carbon atoms, laid out as drug-like data-set molecules are: five- and six-membered rings and short
chains joined by single bonds (1.5 A sides, a little jitter, a random rotation each), the last 12 atoms taken as the
linker.  The bonds are perceived on the GPU first; the timed call is ``metrics.ring_scores`` on that result (launch + output
allocation); the kernel's own time is the profiler's ``ring_scores_kernel`` row."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import rings_ref                                                  # noqa: E402
from difflinker_amd import const                                  # noqa: E402
from difflinker_amd.metrics import ring_scores                    # noqa: E402
from difflinker_amd.molecule_builder import perceive_all_bonds    # noqa: E402

B, N_ATOMS, N_LINKER, SIDE = 256, 50, 12, 1.5
NF = const.GEOM_NUMBER_OF_ATOM_TYPES


def molecule(rng):
    """Rings and chains strung along x: each unit starts one bond to the right of the last unit's rightmost atom."""
    atoms, at = [], np.zeros(3)
    while len(atoms) < N_ATOMS:
        k = int(rng.choice([0, 5, 6], p=[0.4, 0.2, 0.4]))
        if k:                                                             # a k-ring whose leftmost vertex is `at`
            radius = SIDE / (2 * np.sin(np.pi / k))
            angle = np.pi + 2 * np.pi * np.arange(k) / k
            unit = at + np.stack([radius + radius * np.cos(angle), radius * np.sin(angle), np.zeros(k)], 1)
        else:                                                             # a zigzag chain of one to three atoms
            n = int(rng.integers(1, 4))
            unit = at + np.stack([1.3 * np.arange(n), 0.75 * (np.arange(n) % 2), np.zeros(n)], 1)
        atoms += list(unit)
        at = unit[np.argmax(unit[:, 0])] + np.array([SIDE, 0.0, 0.0])
    x = np.array(atoms[:N_ATOMS]) + rng.normal(0, 0.02, size=(N_ATOMS, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return (x - x.mean(0)) @ q.T


def batch(seed=0):
    rng = np.random.default_rng(seed)
    x = np.stack([molecule(rng) for _ in range(B)]).astype(np.float32)
    types = np.zeros((B, N_ATOMS), dtype=np.int64)                        # carbon: every 1.5 A side is a single bond
    linker = np.zeros((B, N_ATOMS), np.float32)
    linker[:, -N_LINKER:] = 1
    return x, np.eye(NF, dtype=np.float32)[types], np.ones((B, N_ATOMS), np.float32), linker


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
    found = perceive_all_bonds(dh, dx, dm, True)
    got, t_call = timed(lambda: ring_scores(dm, found, None, dl), a.reps)
    assert int(got.status.max()) == 0
    print(f'B={B} molecules of {N_ATOMS} atoms, {found.n_bonds.double().mean().item():.1f} bonds and '
          f'{got.n_rings.double().mean().item():.2f} rings each (capacity {found.bonds.shape[1]}): ring_scores '
          f'{t_call:.1f} us per call (device events, {a.reps} calls)', flush=True)
    if a.host:
        lists = (mask, found.bonds.cpu().numpy(), found.n_bonds.cpu().numpy(), found.status.cpu().numpy())
        t0 = time.perf_counter()
        want = rings_ref.ring_scores(*lists, mark_mask=linker)
        t_host = time.perf_counter() - t0
        same = all(np.array_equal(getattr(got, name).cpu().numpy(), want[name]) for name in rings_ref.FIELDS)
        print(f'tests/rings_ref.py on the host: {t_host * 1e3:.1f} ms for the batch ({t_host / B * 1e6:.0f} us per molecule); '
              f'outputs agree: {same}', flush=True)


if __name__ == '__main__':
    main()
