"""Launch time of the symmetry-aware RMSD (csrc/rmsd.hip) at its two ends: many pairs with one map each, and few pairs
with thousands of maps.

    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_rmsd.py

Structures are random chains with 1.1 .. 1.7 A steps; the second of a pair is a rotated, shifted and slightly noisy copy.
Maps are random permutations (the kernel's work does not depend on what a map says) with the identity last.  Prints the
device-event time per launch (launch + output allocation); the kernel's own time is the profiler's `best_rmsd_kernel` row."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difflinker_amd.metrics import best_rmsd    # noqa: E402

# (tag, pairs, atoms, maps per pair)
SHAPES = [('one_map', 4096, 40, 1), ('many_maps', 64, 40, 4096)]


def pairs(P, n, m, seed):
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(P, n, 3))
    step *= rng.uniform(1.1, 1.7, size=(P, n, 1)) / np.linalg.norm(step, axis=2, keepdims=True)
    xa = np.cumsum(step, axis=1)
    q, _ = np.linalg.qr(rng.normal(size=(P, 3, 3)))
    q *= np.sign(np.linalg.det(q))[:, None, None]
    xb = xa @ q.transpose(0, 2, 1) + 20.0 * rng.normal(size=(P, 1, 3)) + 0.2 * rng.normal(size=(P, n, 3))
    maps = np.argsort(rng.random(size=(P, n, m)), axis=1).astype(np.int16)         # [P][n][m]: atom-major, as the kernel reads it
    maps[:, :, -1] = np.arange(n)[None]
    offsets = np.arange(P + 1, dtype=np.int32) * m
    tensors = (xa.astype(np.float32), xb.astype(np.float32), np.full(P, n, np.int32), maps.reshape(-1), offsets)
    return [torch.from_numpy(t).cuda() for t in tensors]


def main(reps=100):
    assert torch.cuda.is_available(), 'needs a GPU'
    for tag, P, n, m in SHAPES:
        args = pairs(P, n, m, seed=P + m)
        for _ in range(5):
            rmsd, best, status = best_rmsd(*args)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            rmsd, best, status = best_rmsd(*args)
        t1.record()
        torch.cuda.synchronize()
        assert int(status.max()) == 0 and int((best == m - 1).sum()) == P, 'the identity, planted last, wins every pair'
        print(tag, f'P={P} n={n} maps={m}: {t0.elapsed_time(t1) / reps * 1e3:.1f} us per call (launch + output allocation, '
              f'device events), mean rmsd {float(rmsd.mean()):.4f} A', flush=True)


if __name__ == '__main__':
    main()
