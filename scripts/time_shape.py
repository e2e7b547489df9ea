"""Launch time of the shape score (csrc/shape.hip) at its use: a sampled batch against the data set's molecules; beside it, the
same scores as ``tests/shape_ref.py`` computes them in numpy on the host.

    python scripts/time_shape.py
    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_shape.py --reps 20 --host-pairs 0

256 pairs of 50 atoms: a zigzag chain with side atoms, molecule B a jittered copy of molecule A (0.3 A), as a sample lies on
its true molecule.  Prints the device-event time per call (launch + output allocation); the kernel's own time is the
profiler's ``shape_scores_kernel`` row."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import shape_ref                                    # noqa: E402
from difflinker_amd import const                    # noqa: E402
from difflinker_amd.metrics import analyze_shapes   # noqa: E402

B, N_ATOMS = 256, 50
NF = const.GEOM_NUMBER_OF_ATOM_TYPES


def batch(seed=0):
    rng = np.random.default_rng(seed)
    k = np.arange(N_ATOMS)
    chain = np.stack([1.25 * k, 0.8 * (k % 2), np.zeros(N_ATOMS)], 1) * 0.5           # a folded chain, about 16 A long
    x_a = chain[None] + rng.normal(0, 1.0, size=(B, N_ATOMS, 3)) + rng.uniform(-20, 20, size=(B, 1, 3))
    x_b = x_a + rng.normal(0, 0.3, size=x_a.shape)
    types = rng.choice(NF, size=(B, N_ATOMS), p=[0.7, 0.1, 0.1, 0.02, 0.02, 0.02, 0.02, 0.01, 0.01])
    one_hot = np.eye(NF, dtype=np.float32)[types]
    return x_a.astype(np.float32), one_hot, np.ones((B, N_ATOMS), np.float32), x_b.astype(np.float32), one_hot, \
        np.ones((B, N_ATOMS), np.float32)


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
    p.add_argument('--host-pairs', type=int, default=32, help='pairs the numpy helper scores for its time (0: skip it)')
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    arrays = batch()
    x_a, one_hot_a, mask_a, x_b, one_hot_b, mask_b = (torch.from_numpy(v).cuda() for v in arrays)
    got, t_kernel = timed(lambda: analyze_shapes(one_hot_a, x_a, mask_a, one_hot_b, x_b, mask_b), a.reps)
    assert int(got.status.max()) == 0
    similarity = (got.vol_min.double() / got.vol_a.double()).mean().item()
    print(f'B={B} pairs of {N_ATOMS} atoms: analyze_shapes {t_kernel:.1f} us per call (device events, {a.reps} calls); '
          f'mean vol_a {got.vol_a.double().mean().item():.0f} points, mean similarity {similarity:.3f}', flush=True)
    if a.host_pairs:
        n = min(a.host_pairs, B)
        t0 = time.perf_counter()
        want = shape_ref.shape_scores(*(v[:n] for v in arrays))
        t_host = (time.perf_counter() - t0) / n
        same = all(np.array_equal(getattr(got, name).cpu().numpy()[:n], want[name]) for name in shape_ref.FIELDS)
        print(f'tests/shape_ref.py on the host: {t_host * 1e3:.2f} ms per pair over {n} pairs ({t_host * B * 1e3:.0f} ms for the '
              f'batch at that rate); outputs agree: {same}', flush=True)


if __name__ == '__main__':
    main()
