"""Launch time of bond perception (csrc/bonds.hip) at the headline shape and at a pocket shape.

    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_bonds.py

Molecules are random chains with 1.1 .. 1.7 A steps (bonded like generated molecules, not like a dense cloud).  Prints the
device-event time per launch as well; the kernel's own time is the profiler's `perceive_bonds_kernel` row."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difflinker_amd.molecule_builder import perceive_bonds, summary    # noqa: E402

# (tag, B, N, real atoms per molecule): with a hidden pocket only the fragments and the linker are real
SHAPES = [('headline', 256, 50, 50), ('pocket_hidden', 64, 292, 40), ('pocket_all_real', 64, 292, 292)]


def chains(B, N, n_real, nf, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, N, 3), np.float32)
    for b in range(B):
        for k in range(1, n_real):
            step = rng.normal(size=3)
            x[b, k] = x[b, k - 1] + step / np.linalg.norm(step) * rng.uniform(1.1, 1.7)
    one_hot = np.zeros((B, N, nf), np.float32)
    one_hot[np.arange(B)[:, None], np.arange(N)[None], rng.integers(0, 3, size=(B, N))] = 1
    mask = np.zeros((B, N, 1), np.float32)
    mask[:, :n_real] = 1
    return [torch.from_numpy(a).cuda() for a in (one_hot, x, mask)]


def main(reps=200):
    assert torch.cuda.is_available(), 'needs a GPU'
    for tag, B, N, n_real in SHAPES:
        args = chains(B, N, n_real, 9, seed=B + N)
        for _ in range(10):
            found = perceive_bonds(*args, True)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            found = perceive_bonds(*args, True)
        t1.record()
        torch.cuda.synchronize()
        print(tag, f'B={B} N={N} real={n_real}: {t0.elapsed_time(t1) / reps * 1e3:.1f} us per call (launch + output '
              f'allocation, device events)', summary([found]), flush=True)


if __name__ == '__main__':
    main()
