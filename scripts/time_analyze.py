"""Launch time of the molecule keys (csrc/mol_keys.hip) at the headline shape and at a pocket shape with the pocket dropped.

    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_analyze.py

Molecules are random chains with 1.1 .. 1.7 A steps (bonded like generated molecules, not like a dense cloud).  Bonds are
perceived once, outside the timed loop; the loop launches `dl_molecule_keys` alone.  Prints the device-event time per call as
well; the kernel's own time is the profiler's `molecule_keys_kernel` row."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from difflinker_amd.metrics import molecule_keys                       # noqa: E402
from difflinker_amd.molecule_builder import perceive_all_bonds         # noqa: E402
from time_bonds import chains                                          # noqa: E402

# (tag, B, N, kept atoms per molecule): at the pocket shape every row is a real atom and the last N - kept are dropped
SHAPES = [('headline', 256, 50, 50), ('pocket_dropped', 64, 292, 40)]


def main(reps=200):
    assert torch.cuda.is_available(), 'needs a GPU'
    for tag, B, N, kept in SHAPES:
        one_hot, x, mask = chains(B, N, N, 9, seed=B + N)
        drop = None
        if kept < N:
            drop = torch.zeros_like(mask)
            drop[:, kept:] = 1
        found = perceive_all_bonds(one_hot, x, mask, True)
        for _ in range(10):
            res = molecule_keys(one_hot, mask, found, True, drop)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            res = molecule_keys(one_hot, mask, found, True, drop)
        t1.record()
        torch.cuda.synchronize()
        print(tag, f'B={B} N={N} kept={kept}: {t0.elapsed_time(t1) / reps * 1e3:.1f} us per call (launch + output '
              f'allocation, device events); mean bonds kept {float(res.n_bonds.float().mean()):.1f}, '
              f'valid {float((res.n_over == 0).float().mean()):.2f}, one piece {float((res.n_components == 1).float().mean()):.2f}, '
              f'distinct keys {int(res.key.unique().numel())}', flush=True)


if __name__ == '__main__':
    main()
