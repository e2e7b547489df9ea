"""Launch time of the clash score (csrc/clash.hip) at its two uses: a batch against its own pocket rows, and a batch against
a protein-sized shared list; beside each, the same counts written as ``torch.cdist`` expressions on the same device.

    python scripts/time_clash.py
    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_clash.py --reps 20

64 molecules of 40 generated atoms in a 20 A box; targets at protein density around them.  Prints the device-event time per
call (launch + output allocation); the kernel's own time is the profiler's `clash_scores_kernel` row."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difflinker_amd import const                    # noqa: E402
from difflinker_amd.metrics import analyze_clashes  # noqa: E402

# (tag, molecules, query atoms, in-batch targets, shared targets)
SHAPES = [('pocket_rows', 64, 40, 252, 0), ('shared_protein', 64, 40, 0, 20000)]
NF = const.GEOM_NUMBER_OF_ATOM_TYPES


def batch(B, nq, nt, M, seed):
    rng = np.random.default_rng(seed)
    N = nq + nt
    x = rng.uniform(0, 20.0, size=(B, N, 3)).astype(np.float32)
    types = rng.integers(0, NF, size=(B, N))
    qm = np.zeros((B, N), np.float32)
    qm[:, :nq] = 1
    px = rng.uniform(-20.0, 40.0, size=(M, 3)).astype(np.float32)       # 20 000 atoms in (60 A)^3: about a protein's density
    pt = rng.integers(0, NF, size=M).astype(np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    return dict(x=dev(x), types=dev(types), one_hot=dev(np.eye(NF, dtype=np.float32)[types]), qm=dev(qm), tm=dev(1 - qm),
                px=dev(px), pt=dev(pt))


def with_kernel(d, nq, nt, M):
    return analyze_clashes(d['one_hot'], d['x'], d['qm'], d['tm'] if nt else None, protein=(d['px'], d['pt']) if M else None)


def with_cdist(d, nq, nt, M, table, cutoff=4.0):
    """The per-molecule outputs of the kernel as tensor expressions (distances, not squared distances)."""
    q, qa = d['x'][:, :nq], d['types'][:, :nq]
    if nt:
        t, tb = d['x'][:, nq:], d['types'][:, nq:]
    else:
        t, tb = d['px'][None].expand(q.shape[0], M, 3), d['pt'][None].expand(q.shape[0], M).long()
    dist = torch.cdist(q, t, compute_mode='donot_use_mm_for_euclid_dist')
    clash = dist < table[qa[:, :, None], tb[:, None, :]]
    return clash.sum((1, 2)), clash.any(2).sum(1), (dist < cutoff).sum((1, 2)), dist.amin((1, 2))


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
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    table = const.clash_threshold_table(True).cuda()
    for tag, B, nq, nt, M in SHAPES:
        d = batch(B, nq, nt, M, seed=nt + M)
        got, t_kernel = timed(lambda: with_kernel(d, nq, nt, M), a.reps)
        ref, t_cdist = timed(lambda: with_cdist(d, nq, nt, M, table), a.reps)
        assert int(got.status.max()) == 0 and int(got.n_target[0]) == nt + M
        same = bool((got.n_clashes == ref[0]).all() and (got.n_clash_atoms == ref[1]).all() and (got.n_contacts == ref[2]).all())
        print(tag, f'B={B} queries={nq} own targets={nt} shared targets={M}: analyze_clashes {t_kernel:.1f} us per call, '
              f'torch.cdist expressions {t_cdist:.1f} us per call (device events, {a.reps} calls each); '
              f'{int(got.n_clashes.sum())} clashes, {int(got.n_contacts.sum())} contacts, counts agree: {same}', flush=True)


if __name__ == '__main__':
    main()
