"""Launch time of the interaction score (csrc/interaction.hip) at its two uses: a batch against its own pocket rows (typing
and scoring, two launches), and a batch against a protein-sized shared list that was typed once before.

    python scripts/time_interactions.py
    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/time_interactions.py --reps 20

64 molecules of 40 ligand atoms (10 of them the generated linker) in a 20 A box; targets at protein density around them.
Prints the device-event time per call (launches + output allocation); the kernels' own times are the profiler's
`interaction_types_kernel` and `interaction_scores_kernel` rows."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difflinker_amd import const                                          # noqa: E402
from difflinker_amd.metrics import analyze_interactions, protein_types   # noqa: E402

# (tag, molecules, ligand atoms, query atoms among them, in-batch targets, shared targets)
SHAPES = [('pocket_rows', 64, 40, 10, 252, 0), ('shared_protein', 64, 40, 10, 0, 20000)]
NF = const.GEOM_NUMBER_OF_ATOM_TYPES


def batch(B, nl, nq, nt, M, seed):
    rng = np.random.default_rng(seed)
    N = nl + nt
    x = rng.uniform(0, 20.0, size=(B, N, 3)).astype(np.float32)
    types = rng.integers(0, 3, size=(B, N))                              # C, O, N
    qm, lig = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    qm[:, :nq] = 1
    lig[:, :nl] = 1
    px = rng.uniform(-20.0, 40.0, size=(M, 3)).astype(np.float32)       # 20 000 atoms in (60 A)^3: about a protein's density
    pt = rng.integers(0, 3, size=M).astype(np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    return dict(x=dev(x), one_hot=dev(np.eye(NF, dtype=np.float32)[types]), qm=dev(qm), lig=dev(lig), tm=dev(1 - lig),
                px=dev(px), pt=dev(pt))


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
    for tag, B, nl, nq, nt, M in SHAPES:
        d = batch(B, nl, nq, nt, M, seed=nt + M)
        protein = None
        if M:
            xs, t_types = timed(lambda: protein_types(d['px'], d['pt']), max(a.reps // 10, 2))
            protein = (d['px'], d['pt'], xs)
            print(tag, f'protein_types of {M} atoms: {t_types:.1f} us per call (once per protein)', flush=True)
        got, t_call = timed(lambda: analyze_interactions(d['one_hot'], d['x'], d['qm'], d['lig'], d['tm'] if nt else None,
                                                         protein=protein), a.reps)
        assert int(got.status.max()) == 0 and int(got.n_target[0]) == nt + M
        print(tag, f'B={B} ligand={nl} queries={nq} own targets={nt} shared targets={M}: analyze_interactions {t_call:.1f} us '
              f'per call (device events, {a.reps} calls); {int(got.n_pairs.sum())} pairs inside 8 A, '
              f'{int(got.n_hbonds.sum())} hydrogen-bond pairs, {int(got.n_hydrophobic.sum())} hydrophobic pairs', flush=True)


if __name__ == '__main__':
    main()
