"""Throughput of the double-cut kernel (csrc/fragment.hip) through ``fragment.fragment_all``; beside it, the same set through
``tests/fragment_ref.py`` in plain Python on the host, the only baseline there is.

    python scripts/time_fragment.py [--molecules 16384] [--batch 256] [--host 1]

Random drug-like graphs of 20..40 heavy atoms: five- and six-membered rings (half of the six-rings aromatic) and chains of one
to three atoms, each unit joined by a single bond to a random earlier atom; 70 % carbon, the rest N and O; one chain carbon in
five carries a double bond to an extra oxygen.  DeLinker's filter (3, 5, 2, 1).  Batches are padded to 40 rows and stay on the
device; the timed loop is one ``fragment_all`` per batch (launch, output allocation and the read of ``n_cuts`` that decides
whether to widen)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fragment_ref                                               # noqa: E402
from difflinker_amd import const                                  # noqa: E402
from difflinker_amd.fragment import fragment_all                  # noqa: E402

N_ROWS, NF = 40, const.NUMBER_OF_ATOM_TYPES
C, O, N_ = (const.ATOM2IDX[s] for s in 'CON')


def molecule(rng):
    want = int(rng.integers(20, 41))
    types, bonds = [], []
    while len(types) < want:
        first = len(types)
        k = int(rng.choice([0, 5, 6], p=[0.45, 0.2, 0.35]))
        size = min(k if k else int(rng.integers(1, 4)), want - first)
        types += [C if rng.random() < 0.7 else (N_ if rng.random() < 0.5 else O) for _ in range(size)]
        if k and size == k:
            order = 4 if k == 6 and rng.random() < 0.5 else 1
            bonds += [(first + a, first + (a + 1) % k, order) for a in range(k)]
        else:
            bonds += [(first + a, first + a + 1, 1) for a in range(size - 1)]
            if types[first] == C and rng.random() < 0.2 and len(types) < want:
                types.append(O)
                bonds.append((first, len(types) - 1, 2))
        if first:
            bonds.append((int(rng.integers(0, first)), first, 1))
    return types, bonds


def batches(n_molecules, batch, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for start in range(0, n_molecules, batch):
        molecules = [molecule(rng) for _ in range(min(batch, n_molecules - start))]
        B, E = len(molecules), max(len(b) for _, b in molecules)
        one_hot, mask = np.zeros((B, N_ROWS, NF), np.float32), np.zeros((B, N_ROWS), np.float32)
        bonds, n_bonds = np.zeros((B, E, 3), np.int32), np.zeros(B, np.int32)
        for b, (types, rows) in enumerate(molecules):
            one_hot[b, np.arange(len(types)), types] = 1
            mask[b, :len(types)] = 1
            bonds[b, :len(rows)] = rows
            n_bonds[b] = len(rows)
        out.append((one_hot, mask, bonds, n_bonds))
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--molecules', type=int, default=16384)
    p.add_argument('--batch', type=int, default=256)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--host', type=int, default=1, help='0: skip the plain-Python run on the host')
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    host = batches(a.molecules, a.batch)
    device = [tuple(torch.from_numpy(v).cuda() for v in item) for item in host]
    run = lambda: [fragment_all(*item, is_geom=False) for item in device]    # noqa: E731
    got = run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    cuts = sum(int(g.n_cuts.sum()) for g in got)
    cuttable = sum(int(g.n_cuttable.sum()) for g in got)
    best = min(times)
    print(f'{a.molecules} molecules of 20..40 atoms, B={a.batch} per launch: {cuttable / a.molecules:.1f} cuttable bonds and '
          f'{cuts / a.molecules:.2f} kept cuts per molecule; fragment_all {best * 1e3:.1f} ms for the set (best of {a.reps}, '
          f'{", ".join(f"{t * 1e3:.1f}" for t in times)}): {a.molecules / best:.0f} molecules/s', flush=True)
    if a.host:
        t0 = time.perf_counter()
        want = [fragment_ref.fragment_cuts(mask, one_hot, bonds, n_bonds, g.cuts.shape[1], carbon_type=C)
                for (one_hot, mask, bonds, n_bonds), g in zip(host, got)]
        t_host = time.perf_counter() - t0
        same = all(np.array_equal(getattr(g, name).cpu().numpy(), w[name]) for g, w in zip(got, want) for name in fragment_ref.FIELDS)
        print(f'tests/fragment_ref.py on the host: {t_host:.1f} s for the set: {a.molecules / t_host:.0f} molecules/s; '
              f'outputs agree: {same}', flush=True)


if __name__ == '__main__':
    main()
