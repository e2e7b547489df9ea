"""Throughput of the multi-cut kernel (csrc/fragment.hip, ``dl_fragment_multicuts``) through ``fragment.multi_all``; beside it,
the same outputs through ``tests/multicut_ref.py`` in plain Python on the host, the only baseline there is, and one launch of
the worst case the kernel takes: a centre with 64 one-atom arms, C(64,3) + C(64,4) + C(64,5) = 8 301 552 sets, all kept.

    python scripts/time_multicut.py [--molecules 16384] [--batch 256] [--host 1] [--host_molecules 1024]

Random drug-like graphs of 20..40 heavy atoms as in ``scripts/time_fragment.py``, drawn until one has at least three rings (the
reference's gate).  The reference's rule: 3 to 5 cuts, linker and fragments of at least 3 atoms, at most 40 atoms, three rings.
Batches are padded to 40 rows and stay on the device; the timed loop is one ``multi_all`` per batch (launch, output allocation,
the read of ``n_cuts`` that decides whether to widen, and the second launch when it does).  The host run covers the first
``--host_molecules`` molecules and is scaled to the set."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import multicut_ref                                               # noqa: E402
import time_fragment                                              # noqa: E402
from difflinker_amd.fragment import multi_all, multi_cuts         # noqa: E402

N_ROWS, NF, C = time_fragment.N_ROWS, time_fragment.NF, time_fragment.C


def molecule(rng):
    while True:
        types, bonds = time_fragment.molecule(rng)
        if len(bonds) - len(types) + 1 >= 3:
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


def timed(run, reps):
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return got, times


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--molecules', type=int, default=16384)
    p.add_argument('--batch', type=int, default=256)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--host', type=int, default=1, help='0: skip the plain-Python run on the host')
    p.add_argument('--host_molecules', type=int, default=1024, help='molecules of the host run (whole batches)')
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    host = batches(a.molecules, a.batch)
    device = [tuple(torch.from_numpy(v).cuda() for v in item) for item in host]
    got, times = timed(lambda: [multi_all(*item, is_geom=False) for item in device], a.reps)
    cuts = sum(int(g.n_cuts.sum()) for g in got)
    by_k = sum(g.n_cuts_k.sum(0).cpu().numpy() for g in got)
    cuttable = sum(int(g.n_cuttable.sum()) for g in got)
    widest = max(g.cuts.shape[1] for g in got)
    best = min(times)
    print(f'{a.molecules} molecules of 20..40 atoms with three rings, B={a.batch} per launch: {cuttable / a.molecules:.1f} cuttable '
          f'bonds and {cuts / a.molecules:.1f} kept stars per molecule ({", ".join(f"{v / a.molecules:.1f} of {k}" for k, v in zip((3, 4, 5), by_k))} '
          f'bonds; the widest batch holds {widest} records per molecule); multi_all {best * 1e3:.1f} ms for the set (best of '
          f'{a.reps}, {", ".join(f"{t * 1e3:.1f}" for t in times)}): {a.molecules / best:.0f} molecules/s', flush=True)

    # the worst case: 64 one-atom arms, every set a kept star; R = 64 records, so the time is the two walks' and not the stores'
    types, entries = multicut_ref.arms(64)
    one_hot = torch.zeros(1, 65, NF)
    one_hot[0, :, C] = 1
    arms = (one_hot.cuda(), torch.ones(1, 65).cuda(), torch.tensor([entries], dtype=torch.int32).cuda(),
            torch.tensor([64], dtype=torch.int32).cuda())
    rule = dict(min_linker=1, min_fragment=1, max_atoms=256, min_rings=0)
    worst, times = timed(lambda: multi_cuts(*arms, is_geom=False, capacity=64, **rule), a.reps)
    print(f'one molecule with 64 cuttable bonds, {int(worst.n_cuts[0])} kept stars ({worst.n_cuts_k[0].tolist()}), 64 records: one '
          f'launch {min(times) * 1e3:.2f} ms (best of {a.reps}, {", ".join(f"{t * 1e3:.2f}" for t in times)})', flush=True)

    if a.host:
        count = max(1, min(a.host_molecules, a.molecules) // a.batch)
        t0 = time.perf_counter()
        want = [multicut_ref.multicuts(mask, one_hot, bonds, n_bonds, g.cuts.shape[1], carbon_type=C)
                for (one_hot, mask, bonds, n_bonds), g in zip(host[:count], got)]
        t_host = time.perf_counter() - t0
        done = sum(len(item[3]) for item in host[:count])
        same = all(np.array_equal(getattr(g, name).cpu().numpy(), w[name]) for g, w in zip(got, want) for name in multicut_ref.FIELDS)
        print(f'tests/multicut_ref.py on the host: {t_host:.1f} s for {done} molecules: {done / t_host:.0f} molecules/s, '
              f'{t_host * a.molecules / done:.0f} s scaled to the set; outputs agree: {same}', flush=True)


if __name__ == '__main__':
    main()
