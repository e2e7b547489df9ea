"""Time of the pocket kernel (csrc/pocket.hip) for a batch of (ligand, protein) pairs, and of a whole ``prepare --proteins`` run
split into its shares; beside them ``io.get_pocket`` per pair on the host, which parses the protein and builds the distance
matrix once per ligand as the reference does.

    python scripts/time_pocket.py [--pairs 1024] [--proteins 64] [--reps 20] [--host_pairs 16] [--complexes 32] [--ligands 4]

The complex is the committed hsp90 fixture: the 3hz1 protein (1635 atoms) and its ligand (26 heavy atoms).  Every protein of
the set is a copy moved as a whole, every ligand the 3hz1 ligand moved with its protein and then by up to 2 A on its own, so the
pockets differ from pair to pair.  The launch is timed with device events after a warm-up, inputs and outputs staying on the
device; the ``prepare`` run reads ``--complexes`` protein files and an SDF of ``--ligands`` records per protein from a temporary
directory and reports the seconds of ``prepare.prepare_pockets``: parse (the proteins, in Python), gpu (upload, both kernels,
until the device is idle) and assembly (the dicts)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from difflinker_amd import io, prepare                           # noqa: E402
from difflinker_amd.pocket import select_pockets                  # noqa: E402

CASE = os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', 'hsp90')
PROTEIN, LIGAND = os.path.join(CASE, '3hz1_protein.pdb'), os.path.join(CASE, '3hz1_ligand_obabel.sdf')


def moved_pdb(lines, shift):
    out = []
    for ln in lines:
        if ln[0:6] in ('ATOM  ', 'HETATM'):
            x, y, z = (float(ln[30 + 8 * k:38 + 8 * k]) + shift[k] for k in range(3))
            ln = f'{ln[:30]}{x:8.3f}{y:8.3f}{z:8.3f}{ln[54:]}'
        out.append(ln)
    return out


def moved_sdf(lines, shift, name):
    n = int(lines[3][0:3])
    out = [name + '\n'] + lines[1:4]
    for ln in lines[4:4 + n]:
        x, y, z = (float(ln[10 * k:10 * k + 10]) + shift[k] for k in range(3))
        out.append(f'{x:10.4f}{y:10.4f}{z:10.4f}{ln[30:]}')
    return out + lines[4 + n:]


def time_launch(a):
    rng = np.random.default_rng(0)
    protein, mol = io.read_pdb_arrays(PROTEIN), io.read_molecule(LIGAND)
    M, group = len(protein.resseq), io.groups(protein)
    shifts = rng.uniform(-50, 50, (a.proteins, 3)).round(3)
    protein_x = np.concatenate([protein.coords + s.astype(np.float32) for s in shifts])
    which = rng.integers(0, a.proteins, a.pairs)
    ligand_x = mol.positions[None] + shifts[which][:, None] + rng.uniform(-2, 2, (a.pairs, 1, 3)).round(4)
    dev = torch.device('cuda:0')
    args = (torch.from_numpy(protein_x).to(dev), torch.from_numpy(np.tile(group, a.proteins)).to(dev),
            torch.arange(a.proteins + 1, dtype=torch.int32, device=dev) * M, torch.from_numpy(which.astype(np.int32)).to(dev),
            torch.from_numpy(ligand_x).to(dev), torch.ones(a.pairs, len(mol), device=dev))
    run = lambda: select_pockets(*args, capacity=512, max_atoms=M)                                  # noqa: E731
    for _ in range(3):
        got = run()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        start.record()
        got = run()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    n_pocket = got.n_pocket.cpu().numpy()
    assert not int(got.status.abs().sum()), 'a pair was truncated or could not be answered'
    med = float(np.median(times))
    print(f'{a.pairs} pairs over {a.proteins} proteins of {M} atoms, {len(mol)} ligand atoms: {n_pocket.mean():.0f} pocket atoms per '
          f'pair; one select_pockets launch (with its output allocation) {med:.3f} ms median of {a.reps} (min {min(times):.3f}, max '
          f'{max(times):.3f}): {med * 1e3 / a.pairs:.2f} us per pair, {a.pairs * M * len(mol) / med / 1e6:.1f} G pair tests/s '
          'if none left early', flush=True)
    # the host rule of the same machine: io.get_pocket per pair (parse + matrix), and the matrix alone on parsed arrays
    t0 = time.perf_counter()
    for _ in range(a.host_pairs):
        want = io.get_pocket(mol, PROTEIN)
    t_host = (time.perf_counter() - t0) / a.host_pairs
    t0 = time.perf_counter()
    for _ in range(a.host_pairs):
        d = np.linalg.norm(protein.coords[:, None, :] - mol.positions[None, :, :], axis=-1)
        np.isin(protein.resseq, np.unique(protein.resseq[d.min(1) <= 6]))
    t_matrix = (time.perf_counter() - t0) / a.host_pairs
    print(f'io.get_pocket on the host: {t_host * 1e3:.1f} ms per pair ({len(want[2])} atoms), of which the distance matrix and the '
          f'selection on parsed arrays {t_matrix * 1e3:.2f} ms; {a.pairs} pairs: {t_host * a.pairs:.1f} s and {t_matrix * a.pairs:.2f} s '
          f'against {med:.3f} ms on the device', flush=True)


def time_prepare(a):
    rng = np.random.default_rng(1)
    with open(PROTEIN) as f:
        pdb = f.readlines()
    with open(LIGAND) as f:
        sdf = f.readlines()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, 'ligands.sdf'), 'w') as out:
            for k in range(a.complexes):
                shift = rng.uniform(-50, 50, 3).round(3)
                with open(os.path.join(tmp, f'c{k:04d}_protein.pdb'), 'w') as f:
                    f.writelines(moved_pdb(pdb, shift))
                for j in range(a.ligands):
                    out.writelines(moved_sdf(sdf, shift + rng.uniform(-2, 2, 3).round(4), f'c{k:04d}_ligand_{j}'))
        t0 = time.perf_counter()
        molecules, _ = io.read_sdf_molecules(os.path.join(tmp, 'ligands.sdf'))
        t_sdf = time.perf_counter() - t0
        for attempt in ('first', 'second'):                               # the first run loads the code objects
            seconds = {}
            t0 = time.perf_counter()
            full, bb, rows, skipped = prepare.prepare_pockets(molecules, tmp, torch.device('cuda:0'), seconds=seconds)
            total = time.perf_counter() - t0
            shares = ', '.join(f'{k} {v:.3f} s ({100 * v / total:.0f} %)' for k, v in seconds.items())
            print(f'prepare_pockets, {attempt} run: {a.complexes} proteins, {len(molecules)} ligands (read in {t_sdf:.3f} s), '
                  f'{len(full)} examples, {total:.3f} s: {shares}; skipped {skipped}', flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--pairs', type=int, default=1024)
    p.add_argument('--proteins', type=int, default=64)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--host_pairs', type=int, default=16)
    p.add_argument('--complexes', type=int, default=32)
    p.add_argument('--ligands', type=int, default=4)
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), 'needs a GPU'
    time_launch(a)
    time_prepare(a)


if __name__ == '__main__':
    main()
