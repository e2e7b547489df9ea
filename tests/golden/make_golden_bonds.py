"""Generate ``bond_orders.npz`` from the UNMODIFIED reference: the decisions of ``get_bond_order`` around every threshold
of every element pair, and the ``E`` matrices of ``build_xae_molecule`` for random molecules (src/molecule_builder.py:44-102).

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bonds.py

RDKit is replaced by the stand-ins of ``make_golden._stub_reference_dependencies``; neither function touches it.  The file
holds data only and is written with fixed zip time stamps, so a second run reproduces it bit for bit.

``sweep_*``  one row per (vocabulary, ordered element pair a, b, distance): the order the reference gives two atoms of
             these types at that distance (it looks the pair up with the lower atom index first).  Distances: a relative
             1e-4 below and above every threshold the pair has, 8 A for every pair, and 1.0 A for the pairs without a
             single-bond length.
``b<k>_*``   ragged batches: ``one_hot [B,N,nf]``, ``x [B,N,3]``, ``mask [B,N]`` (masked rows sit between the real ones and hold
             the coordinates of real atoms plus a small shift, so an unmasked read would bond them), ``E [B,60,60]`` (the
             reference's matrix of the masked molecule, zero-padded), ``is_geom``.
Condition (asserted here, relied on by the tests): no pair of a stored molecule lies within a relative 1e-5 of a threshold of
its element pair; a molecule that violates it is redrawn, so the tests compare every pair of every molecule.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_reference_dependencies      # noqa: E402  (sets sys.path: repository, tests/, reference)

_stub_reference_dependencies()
from src import const as ref_const                         # noqa: E402
from src.molecule_builder import build_xae_molecule, get_bond_order    # noqa: E402

BAND = 1e-5
MAX_ATOMS = 60
# (is_geom, padded width N, molecules)
BATCHES = [(True, 64, 16), (True, 64, 16), (True, 72, 16), (True, 320, 16), (False, 64, 16), (False, 61, 16)]


def thresholds(idx2atom, a, b):
    """The upper bounds (pm) the reference compares a pair of atom indices against, in nesting order."""
    lo, hi = idx2atom[min(a, b)], idx2atom[max(a, b)]
    out = []
    for table, margin in zip((ref_const.BONDS_1, ref_const.BONDS_2, ref_const.BONDS_3), ref_const.MARGINS_EDM):
        if lo not in table or hi not in table[lo]:
            break
        out.append(table[lo][hi] + margin)
    return out


def reference_order(idx2atom, a, b, dist):
    pair = sorted([torch.tensor(a), torch.tensor(b)])                       # molecule_builder.py:66-67
    return int(get_bond_order(idx2atom[pair[0].item()], idx2atom[pair[1].item()], torch.tensor(dist, dtype=torch.float32)))


def sweep():
    rows = []
    for is_geom in (False, True):
        idx2atom = ref_const.GEOM_IDX2ATOM if is_geom else ref_const.IDX2ATOM
        for a in range(len(idx2atom)):
            for b in range(len(idx2atom)):
                thr = thresholds(idx2atom, a, b)
                dists = [8.0] + ([] if thr else [1.0])
                for t in thr:
                    dists += [t / 100 * (1 - 1e-4), t / 100 * (1 + 1e-4)]
                for d in dists:
                    d32 = float(np.float32(d))
                    rows.append((int(is_geom), a, b, d32, reference_order(idx2atom, a, b, d32)))
    rows = np.array(rows, dtype=np.float64)
    return {'sweep_is_geom': rows[:, 0].astype(np.int8), 'sweep_a': rows[:, 1].astype(np.int8),
            'sweep_b': rows[:, 2].astype(np.int8), 'sweep_dist': rows[:, 3].astype(np.float32),
            'sweep_order': rows[:, 4].astype(np.int8)}


def grow(rng, n, n_types):
    """A random chain: every atom sits 1.1 .. 1.7 A from the previous one (or, one time in four, from an earlier one)."""
    weights = np.array([6, 3, 3] + [1] * (n_types - 3), dtype=np.float64)
    types = rng.choice(n_types, size=n, p=weights / weights.sum())
    pos = np.zeros((n, 3))
    for k in range(1, n):
        parent = k - 1 if rng.random() < 0.75 else rng.integers(0, k)
        step = rng.normal(size=3)
        pos[k] = pos[parent] + step / np.linalg.norm(step) * rng.uniform(1.1, 1.7)
    pos -= pos.mean(0)
    return types, pos.astype(np.float32)


def in_band(idx2atom, types, pos):
    d = 100 * np.linalg.norm(pos[:, None].astype(np.float64) - pos[None].astype(np.float64), axis=-1)
    for i in range(len(types)):
        for j in range(i):
            for t in thresholds(idx2atom, types[i], types[j]):
                if abs(d[i, j] / t - 1) < BAND:
                    return True
    return False


def batches():
    rng = np.random.default_rng(20240)
    out, orders, pieces, redrawn, total = {}, set(), 0, 0, 0
    for k, (is_geom, N, B) in enumerate(BATCHES):
        idx2atom = ref_const.GEOM_IDX2ATOM if is_geom else ref_const.IDX2ATOM
        nf = len(idx2atom)
        one_hot = np.zeros((B, N, nf), np.float32)
        x = np.zeros((B, N, 3), np.float32)
        mask = np.zeros((B, N), np.float32)
        E_all = np.zeros((B, MAX_ATOMS, MAX_ATOMS), np.int8)
        for b in range(B):
            n = int(rng.integers(5, min(MAX_ATOMS, N) + 1))
            while True:
                types, pos = grow(rng, n, nf)
                total += 1
                if not in_band(idx2atom, types, pos):
                    break
                redrawn += 1
            _, A, E = build_xae_molecule(torch.from_numpy(pos), torch.from_numpy(types), is_geom=is_geom)
            assert torch.equal(A, E.bool())
            E = E.numpy()
            rows = np.sort(rng.choice(N, size=n, replace=False))
            mask[b, rows] = 1
            x[b, rows] = pos
            one_hot[b, rows, types] = 1
            junk = np.setdiff1d(np.arange(N), rows)
            x[b, junk] = pos[rng.integers(0, n, size=len(junk))] + rng.normal(scale=0.3, size=(len(junk), 3)).astype(np.float32)
            one_hot[b, junk, rng.integers(0, nf, size=len(junk))] = 1
            E_all[b, :n, :n] = E
            orders |= set(np.unique(E).tolist())
            # pieces of the bond graph, for the assertion below only
            label = np.arange(n)
            for _ in range(n):
                for i, j in zip(*np.nonzero(E)):
                    label[i] = label[j] = min(label[i], label[j])
            pieces += len(np.unique(label)) > 1
        out.update({f'b{k}_one_hot': one_hot, f'b{k}_x': x, f'b{k}_mask': mask, f'b{k}_E': E_all,
                    f'b{k}_is_geom': np.int8(is_geom)})
    assert orders == {0, 1, 2, 3}, orders
    assert pieces >= 4, pieces
    print(f'{total - redrawn} molecules, {redrawn} redrawn for the {BAND:g} band, {pieces} in more than one piece')
    out['n_batches'] = np.int32(len(BATCHES))
    return out


def save_deterministic(name, arrays):
    path = os.path.join(HERE, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print('wrote', name, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(1)
    save_deterministic('bond_orders', {**sweep(), **batches()})
