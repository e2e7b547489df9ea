"""Bond perception on the GPU against the reference's recorded ``E`` matrices (tests/golden/bond_orders.npz, made by
make_golden_bonds.py from the unmodified reference): every pair of every molecule, exactly.  The fixture keeps every pair a
relative 1e-5 away from the thresholds of its element pair, far more than the few ulp (~1e-7) by which two fp32 evaluations
of a distance differ, so no pair is excluded and nothing is compared with a tolerance."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_generate import IO_DIR, ddpm_hparams, read_xyz

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def every_pair(n):
    """A list capacity no molecule of n atoms can overflow (the fixture's random chains fold back on themselves and hold
    several bonds per atom, more than the default 4 * N of a batch as narrow as its largest molecule)."""
    return n * (n - 1) // 2


def batches(golden_dir):
    g = np.load(os.path.join(golden_dir, 'bond_orders.npz'))
    for k in range(int(g['n_batches'])):
        yield (torch.from_numpy(g[f'b{k}_one_hot']), torch.from_numpy(g[f'b{k}_x']), torch.from_numpy(g[f'b{k}_mask'])[:, :, None],
               bool(g[f'b{k}_is_geom']), g[f'b{k}_E'].astype(np.int64))


def expected(E, n):
    """Bond list in torch.nonzero order, valences and union-find components of one recorded matrix."""
    E = E[:n, :n]
    rows = [(i, j, int(E[i, j])) for i, j in zip(*np.nonzero(E))]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j, _ in rows:
        ri, rj = find(i), find(j)
        parent[max(ri, rj)] = min(ri, rj)
    labels = [find(a) for a in range(n)]
    smallest = {}
    for a, r in enumerate(labels):
        smallest.setdefault(r, a)
    return rows, (E.sum(0) + E.sum(1)).tolist(), [smallest[r] for r in labels]


def test_bonds_valences_components_equal_the_reference(golden_dir):
    from difflinker_amd.molecule_builder import build_xae_molecules, is_connected, perceive_bonds
    n_mols, widest, orders, split = 0, 0, set(), 0
    for one_hot, x, mask, is_geom, E_all in batches(golden_dir):
        dev = [t.to(DEV) for t in (one_hot, x, mask)]
        cap = every_pair(int(mask.sum(1).max()))
        found = perceive_bonds(*dev, is_geom, capacity=cap)
        again = perceive_bonds(*dev, is_geom, capacity=cap)
        one_piece = is_connected(*dev, is_geom).cpu()
        xae = build_xae_molecules(*dev, is_geom)
        B, N = mask.shape[:2]
        widest = max(widest, N)
        assert found.bonds.shape == (B, cap, 3) and found.bonds.dtype == torch.int32
        for name, a, b in zip(found._fields, found, again):
            if name == 'bonds':                                   # rows from n_bonds on are not written
                for m in range(B):
                    nb = int(found.n_bonds[m])
                    assert torch.equal(a[m, :nb], b[m, :nb])
            else:
                assert torch.equal(a, b), f'{name} differs between two runs'
        for m in range(B):
            n = int(mask[m].sum())
            rows, valence, labels = expected(E_all[m], n)
            assert int(found.n_bonds[m]) == len(rows)
            assert found.bonds[m, :len(rows)].cpu().tolist() == [list(r) for r in rows], 'bond list, orders or their order'
            assert found.valence[m].cpu().tolist() == valence + [0] * (N - n)
            assert found.component[m].cpu().tolist() == labels + [-1] * (N - n)
            assert int(found.n_components[m]) == len(set(labels))
            assert bool(one_piece[m]) == (len(set(labels)) == 1)
            assert int(found.status[m]) == 0
            X, A, E = xae[m]
            assert X.tolist() == one_hot[m][mask[m, :, 0] != 0].argmax(1).tolist()
            assert E.dtype == torch.int32 and np.array_equal(E.numpy(), E_all[m][:n, :n]) and torch.equal(A, E.bool())
            n_mols += 1
            orders |= {r[2] for r in rows}
            split += len(set(labels)) > 1
    assert n_mols >= 96 and widest >= 300 and orders == {1, 2, 3} and split >= 4


def test_masked_rows_and_their_contents_change_nothing(golden_dir):
    from difflinker_amd.molecule_builder import perceive_bonds
    one_hot, x, mask, is_geom, _ = next(batches(golden_dir))
    cap = every_pair(int(mask.sum(1).max()))
    found = perceive_bonds(one_hot.to(DEV), x.to(DEV), mask.to(DEV), is_geom, capacity=cap)
    g = torch.Generator().manual_seed(1)
    off = mask[:, :, 0] == 0
    x2, h2 = x.clone(), one_hot.clone()
    x2[off] = torch.randn(int(off.sum()), 3, generator=g) * 50
    rows = torch.nonzero(off)[::3]
    x2[rows[:, 0], rows[:, 1]] = float('nan')                     # not a real atom: no status bit either
    h2[off] = torch.rand(int(off.sum()), h2.shape[2], generator=g)
    other = perceive_bonds(h2.to(DEV), x2.to(DEV), mask.to(DEV), is_geom, capacity=cap)
    # the same molecules with the masked rows removed and the real rows packed to the front of a narrower batch
    n_max = int(mask.sum(1).max())
    h3, x3, m3 = torch.zeros(len(x), n_max, h2.shape[2]), torch.zeros(len(x), n_max, 3), torch.zeros(len(x), n_max, 1)
    for b in range(len(x)):
        keep = ~off[b]
        n = int(keep.sum())
        h3[b, :n], x3[b, :n], m3[b, :n] = one_hot[b][keep], x[b][keep], 1
    packed = perceive_bonds(h3.to(DEV), x3.to(DEV), m3.to(DEV), is_geom, capacity=cap)
    for res, width in ((other, x.shape[1]), (packed, n_max)):
        assert torch.equal(res.n_bonds, found.n_bonds) and torch.equal(res.n_components, found.n_components)
        assert torch.equal(res.status, found.status)
        assert torch.equal(res.valence[:, :n_max], found.valence[:, :n_max])
        assert torch.equal(res.component[:, :n_max], found.component[:, :n_max])
        for b in range(len(x)):
            nb = int(found.n_bonds[b])
            assert torch.equal(res.bonds[b, :nb], found.bonds[b, :nb])


def test_overflow_and_nonfinite_set_their_bits_only(golden_dir):
    from difflinker_amd import _lib
    from difflinker_amd.molecule_builder import build_xae_molecules, perceive_bonds
    one_hot, x, mask, is_geom, E_all = next(batches(golden_dir))
    dev = [t.to(DEV) for t in (one_hot, x, mask)]
    every = every_pair(int(mask.sum(1).max()))
    full = perceive_bonds(*dev, is_geom, capacity=every)
    assert int(full.status.max()) == 0
    cap = (int(full.n_bonds.min()) + int(full.n_bonds.max())) // 2
    assert int(full.n_bonds.min()) < cap < int(full.n_bonds.max()), 'the batch has molecules on both sides of the capacity'
    guard = torch.full((len(x), cap + 2, 3), -7, dtype=torch.int32, device=DEV)
    small = perceive_bonds(*dev, is_geom, capacity=cap)
    assert torch.equal(small.n_bonds, full.n_bonds), 'the true count is reported beyond the capacity'
    assert torch.equal(small.status, (full.n_bonds > cap).int() * _lib.DL_BONDS_OVERFLOW)
    for name in ('valence', 'n_components', 'component'):
        assert torch.equal(getattr(small, name), getattr(full, name))
    for b in range(len(x)):
        nb = min(cap, int(full.n_bonds[b]))
        assert torch.equal(small.bonds[b, :nb], full.bonds[b, :nb])
    # nothing is written past the capacity: run the C entry on a guarded buffer
    lib = _lib.load()
    B, N, nf = one_hot.shape
    from difflinker_amd import const
    table = const.bond_threshold_table(is_geom).to(DEV)
    outs = [torch.empty(s, dtype=torch.int32, device=DEV) for s in ((B,), (B, N), (B,), (B, N), (B,))]
    args = _lib.DLBondsArgs(B=B, N=N, nf=nf, one_hot=dev[0].data_ptr(), x=dev[1].data_ptr(),
                            node_mask=dev[2].contiguous().data_ptr(), table=table.data_ptr(), table_len=table.numel(),
                            capacity=cap, n_bonds=outs[0].data_ptr(), bonds=guard.data_ptr(), valence=outs[1].data_ptr(),
                            n_components=outs[2].data_ptr(), component=outs[3].data_ptr(), status=outs[4].data_ptr())
    assert lib.dl_perceive_bonds(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    flat = guard.reshape(-1)
    assert bool((flat[B * cap * 3:] == -7).all()), 'written past B * capacity rows'
    assert torch.equal(outs[0], full.n_bonds)
    # build_xae_molecules widens the list by itself
    one = [(torch.zeros(1, 12, 8)), torch.zeros(1, 12, 3), torch.ones(1, 12, 1)]
    one[0][:, :, 0] = 1
    one[1][0, :, 0] = torch.arange(12) * 0.01                    # twelve carbons within 0.11 A: all 66 pairs are triple bonds
    X, A, E = build_xae_molecules(*[t.to(DEV) for t in one], False)[0]
    assert int(A.sum()) == 66 and set(E[A].tolist()) == {3}
    crowded = perceive_bonds(*[t.to(DEV) for t in one], False)
    assert int(crowded.n_bonds) == 66 and int(crowded.status) == _lib.DL_BONDS_OVERFLOW and int(crowded.n_components) == 1

    # a NaN and an inf coordinate: their atoms bond to nothing, every other pair is as before
    for bad_value in (float('nan'), float('inf')):
        xb = x.clone()
        victim = int(torch.nonzero(mask[2, :, 0])[3])            # the fourth real atom of molecule 2
        xb[2, victim, 1] = bad_value
        res = perceive_bonds(one_hot.to(DEV), xb.to(DEV), mask.to(DEV), is_geom, capacity=every)
        want = torch.zeros(len(x), dtype=torch.int32)
        want[2] = _lib.DL_BONDS_NONFINITE
        assert torch.equal(res.status.cpu(), want)
        keep = [r for r in full.bonds[2, :int(full.n_bonds[2])].cpu().tolist() if 3 not in r[:2]]
        assert res.bonds[2, :int(res.n_bonds[2])].cpu().tolist() == keep
        assert int(res.valence[2, 3]) == 0 and int(res.component[2, 3]) == 3
        others = [b for b in range(len(x)) if b != 2]
        assert torch.equal(res.n_bonds[others], full.n_bonds[others])
        assert torch.equal(res.component[others], full.component[others])


def test_empty_batch_and_raw_c_entry_error_codes():
    from difflinker_amd import _lib, const
    from difflinker_amd.molecule_builder import perceive_bonds
    found = perceive_bonds(torch.zeros(0, 10, 9, device=DEV), torch.zeros(0, 10, 3, device=DEV),
                           torch.zeros(0, 10, 1, device=DEV), True)
    assert found.n_bonds.shape == (0,) and found.bonds.shape == (0, 40, 3) and found.component.shape == (0, 10)
    none = perceive_bonds(torch.zeros(2, 6, 9, device=DEV), torch.zeros(2, 6, 3, device=DEV), torch.zeros(2, 6, 1, device=DEV), True)
    assert none.n_bonds.tolist() == [0, 0] and none.n_components.tolist() == [0, 0] and none.component.unique().tolist() == [-1]
    # two carbons 1.5 A apart through raw ctypes
    lib = _lib.load()
    h = torch.zeros(1, 2, 8, device=DEV); h[:, :, 0] = 1
    x = torch.tensor([[[0.0, 0, 0], [1.5, 0, 0]]], device=DEV)
    m = torch.ones(1, 2, device=DEV)
    table = const.bond_threshold_table(False).to(DEV)
    o = [torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((1,), (1, 4, 3), (1, 2), (1,), (1, 2), (1,))]
    kw = dict(B=1, N=2, nf=8, one_hot=h.data_ptr(), x=x.data_ptr(), node_mask=m.data_ptr(), table=table.data_ptr(),
              table_len=table.numel(), capacity=4, n_bonds=o[0].data_ptr(), bonds=o[1].data_ptr(), valence=o[2].data_ptr(),
              n_components=o[3].data_ptr(), component=o[4].data_ptr(), status=o[5].data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in (dict(N=0), dict(N=1025), dict(table_len=9 * 9 * 3), dict(x=None), dict(status=None), dict(nf=17)):
        assert lib.dl_perceive_bonds(ctypes.byref(_lib.DLBondsArgs(**dict(kw, **bad))), stream) == -1, bad
    assert lib.dl_perceive_bonds(ctypes.byref(_lib.DLBondsArgs(**dict(kw, B=0))), stream) == 0
    torch.cuda.synchronize()
    assert o[0].tolist() == [0], 'nothing ran yet'
    assert lib.dl_perceive_bonds(ctypes.byref(_lib.DLBondsArgs(**kw)), stream) == 0
    torch.cuda.synchronize()
    assert o[0].tolist() == [1] and o[1][0, 0].tolist() == [1, 0, 1] and o[2].tolist() == [[1, 1]]
    assert o[3].tolist() == [1] and o[4].tolist() == [[0, 0]] and o[5].tolist() == [0]
    wide = const.bond_threshold_table(False, margins=(-10, 5, 2)).to(DEV)          # other margins only change the table
    assert lib.dl_perceive_bonds(ctypes.byref(_lib.DLBondsArgs(**dict(kw, table=wide.data_ptr()))), stream) == 0
    torch.cuda.synchronize()
    assert o[0].tolist() == [0] and o[3].tolist() == [2]


def read_sdf_bonds(path):
    lines = open(path).read().split('\n')
    n_atoms, n_bonds = int(lines[3][0:3]), int(lines[3][3:6])
    assert lines[3].endswith('V2000') and lines[4 + n_atoms + n_bonds] == 'M  END' and lines[5 + n_atoms + n_bonds] == '$$$$'
    return [[int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])] for ln in lines[4 + n_atoms:4 + n_atoms + n_bonds]]


def near_threshold(symbols, pos, is_geom, band=1e-5):
    """A pair within a relative `band` of a threshold of its element pair (CPU, float64)?"""
    from difflinker_amd import const
    table = const.bond_threshold_table(is_geom).numpy()
    idx = [(const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX)[s] for s in symbols]
    d = 100 * np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    return any(t > 0 and abs(d[i, j] / t - 1) < band for i in range(len(idx)) for j in range(i) for t in table[idx[i], idx[j]])


def test_generate_output_format_both(tmp_path, capsys):
    from difflinker_amd import DDPM, io
    from difflinker_amd.generate import generate
    from difflinker_amd.molecule_builder import perceive_bonds
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    seed = 11
    torch.manual_seed(seed)
    plain = generate(frag, ddpm, str(tmp_path / 'plain'), n_samples=3, n_steps=5, linker_size='4')
    assert 'mean_bonds' not in capsys.readouterr().out, 'the default format prints nothing new'
    torch.manual_seed(seed)
    both = generate(frag, ddpm, str(tmp_path / 'both'), n_samples=3, n_steps=5, linker_size='4', output_format='both')
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    torch.manual_seed(seed)
    only = generate(frag, ddpm, str(tmp_path / 'only'), n_samples=3, n_steps=5, linker_size='4', output_format='sdf')
    assert isinstance(both, list)
    assert sorted(os.path.basename(f) for f in both) == sorted(f'output_{i}_frag_{ext}' for i in range(3) for ext in ('.xyz', '.sdf'))
    assert [os.path.basename(f) for f in only] == [f'output_{i}_frag_.sdf' for i in range(3)]
    assert sorted(os.listdir(tmp_path / 'only')) == sorted(os.path.basename(f) for f in only)
    xyz = [f for f in both if f.endswith('.xyz')]
    assert [os.path.basename(f) for f in xyz] == [os.path.basename(f) for f in plain]
    for a, b in zip(plain, xyz):
        assert open(a, 'rb').read() == open(b, 'rb').read(), 'the .xyz files do not depend on the flag'
    counts = []
    for f_xyz, f_sdf, f_only in zip(xyz, [f for f in both if f.endswith('.sdf')], only):
        assert open(f_sdf, 'rb').read() == open(f_only, 'rb').read()
        syms, pos = read_xyz(f_xyz)
        mol = io.read_molecule(f_sdf)
        assert mol.symbols == syms and np.abs(mol.positions - pos).max() <= 5.1e-5
        assert not near_threshold(syms, pos, False) and not near_threshold(syms, mol.positions, False), \
            'pick another seed: a pair sits in the band the 4-decimal rounding could cross'
        _, one_hot, _ = io.parse_molecule(mol, is_geom=False)
        back = perceive_bonds(torch.tensor(one_hot[None], dtype=torch.float32, device=DEV),
                              torch.tensor(mol.positions[None], dtype=torch.float32, device=DEV),
                              torch.ones(1, len(mol), 1, device=DEV), False)
        assert read_sdf_bonds(f_sdf) == back.bonds[0, :int(back.n_bonds[0])].cpu().tolist()
        counts.append((int(back.n_bonds[0]), int(back.n_components[0])))
    assert line['molecules'] == 3
    assert line['mean_bonds'] == pytest.approx(np.mean([c[0] for c in counts]))
    assert line['connected'] == pytest.approx(np.mean([c[1] == 1 for c in counts]))


def test_generate_with_protein_sdf_hides_the_pocket(tmp_path):
    from difflinker_amd import DDPM, io
    from difflinker_amd.generate import generate_with_protein
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(True))
    frag = io.read_molecule(os.path.join(IO_DIR, 'frag.sdf'))
    files = generate_with_protein(os.path.join(IO_DIR, 'frag.sdf'), os.path.join(IO_DIR, 'protein.pdb'), False, ddpm,
                                  str(tmp_path), n_samples=2, n_steps=4, linker_size='3', random_seed=11, output_format='both')
    assert len(files) == 4
    for f_xyz, f_sdf in zip([f for f in files if f.endswith('.xyz')], [f for f in files if f.endswith('.sdf')]):
        mol = io.read_molecule(f_sdf)
        assert mol.symbols == read_xyz(f_xyz)[0] and len(mol) == len(frag) + 3, 'the atoms the .xyz file gets'
        assert all(max(r[:2]) < len(mol) for r in read_sdf_bonds(f_sdf))
