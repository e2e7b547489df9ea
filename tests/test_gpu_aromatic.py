"""Aromatic rings on the GPU (``dl_aromatic_rings``, ``csrc/aromatic.hip``) against the plain-Python rule of
``tests/aromatic_ref.py``: every output is an integer and every comparison is exact, the planarity arithmetic included (fp64,
one rounding per operation on both sides).  The C entry point is called on outputs pre-filled with 0x5a bytes, so an element
it does not write shows.  The public path (``refine_bond_orders``, ``analyze_aromatic``, ``generate``) comes last."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import aromatic_ref as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5a5a5a5a
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read


def classes():
    from difflinker_amd import const
    return ar.ring_class_table(const.ATOM2IDX)


def pack(molecules, width, capacity=None, rng=None):
    """``molecules``: dicts with ``types``, ``points``, ``entries`` and optionally ``dropped`` / ``marked`` atom numbers,
    ``n_in``, ``status``.  With ``rng`` the real rows are scattered over ``width`` and the masks carry garbage on rows that
    are not real; without it they come first."""
    B = len(molecules)
    capacity = max(len(m['entries']) for m in molecules) + 3 if capacity is None else capacity
    out = {'x': np.zeros((B, width, 3), np.float32), 'one_hot': np.zeros((B, width, 8), np.float32),
           'mask': np.zeros((B, width), np.float32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_in': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32),
           'drop': np.zeros((B, width), np.float32), 'mark': np.zeros((B, width), np.float32)}
    out['bonds'][:] = GARBAGE
    if rng is not None:
        out['x'][:] = rng.normal(0, 3, out['x'].shape)
        out['one_hot'][:] = rng.random(out['one_hot'].shape)
        out['drop'][:] = rng.random((B, width)) < 0.5
        out['mark'][:] = rng.random((B, width)) < 0.5
    for b, m in enumerate(molecules):
        n = len(m['types'])
        real = np.arange(n) if rng is None else np.sort(rng.choice(width, n, replace=False))
        out['mask'][b, real] = 1
        if n:
            out['x'][b, real] = np.asarray(m['points'], dtype=np.float64).reshape(n, 3)
            out['one_hot'][b, real] = 0
            out['one_hot'][b, real, m['types']] = 1
        for key, atoms in (('drop', m.get('dropped', [])), ('mark', m.get('marked', []))):
            out[key][b, real] = 0                                       # on real rows exactly what the molecule says
            out[key][b, real[np.asarray(atoms, dtype=int)]] = 1
        rows = m['entries']
        if rows:
            out['bonds'][b, :len(rows)] = rows
        out['n_in'][b] = m.get('n_in', len(rows))
        out['status'][b] = m.get('status', 0)
    return out


def mol(triple, **more):
    types, points, entries = triple
    return dict(types=list(types), points=list(points), entries=list(entries), **more)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def launch(batch, drop=True, mark=True, tol=(ar.TOL2_RING, ar.TOL2_SUB)):
    """The C entry point on outputs full of 0x5a bytes: a dict of int32 numpy arrays by the names of ``aromatic_ref.FIELDS``."""
    from difflinker_amd import _lib
    B, N = batch['mask'].shape
    capacity = batch['bonds'].shape[1]
    held = [dev(batch['x']), dev(batch['one_hot']), dev(batch['mask']), dev(batch['drop']), dev(batch['mark']),
            dev(classes(), torch.int32), dev(batch['n_in'], torch.int32), dev(batch['bonds'], torch.int32),
            dev(batch['status'], torch.int32)]
    x, one_hot, mask, drop_t, mark_t, table, n_in, bonds, status_in = held
    shapes = {'order_out': (B, capacity), 'bond_aromatic': (B, capacity), 'atom_aromatic': (B, N), 'valence_out': (B, N)}
    out = {name: torch.full(shapes.get(name, (B,)), FILL, dtype=torch.int32, device=DEV) for name in ar.FIELDS}
    ptr = lambda t: t.data_ptr() if t.numel() else None      # noqa: E731
    args = _lib.DLAromaticArgs(
        B=B, N=N, nf=8, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=mask.data_ptr(),
        drop_mask=drop_t.data_ptr() if drop else None, mark_mask=mark_t.data_ptr() if mark else None, ring_class=table.data_ptr(),
        capacity=capacity, n_bonds_in=n_in.data_ptr(), bonds=ptr(bonds), status_in=status_in.data_ptr(),
        tol2_ring=tol[0], tol2_sub=tol[1], order_out=ptr(out['order_out']), bond_aromatic=ptr(out['bond_aromatic']),
        atom_aromatic=out['atom_aromatic'].data_ptr(), valence_out=out['valence_out'].data_ptr(),
        n_planar_rings=out['n_planar_rings'].data_ptr(), n_aromatic_rings=out['n_aromatic_rings'].data_ptr(),
        n_aromatic_marked=out['n_aromatic_marked'].data_ptr(), status=out['status'].data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(_lib.load().dl_aromatic_rings(ctypes.byref(args), stream), 'dl_aromatic_rings')
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def reference(batch, drop=True, mark=True, tol=(ar.TOL2_RING, ar.TOL2_SUB)):
    return ar.aromatic_rings(batch['x'], batch['one_hot'], batch['mask'], batch['bonds'], batch['n_in'], classes(),
                             batch['status'], batch['drop'] if drop else None, batch['mark'] if mark else None, *tol)


def check(batch, **kwargs):
    got, want = launch(batch, **kwargs), reference(batch, **kwargs)
    for name in ar.FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == np.int32
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5].tolist())
    return got


def row(batch, b):
    return {key: value[b:b + 1] for key, value in batch.items()}


@pytest.fixture(scope='module')
def hand():
    names = sorted(ar.HAND)
    molecules = [mol(ar.hand_molecule(name)) for name in names] + [mol(([], [], []))]
    return names, pack(molecules, 16, rng=np.random.default_rng(0))


@pytest.fixture(scope='module')
def fused():
    rng = np.random.default_rng(21)
    molecules = []
    for _ in range(64):
        types, points, entries = ar.random_fused(rng)
        marked = [k for k in range(len(types)) if rng.random() < 0.7]
        molecules.append(dict(types=types, points=points, entries=entries, marked=marked))
    return pack(molecules, 40, rng=rng)


@pytest.mark.parametrize('name', sorted(ar.HAND))
def test_hand_molecule_alone(name):
    types, points, entries, want = ar.HAND[name]
    got = check(pack([mol((types, points, entries))], len(types)), drop=False, mark=False)
    assert (got['n_planar_rings'][0], got['n_aromatic_rings'][0], got['status'][0]) == (want['planar'], want['aromatic'], 0)
    doubles = sorted((min(i, j), max(i, j)) for (i, j, _), order in zip(entries, got['order_out'][0]) if order == 2)
    assert doubles == want['doubles']


def test_hand_molecules_in_one_ragged_batch(hand):
    names, batch = hand
    got = check(batch)
    assert batch['mask'].shape == (16, 16)
    for b, name in enumerate(names):
        want = ar.HAND[name][3]
        assert (got['n_planar_rings'][b], got['n_aromatic_rings'][b]) == (want['planar'], want['aromatic']), name
    assert got['n_planar_rings'][-1] == 0 and got['status'][-1] == 0, 'the empty molecule'
    check(batch, drop=False, mark=False)
    assert np.all(launch(batch, mark=False)['n_aromatic_marked'] == 0)


def test_case_study_molecules():
    from difflinker_amd import const
    from difflinker_amd.io import read_sdf_molecules
    molecules = []
    for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', '**', '*.sdf'), recursive=True)):
        for m in read_sdf_molecules(path)[0]:
            molecules.append(dict(types=[const.ATOM2IDX[s] for s in m.symbols], points=m.positions,
                                  entries=[(i, j, 1 if order == 4 else order) for i, j, order in m.bonds]))
    assert molecules and max(len(m['types']) for m in molecules) <= 48
    got = check(pack(molecules, 48, rng=np.random.default_rng(2)), drop=False)
    assert got['n_aromatic_rings'].sum() == got['n_planar_rings'].sum() == 29 and not got['status'].any()


def test_random_fused_systems(fused):
    got = check(fused)
    assert got['n_planar_rings'].sum() > 64 and 0 < got['n_aromatic_rings'].sum() < got['n_planar_rings'].sum()
    assert got['n_aromatic_marked'].sum() > 0 and (got['order_out'] == 2).sum() > 64
    check(fused, tol=(0.02 ** 2, 0.2 ** 2))      # tighter than the noise: other rings pass, the same agreement


def test_every_order_of_the_list_gives_the_same_bits(fused):
    rng = np.random.default_rng(5)
    base = launch(fused)
    shuffled = {key: value.copy() for key, value in fused.items()}
    orders = []
    for b in range(len(fused['n_in'])):
        order = rng.permutation(int(fused['n_in'][b]))
        flip = rng.random(len(order)) < 0.5
        rows = fused['bonds'][b, order]
        rows[flip] = rows[flip][:, [1, 0, 2]]
        shuffled['bonds'][b, :len(order)] = rows
        orders.append(order)
    got = check(shuffled)
    for b, order in enumerate(orders):
        assert np.array_equal(got['order_out'][b, :len(order)], base['order_out'][b, order])
        assert np.array_equal(got['bond_aromatic'][b, :len(order)], base['bond_aromatic'][b, order])
    for name in ar.PER_MOLECULE:
        assert np.array_equal(got[name], base[name])


def test_each_molecule_alone_equals_its_row(fused, hand):
    for batch, rows in ((fused, range(0, 64, 7)), (hand[1], range(16))):
        whole = launch(batch)
        for b in rows:
            alone = launch(row(batch, b))
            for name in ar.FIELDS:
                assert np.array_equal(alone[name][0], whole[name][b]), (name, b)


def test_pocket_rows_are_dropped():
    """N = 300: 30 ligand atoms among 270 pocket atoms that are dropped, some of them bonded to the ligand."""
    rng = np.random.default_rng(9)
    molecules = []
    for _ in range(4):
        types, points, entries = ar.random_fused(rng, max_atoms=30)
        n, total = len(types), len(types) + 270
        number = np.sort(rng.choice(total, n, replace=False))           # the ligand's atom numbers among the pocket's
        pocket = np.setdiff1d(np.arange(total), number)
        all_types, all_points = rng.integers(0, 3, total), rng.normal(0, 6, (total, 3))
        all_types[number], all_points[number] = types, points
        listed = [(int(number[i]), int(number[j]), o) for i, j, o in entries]
        listed += [(int(p), int(number[rng.integers(n)]), 1) for p in pocket[:40]]       # pocket - ligand
        listed += [(int(pocket[k]), int(pocket[k + 1]), 2) for k in range(40, 200)]     # pocket - pocket
        rng.shuffle(listed)
        molecules.append(dict(types=all_types.tolist(), points=all_points, entries=listed, dropped=pocket.tolist(),
                              marked=number.tolist()))
    batch = pack(molecules, 300, rng=rng)
    got = check(batch)
    assert got['n_planar_rings'].sum() > 0 and not got['status'].any()
    alone = reference(pack([mol(ar.random_fused(np.random.default_rng(9), max_atoms=30))], 30))
    assert got['n_planar_rings'][0] == alone['n_planar_rings'][0], 'the pocket changes nothing'


def test_too_many_kept_atoms_leave_the_neighbours_alone():
    chain = ([0] * 257, np.arange(257 * 3).reshape(257, 3) * 0.5, [(k + 1, k, 1 + k % 3) for k in range(256)] + [(5, 5, 1)])
    batch = pack([mol(ar.hand_molecule('benzene')), mol(chain), mol(ar.hand_molecule('naphthalene'))], 300,
                 rng=np.random.default_rng(4))
    got = check(batch, drop=False)
    assert got['status'].tolist() == [0, ar.TOO_LARGE | ar.BAD_BOND, 0] and got['n_aromatic_rings'].tolist() == [1, 0, 2]
    assert got['order_out'][1, :257].tolist() == [1 + k % 3 for k in range(256)] + [0] and not got['valence_out'][1].any()
    chain256 = ([0] * 256, chain[1][:256], chain[2][:255])
    got = check(pack([mol(chain256)], 1024, rng=np.random.default_rng(4)), drop=False)
    assert got['status'].tolist() == [0], '256 kept atoms among 1024 rows fit'


def test_non_finite_coordinates_are_not_planar():
    types, points, entries = ar.hand_molecule('naphthalene')
    molecules = []
    for value in (float('nan'), float('inf'), -float('inf')):
        bad = [list(p) for p in points]
        bad[3][1] = value                         # atom 3 lies in the first ring only
        molecules.append(mol((types, bad, entries)))
    sub = [list(p) for p in ar.HAND['pyridone'][1]]
    sub[7][2] = float('inf')                      # the carbonyl oxygen: a substituent
    molecules.append(mol((ar.HAND['pyridone'][0], sub, ar.HAND['pyridone'][2])))
    got = check(pack(molecules, 12), drop=False, mark=False)
    assert got['n_planar_rings'].tolist() == [1, 1, 1, 0] and got['n_aromatic_rings'].tolist() == [1, 1, 1, 0]


def test_bad_entries_set_the_bit_and_are_skipped():
    types, points, entries = ar.hand_molecule('biphenyl')
    wrong = [(0, 1, 0), (0, 1, 4), (3, 3, 1), (-1, 2, 1), (2, 12, 1)]
    repeated = [(1, 0, 3), (9, 0, 2), (0, 9, 3)]
    molecules = [mol((types, points, entries + [w])) for w in wrong + repeated]
    molecules.append(mol((types, points, wrong + repeated[::-1] + entries + repeated)))
    molecules.append(mol((types, points, entries)))
    got = check(pack(molecules, 14, rng=np.random.default_rng(8)), drop=False)
    assert got['status'].tolist() == [ar.BAD_BOND] * 9 + [0]
    assert got['order_out'][:8, len(entries)].tolist() == [0, 0, 0, 0, 0, 2, 2, 3], 'a ring pair\'s order; outside the rings its own'
    assert got['n_aromatic_rings'][:8].tolist() == [2] * 8
    clean = got['valence_out'][9]
    assert all(np.array_equal(got['valence_out'][b], clean) for b in range(8)), 'a repeated pair counts once'
    # in the ninth list the FIRST entry of the link (0, 9) has order 3: both its ends are X, five P are left in either ring
    assert got['order_out'][8, 5:8].tolist() == [3, 2, 1] and got['n_aromatic_rings'][8] == 0


def test_counts_beyond_the_capacity_and_below_zero():
    types, points, entries = ar.hand_molecule('benzene')
    molecules = [mol((types, points, entries), n_in=9, status=2), mol((types, points, entries), n_in=-3),
                 mol((types, points, entries), n_in=4)]
    got = check(pack(molecules, 8, capacity=6), drop=False)
    assert got['status'].tolist() == [2 | ar.BONDS_OVERFLOW, 0, 0] and got['n_planar_rings'].tolist() == [1, 0, 0]
    assert got['order_out'][1].tolist() == [0] * 6 and got['order_out'][2].tolist() == [1, 1, 1, 1, 0, 0]


def test_capacity_zero_and_a_null_list():
    types, points, _ = ar.hand_molecule('benzene')
    batch = pack([mol((types, points, []), n_in=6), mol(([], [], []))], 8, capacity=0)
    got = check(batch)
    assert got['order_out'].shape == (2, 0) and got['status'].tolist() == [ar.BONDS_OVERFLOW, 0]
    assert not got['valence_out'].any() and not got['n_planar_rings'].any()


def test_system_limit():
    """33 atoms in one system (seven hexagons and a pentagon in a strip) keep their orders; 30 atoms are assigned; the
    benzene beside them is untouched by either."""
    big, fits = ar.strip(8, last=5), ar.strip(7)
    assert len(big[0]) == 33 and len(fits[0]) == 30
    benzene = ar.hand_molecule('benzene')
    both = (big[0] + benzene[0], list(big[1]) + [(p[0], p[1] + 9.0, 0.0) for p in benzene[1]],
            [(i, j, 2) for i, j, _ in big[2]] + [(i + 33, j + 33, o) for i, j, o in benzene[2]])
    got = check(pack([mol(big), mol(fits), mol(both)], 40, rng=np.random.default_rng(6)), drop=False)
    assert got['status'].tolist() == [ar.BIG_SYSTEM, 0, ar.BIG_SYSTEM]
    assert got['n_planar_rings'].tolist() == [8, 7, 9] and got['n_aromatic_rings'].tolist() == [0, 7, 1]
    assert set(got['order_out'][2, :len(big[2])].tolist()) == {2}, 'the input orders of the large system'
    assert sorted(got['order_out'][2, len(big[2]):len(both[2])].tolist()) == [1, 1, 1, 2, 2, 2]


def test_ring_limit():
    """65 planar rings (a 5 x 13 flake of the honeycomb) pass through; 64 (8 x 8) are counted, in one system too large."""
    many, most = ar.flake(5, 13), ar.flake(8, 8)
    got = check(pack([mol(many), mol(most), mol(ar.hand_molecule('pyridine'))], 176, rng=np.random.default_rng(12)), drop=False)
    assert got['status'].tolist() == [ar.MANY_RINGS, ar.BIG_SYSTEM, 0] and got['n_planar_rings'].tolist() == [0, 64, 1]
    assert got['n_aromatic_rings'].tolist() == [0, 0, 1] and not got['bond_aromatic'][:2].any()
    assert got['valence_out'][0].max() == 3 and set(got['order_out'][0, :len(many[2])].tolist()) == {1}


def test_empty_batch_launches_nothing():
    batch = pack([mol(ar.hand_molecule('benzene'))], 8)
    got = launch({key: value[:0] for key, value in batch.items()})
    assert all(got[name].shape[0] == 0 for name in ar.FIELDS)


# ---- the public path -------------------------------------------------------------------------------------------------------
def test_refined_5ou2_fragment_through_the_sdf_writer(tmp_path):
    """The 5OU2 fragments at their file coordinates: the distance table makes all six benzene bonds double; refined, every
    benzene carbon carries exactly one, nobody is over its valence, and the file written without refinement is unchanged."""
    from difflinker_amd import const
    from difflinker_amd.io import read_sdf_molecules, save_sdf_file
    from difflinker_amd.metrics import molecule_keys
    from difflinker_amd.molecule_builder import perceive_all_bonds, refine_bond_orders
    path = os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', 'impdh', '5ou2_fragments_input.sdf')
    source = read_sdf_molecules(path)[0][0]
    n = len(source.symbols)
    batch = pack([dict(types=[const.ATOM2IDX[s] for s in source.symbols], points=source.positions, entries=[])], n + 3)
    one_hot, x, mask = dev(batch['one_hot']), dev(batch['x']), dev(batch['mask']).unsqueeze(2)
    found = perceive_all_bonds(one_hot, x, mask, False)
    refined, aromatic = refine_bond_orders(found, one_hot, x, mask, False)
    assert refined._fields == found._fields and refined.bonds.shape == found.bonds.shape
    assert torch.equal(refined.n_bonds, found.n_bonds) and torch.equal(refined.bonds[:, :, :2], found.bonds[:, :, :2])
    for name, bonds in (('distance', found), ('geometric', refined)):
        os.makedirs(tmp_path / name)
        save_sdf_file(str(tmp_path / name), one_hot, x, mask, bonds.bonds, bonds.n_bonds, names=['m'], is_geom=False)
    again = read_sdf_molecules(str(tmp_path / 'geometric' / 'm_.sdf'))[0][0]
    before = read_sdf_molecules(str(tmp_path / 'distance' / 'm_.sdf'))[0][0]
    assert again.symbols == source.symbols and [b[:2] for b in again.bonds] == [b[:2] for b in before.bonds]
    adj = {k: set() for k in range(n)}
    for i, j, _ in again.bonds:
        adj[i].add(j)
        adj[j].add(i)
    benzenes = [c for c in ar.candidate_rings(adj, {k: True for k in adj}) if len(c) == 6 and all(again.symbols[a] == 'C' for a in c)]
    assert benzenes and int(aromatic.n_aromatic_rings[0]) >= len(benzenes)
    inside = lambda bonds, c, a: sorted(o for i, j, o in bonds if a in (i, j) and i in c and j in c)      # noqa: E731
    assert any(all(inside(before.bonds, c, a) == [2, 2] for a in c) for c in benzenes), 'the table: six double bonds in a ring'
    assert all(inside(again.bonds, c, a) == [1, 2] for c in benzenes for a in c), 'refined: one double bond per carbon'
    valence = [0] * n
    for i, j, o in again.bonds:
        assert o in (1, 2, 3)
        valence[i] += o
        valence[j] += o
    assert all(valence[k] <= const.ALLOWED_BONDS[s] for k, s in enumerate(again.symbols))
    assert refined.valence[0, :n].tolist() == valence
    assert int(molecule_keys(one_hot, mask, refined, False).n_over[0]) == 0 < int(molecule_keys(one_hot, mask, found, False).n_over[0])
    want = reference(dict(batch, bonds=found.bonds.cpu().numpy(), n_in=found.n_bonds.cpu().numpy(),
                          status=found.status.cpu().numpy()), drop=False, mark=False)
    assert np.array_equal(refined.bonds[:, :, 2].cpu().numpy(), want['order_out'])
    assert np.array_equal(aromatic.bond_aromatic.cpu().numpy(), want['bond_aromatic'])


def test_compute_aromatic_on_a_batch_with_a_known_answer():
    from difflinker_amd.metrics import AROMATIC_NAMES, analyze_aromatic, aromatic_to_host, compute_aromatic
    names = ('benzene', 'cyclopentadiene', 'cyclohexane_chair')
    batch = pack([mol(ar.hand_molecule(name)) for name in names], 8)
    one_hot, x, mask = dev(batch['one_hot']), dev(batch['x']), dev(batch['mask'])
    result = analyze_aromatic(one_hot, x, mask, False, mask)
    assert result.refined.n_bonds.tolist() == [6, 5, 6], 'the rings and nothing else are bonded at these distances'
    records = aromatic_to_host(result)
    assert [r.n_aromatic_linker for r in records] == [1, 0, 0] and [r.n_filtered_bonds for r in records] == [0, 2, 0]
    got = compute_aromatic(records)
    assert list(got) == list(AROMATIC_NAMES)
    assert got['ring_filter'] == 2 / 3 and got['aromatic_rings_n'] == 1 / 3 and got['valence_validity_geometric'] == 1.0
    assert (got['aromatic_molecules'], got['aromatic_flagged']) == (3, 0)
    nothing_marked = aromatic_to_host(analyze_aromatic(one_hot, x, mask, False, torch.zeros_like(mask)))
    assert [r.n_aromatic_linker for r in nothing_marked] == [0, 0, 0] and [r.n_aromatic for r in nothing_marked] == [1, 0, 0]
    json.dumps(compute_aromatic(records, records))


def test_generate_switches(tmp_path):
    """``generate`` without the switches writes what it wrote before; ``bond_orders='geometric'`` changes bond orders only, and
    ``aromatic=True`` adds the three scores to ``metrics.json``."""
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.io import read_sdf_molecules
    from difflinker_amd.metrics import AROMATIC_NAMES
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    runs = {'plain': {}, 'distance': dict(bond_orders='distance'), 'geometric': dict(bond_orders='geometric', aromatic=True)}
    files = {}
    for name, more in runs.items():
        torch.manual_seed(11)
        written = generate(frag, ddpm, str(tmp_path / name), n_samples=3, n_steps=5, linker_size='4', output_format='sdf', **more)
        files[name] = [open(path).read() for path in written]
    assert len(files['plain']) == 3 and files['plain'] == files['distance']
    assert not os.path.exists(tmp_path / 'plain' / 'metrics.json')
    got = json.load(open(tmp_path / 'geometric' / 'metrics.json'))
    assert list(got) == list(AROMATIC_NAMES) and got['aromatic_molecules'] + got['aromatic_flagged'] == 3
    for k in range(3):
        a = read_sdf_molecules(str(tmp_path / 'plain' / f'output_{k}_frag_.sdf'))[0][0]
        b = read_sdf_molecules(str(tmp_path / 'geometric' / f'output_{k}_frag_.sdf'))[0][0]
        assert a.symbols == b.symbols and np.array_equal(a.positions, b.positions)
        assert [e[:2] for e in a.bonds] == [e[:2] for e in b.bonds] and all(e[2] in (1, 2, 3) for e in b.bonds)


TRUE_KEYS = {'true_aromatic_rings_n', 'true_ring_filter', 'true_valence_validity_geometric'}


def check_scores(got, n_samples):
    from difflinker_amd.metrics import AROMATIC_NAMES
    assert set(AROMATIC_NAMES) | TRUE_KEYS <= set(got)
    assert got['aromatic_molecules'] + got['aromatic_flagged'] == n_samples and type(got['aromatic_molecules']) is int
    if got['aromatic_molecules']:
        assert all(0.0 <= got[k] <= 1.0 for k in ('ring_filter', 'valence_validity_geometric')) and got['aromatic_rings_n'] >= 0.0
        assert got['true_aromatic_rings_n'] == 0.0 and got['true_ring_filter'] == 1.0, 'the toy molecules are chains'
    json.dumps(got)


def test_sample_switches(tmp_path):
    """``sample``: the three scores beside the others only when asked for, and ``.sdf`` files that differ from the default ones
    in bond orders at most."""
    from difflinker_amd.metrics import AROMATIC_NAMES, METRIC_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_rings import gentle_model
    m = gentle_model(tmp_path, False)
    m.edm.noise_seed = 5
    out = sample(m, str(tmp_path / 'new'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, aromatic=True,
                 output_format='sdf', bond_orders='geometric')
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | set(AROMATIC_NAMES) | TRUE_KEYS
    check_scores(got, 5 * 2)
    m.edm.noise_seed = 5
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True,
                   output_format='sdf')
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}
    files = sorted(glob.glob(os.path.join(plain, '*', '*_.sdf')))
    assert len(files) == 5 * 2
    for path in files:
        a, b = open(path).read().splitlines(), open(path.replace(plain, out)).read().splitlines()
        assert len(a) == len(b) and all(p == q or (p[:6] == q[:6] and len(p.split()) == 7) for p, q in zip(a, b))


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path, pockets):
    from difflinker_amd.metrics import AROMATIC_NAMES, METRIC_NAMES
    from test_gpu_rings import gentle_model
    m = gentle_model(tmp_path, pockets)
    assert m.aromatic_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.aromatic_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(AROMATIC_NAMES) | TRUE_KEYS
    assert {k: got[k] for k in METRIC_NAMES} == plain
    check_scores(got, 5 * 3)
