"""Ring perception on the GPU (``dl_ring_scores``, ``csrc/rings.hip``) against the plain-Python rule of ``tests/rings_ref.py``.
Every output is an integer and every comparison is exact.  The batches are fed as bond lists directly, no geometry needed;
the public path (``analyze_rings``, ``sample(..., rings=True)``, ``generate(..., rings=True)``, ``DDPM.ring_metrics``) comes last."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rings_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = rings_ref.FIELDS
N = 300
KEPT = (1, 2, 3, 63, 64, 65, 128, 129, 255, 256)  # the word boundaries of the bit rows
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read


def scattered_rows(rng, n_real, width):
    mask = np.zeros(width, np.float32)
    mask[np.sort(rng.choice(width, n_real, replace=False))] = 1
    return mask


def union(names):
    """The disjoint union of hand molecules: ``(atoms, pairs)``."""
    atoms, pairs = 0, []
    for name in names:
        n, bonds = rings_ref.HAND[name]
        pairs += [(i + atoms, j + atoms) for i, j in bonds]
        atoms += n
    return atoms, pairs


def random_graph(rng, n_kept, n_dropped, degree=2.2):
    """A random graph of average degree ``degree`` over ``n_kept`` atoms, numbered at random among ``n_dropped`` atoms that
    are dropped and carry one bond each; distinct pairs in random order and orientation.  Returns ``(atoms, pairs, dropped)``."""
    n = n_kept + n_dropped
    dropped = rng.choice(n, n_dropped, replace=False)
    kept = np.setdiff1d(np.arange(n), dropped)
    want = min(int(round(degree * n_kept / 2)), n_kept * (n_kept - 1) // 2)
    pairs = set()
    while len(pairs) < want:
        i, j = (int(v) for v in rng.choice(kept, 2, replace=False))
        if (j, i) not in pairs:
            pairs.add((i, j))
    pairs = sorted(pairs) + [(int(d), int((d + 1 + rng.integers(0, n - 1)) % n)) for d in dropped if n > 1]
    return n, [pairs[k] for k in rng.permutation(len(pairs))], dropped


def pack(rng, molecules, width=N, capacity=None):
    """``molecules``: dicts with ``atoms``, ``pairs`` (or ``entries``) and optionally ``dropped`` / ``marked`` atom numbers,
    ``n_in``, ``status``.  Real rows are scattered over ``width``; masks carry NaN-free garbage on rows that are not real."""
    B = len(molecules)
    lists = [m.get('entries', [(i, j, int(rng.integers(1, 4))) for i, j in m.get('pairs', [])]) for m in molecules]
    capacity = max(len(rows) for rows in lists) + 3 if capacity is None else capacity
    out = {'mask': np.zeros((B, width), np.float32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_in': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32),
           'drop': (rng.random((B, width)) < 0.5).astype(np.float32), 'mark': (rng.random((B, width)) < 0.5).astype(np.float32)}
    out['bonds'][:] = GARBAGE
    for b, (m, rows) in enumerate(zip(molecules, lists)):
        out['mask'][b] = scattered_rows(rng, m['atoms'], width)
        real = np.nonzero(out['mask'][b])[0]
        for key, atoms in (('drop', m.get('dropped', [])), ('mark', m.get('marked', []))):
            out[key][b, real] = 0                                       # on real rows exactly what the molecule says
            out[key][b, real[np.asarray(atoms, dtype=int)]] = 1
        if rows:
            out['bonds'][b, :len(rows)] = rows
        out['n_in'][b] = m.get('n_in', len(rows))
        out['status'][b] = m.get('status', 0)
    return out


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def launch(batch, drop=True, mark=True):
    from difflinker_amd.metrics import ring_scores
    from difflinker_amd.molecule_builder import Bonds
    found = Bonds(dev(batch['n_in'], torch.int32), dev(batch['bonds'], torch.int32), None, None, None, dev(batch['status'], torch.int32))
    return ring_scores(dev(batch['mask']), found, dev(batch['drop']) if drop else None, dev(batch['mark']) if mark else None)


def reference(batch, drop=True, mark=True):
    return rings_ref.ring_scores(batch['mask'], batch['bonds'], batch['n_in'], batch['status'],
                                 batch['drop'] if drop else None, batch['mark'] if mark else None)


def as_dict(got):
    return got if isinstance(got, dict) else {name: getattr(got, name).cpu().numpy() for name in FIELDS}


def assert_exact(got, want, what=''):
    got = as_dict(got)
    for name in FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def build_mixed():
    rng = np.random.default_rng(3)
    names = ['tree', 'cyclopropylbenzene', ('naphthalene', 'norbornane'), ('spiro[4.4]nonane', 'cubane'), 'macrocycle_tail',
             tuple(sorted(rings_ref.HAND))]
    molecules = []
    for k, name in enumerate(names):
        atoms, pairs = union([name] if isinstance(name, str) else name)
        molecules.append({'atoms': atoms, 'pairs': pairs, 'marked': rng.choice(atoms, atoms // 3, replace=False),
                          'status': 2 if k == 1 else 0})
    for n_kept in KEPT:
        n_dropped = min(n_kept // 8 + 1, N - n_kept)
        atoms, pairs, dropped = random_graph(rng, n_kept, n_dropped)
        molecules.append({'atoms': atoms, 'pairs': pairs, 'dropped': dropped, 'marked': rng.choice(atoms, atoms // 3, replace=False)})
    return names, molecules, pack(rng, molecules)


@pytest.fixture(scope='module')
def mixed():
    names, molecules, batch = build_mixed()
    return {'names': names, 'molecules': molecules, 'batch': batch, 'want': reference(batch)}


def test_mixed_batch_is_exact(mixed):
    batch, want = mixed['batch'], mixed['want']
    assert len(batch['mask']) == 16 and batch['bonds'].shape[1] > 256
    assert want['n_atoms'][6:].tolist() == list(KEPT) and (want['status'] == [0, 2] + [0] * 14).all()
    for b, name in enumerate(mixed['names']):                          # the hand molecules: the answers known beforehand
        parts = [name] if isinstance(name, str) else name
        answers = [rings_ref.HAND_ANSWERS[p] for p in parts]
        n_bonds = int(batch['n_in'][b])
        assert sorted(want['bond_ring'][b, :n_bonds].tolist()) == sorted(sum((a[0] for a in answers), []))
        assert want['n_rings'][b] == sum(a[1] for a in answers) and want['n_components'][b] == len(parts)
    sizes = set(want['bond_ring'][6:].ravel().tolist())
    assert {0, 3, 4, 5, 6, 7}.issubset(sizes) and max(sizes) >= 8, 'the random graphs hold rings of many sizes'
    assert want['n_components'][-1] > 1 and want['n_rings'][-1] > 1 and (want['ring_hist'][-7:, 1, 1:].sum(1) > 0).all()
    assert_exact(launch(batch), want, 'mixed')
    # without the optional masks: nothing dropped, nothing marked
    for drop, mark in ((False, True), (True, False), (False, False)):
        got = launch(batch, drop, mark)
        assert_exact(got, reference(batch, drop, mark), f'drop {drop} mark {mark}')
        if not mark:
            assert int(got.ring_hist[:, 1].abs().sum()) == 0
    assert int(launch(batch, False, False).status[-1]) == rings_ref.TOO_LARGE, '256 kept + 33 dropped atoms, none dropped'


def test_every_order_of_the_list_gives_the_same_bits(mixed):
    rng = np.random.default_rng(4)
    batch, want = mixed['batch'], mixed['want']
    shuffled = {k: v.copy() for k, v in batch.items()}
    moved = want['bond_ring'].copy()
    for b in range(len(batch['mask'])):
        n = int(batch['n_in'][b])
        perm = rng.permutation(n)
        flip = rng.random(n) < 0.5
        rows = batch['bonds'][b, :n][perm]
        rows[flip] = rows[flip][:, [1, 0, 2]]                           # either orientation
        shuffled['bonds'][b, :n] = rows
        moved[b, :n] = want['bond_ring'][b, :n][perm]
    got = as_dict(launch(shuffled))
    for name in rings_ref.PER_MOLECULE:
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got['bond_ring'], moved), 'permuted with the list'
    again = as_dict(launch(batch))
    for name in FIELDS:                                                 # two launches: the same bits
        assert np.array_equal(again[name], want[name]), name


def test_more_entries_than_threads():
    rng = np.random.default_rng(5)
    atoms, pairs, dropped = random_graph(rng, 90, 10, degree=13.0)
    assert len(pairs) == 595
    sparse = random_graph(rng, 200, 0, degree=2.9)
    batch = pack(rng, [{'atoms': atoms, 'pairs': pairs, 'dropped': dropped, 'marked': range(0, 100, 3)},
                       {'atoms': sparse[0], 'pairs': sparse[1]}])
    want = reference(batch)
    assert want['n_bonds'][0] > 512 and set(want['bond_ring'][0].tolist()) <= {0, 3, 4} and want['n_bonds'][1] == 290
    assert_exact(launch(batch), want, 'stride')


def test_capacity_zero_and_a_null_list():
    rng = np.random.default_rng(6)
    batch = pack(rng, [{'atoms': 5, 'dropped': [1]}, {'atoms': 1}, {'atoms': 40, 'n_in': 7, 'status': 2}], width=64, capacity=0)
    assert batch['bonds'].shape == (3, 0, 3)
    want = reference(batch)
    assert want['n_components'].tolist() == [4, 1, 40] and want['status'].tolist() == [0, 0, 2 | rings_ref.BONDS_OVERFLOW]
    got = launch(batch)
    assert got.bond_ring.shape == (3, 0)
    assert_exact(got, want, 'capacity 0')


def test_too_many_kept_atoms_leave_the_neighbours_alone(mixed):
    rng = np.random.default_rng(7)
    atoms, pairs, _ = random_graph(rng, 257, 0)
    small = [mixed['molecules'][1], mixed['molecules'][9]]
    batch = pack(rng, [small[0], {'atoms': atoms, 'pairs': pairs, 'status': 2, 'marked': range(50)}, small[1]])
    want = reference(batch)
    got = launch(batch)
    assert_exact(got, want, '257')
    assert got.status.tolist() == [2, 2 | rings_ref.TOO_LARGE, 0] and int(got.n_atoms[1]) == 257
    for name in FIELDS[1:7]:
        assert int(getattr(got, name)[1].abs().sum()) == 0, name
    assert want['n_rings'][0] == 2 and want['n_atoms'][2] == 63
    # the same 257 atoms with one of them dropped fit
    fits = pack(rng, [{'atoms': atoms, 'pairs': pairs, 'dropped': [100], 'marked': range(50)}])
    want = reference(fits)
    assert want['n_atoms'][0] == 256 and want['status'][0] == 0 and want['n_rings'][0] > 0
    assert_exact(launch(fits), want, '257 less one')


def test_256_kept_atoms_among_1024_rows():
    rng = np.random.default_rng(8)
    atoms, pairs, dropped = random_graph(rng, 256, 700)
    batch = pack(rng, [{'atoms': atoms, 'pairs': pairs, 'dropped': dropped, 'marked': rng.choice(atoms, 300, replace=False)},
                       {'atoms': 1024, 'pairs': rings_ref.ring(9, 1000) + [(0, 1023)], 'dropped': range(256, 990)}], width=1024)
    want = reference(batch)
    assert want['n_atoms'].tolist() == [256, 290] and want['status'].tolist() == [0, rings_ref.TOO_LARGE]
    assert want['n_rings'][0] > 0 and want['atom_ring'][0].max() > 0
    assert_exact(launch(batch), want, 'N = 1024')
    batch['drop'][1, 0:40] = 1                                          # every row is real here: 250 kept atoms
    want = reference(batch)
    assert want['n_atoms'][1] == 250 and want['n_rings'][1] == 1 and sorted(set(want['bond_ring'][1].tolist())) == [0, 9]
    assert_exact(launch(batch), want, 'N = 1024, all rows real')


def test_bad_entries_set_the_bit_and_are_skipped():
    rng = np.random.default_rng(9)
    square = [(0, 1, 1), (1, 2, 2), (2, 3, 3), (3, 0, 1)]
    cases = [[(2, 2, 1)], [(0, 6, 1)], [(-1, 2, 1)], [(0, 2, 0)], [(0, 2, 4)], [(1, 2, 1)], [(2, 1, 3)], [(4, 5, 1)], []]
    molecules = [{'atoms': 6, 'entries': square[:2] + extra + square[2:], 'dropped': [5]} for extra in cases]
    molecules.append({'atoms': 6, 'entries': [(j, i, o) for i, j, o in square]})       # i < j everywhere: as good as j < i
    batch = pack(rng, molecules, width=40)
    want = reference(batch)
    bad = rings_ref.BAD_BOND
    assert want['status'].tolist() == [bad] * 7 + [0, 0, 0], 'a bond to a dropped atom is no error'
    assert [row[:5].tolist() for row in want['bond_ring'][:8]] == [[4, 4, 0, 4, 4]] * 5 + [[4] * 5] * 2 + [[4, 4, 0, 4, 4]]
    assert want['n_bonds'].tolist() == [4] * 10 and want['n_rings'].tolist() == [1] * 10
    got = launch(batch)
    assert_exact(got, want, 'bad entries')


def test_counts_beyond_the_capacity_and_below_zero():
    rng = np.random.default_rng(10)
    atoms, pairs = rings_ref.HAND['naphthalene']
    molecules = [{'atoms': atoms, 'pairs': pairs, 'n_in': n_in, 'status': status}
                 for n_in, status in ((11, 0), (12, 0), (1 << 30, 2), (-1, 0), (-(1 << 31), 2), (10, 0), (0, 0))]
    batch = pack(rng, molecules, width=33, capacity=11)
    want = reference(batch)
    over = rings_ref.BONDS_OVERFLOW
    assert want['status'].tolist() == [0, over, over | 2, 0, 2, 0, 0]
    assert want['n_rings'].tolist() == [2, 2, 2, 0, 0, 1, 0] and want['n_components'].tolist() == [1, 1, 1, 10, 10, 1, 10]
    assert_exact(launch(batch), want, 'counts')


@pytest.mark.parametrize('fill', [0x7f, 0xa5])
def test_c_entry_writes_every_element_of_stale_buffers(mixed, fill):
    """The C entry on output buffers that hold ``fill`` bytes; the rows that are not real hold NaN in the optional masks."""
    from difflinker_amd import _lib
    batch, want = mixed['batch'], mixed['want']
    B, capacity = batch['bonds'].shape[:2]
    drop, mark = batch['drop'].copy(), batch['mark'].copy()
    drop[batch['mask'] == 0] = np.nan
    mark[batch['mask'] == 0] = np.nan
    ins = {'node_mask': dev(batch['mask']), 'drop_mask': dev(drop), 'mark_mask': dev(mark), 'n_bonds_in': dev(batch['n_in'], torch.int32),
           'bonds': dev(batch['bonds'], torch.int32), 'status_in': dev(batch['status'], torch.int32)}
    out = {name: torch.full(want[name].shape + (4,), fill, dtype=torch.uint8, device=DEV) for name in FIELDS}
    args = _lib.DLRingsArgs(B=B, N=N, capacity=capacity, **{k: v.data_ptr() for k, v in ins.items()},
                            **{k: v.data_ptr() for k, v in out.items()})
    _lib.check(_lib.load().dl_ring_scores(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'rings')
    torch.cuda.synchronize()
    assert_exact({name: out[name].view(torch.int32).squeeze(-1).cpu().numpy() for name in FIELDS}, want, 'stale')


def test_single_molecule_and_empty_batch(mixed):
    from difflinker_amd.metrics import ring_scores
    from difflinker_amd.molecule_builder import Bonds
    batch, want = mixed['batch'], mixed['want']
    one = launch({k: v[3:4] for k, v in batch.items()})
    assert_exact(one, {name: want[name][3:4] for name in FIELDS}, 'one molecule')
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)     # noqa: E731
    none = ring_scores(torch.zeros(0, 5, 1, device=DEV), Bonds(i32(0), i32(0, 20, 3), None, None, None, i32(0)))
    assert none.n_rings.shape == (0,) and none.bond_ring.shape == (0, 20) and none.atom_ring.shape == (0, 5)


# ---- the public path ------------------------------------------------------------------------------------------------------

def polygon(k, centre, side=1.5):
    """A regular ``k``-gon of carbon-carbon single-bond sides in the xy plane."""
    radius = side / (2 * np.sin(np.pi / k))
    angle = 2 * np.pi * np.arange(k) / k
    return np.stack([radius * np.cos(angle), radius * np.sin(angle), np.zeros(k)], 1) + np.asarray(centre, float)


def geometric_batch():
    """Three all-carbon molecules, rows ``[fragment..., pocket..., linker...]``, width 16:
    0  a six-ring of fragment atoms, and 8 A away a three-ring of linker atoms
    1  a four-ring, two atoms fragment and two linker: a ring closed through the fragment
    2  a five-ring of linker atoms next to a five-ring of pocket atoms sharing no atom (10 A away), fragment a two-atom chain"""
    width, nf = 16, 8
    x, mask = np.full((3, width, 3), 50.0, np.float32), np.zeros((3, width), np.float32)
    linker, pocket = np.zeros((3, width), np.float32), np.zeros((3, width), np.float32)
    parts = [[(polygon(6, (0, 0, 0)), None), (polygon(3, (8, 0, 0)), linker)],
             [(polygon(4, (0, 0, 0))[:2], None), (polygon(4, (0, 0, 0))[2:], linker)],
             [(np.array([[20.0, 0, 0], [21.5, 0, 0]]), None), (polygon(5, (10, 0, 0)), pocket), (polygon(5, (0, 0, 0)), linker)]]
    for b, rows in enumerate(parts):
        at = 1 if b == 2 else 0                                         # a padding row in front as well
        for pos, flags in rows:
            x[b, at:at + len(pos)], mask[b, at:at + len(pos)] = pos, 1
            if flags is not None:
                flags[b, at:at + len(pos)] = 1
            at += len(pos)
    one_hot = np.zeros((3, width, nf), np.float32)
    one_hot[:, :, 0] = 1
    return one_hot, x, mask, linker, pocket


def test_analyze_rings_on_a_geometric_batch():
    from difflinker_amd.metrics import analyze_rings, compute_rings, rings_to_host
    one_hot, x, mask, linker, pocket = geometric_batch()
    ligand, alone = analyze_rings(dev(one_hot), dev(x), dev(mask)[:, :, None], False, dev(linker)[:, :, None], drop_mask=dev(pocket))
    found = ligand.bonds
    assert alone.bonds is found and found.n_bonds.tolist() == [9, 4, 11], 'one perception for both views'
    lists = (mask, found.bonds.cpu().numpy(), found.n_bonds.cpu().numpy(), found.status.cpu().numpy())
    assert_exact(ligand, rings_ref.ring_scores(*lists, drop_mask=pocket, mark_mask=linker), 'ligand view')
    assert_exact(alone, rings_ref.ring_scores(*lists, drop_mask=1 - linker), 'linker view')
    assert ligand.n_rings.tolist() == [2, 1, 1] and alone.n_rings.tolist() == [1, 0, 1]
    assert ligand.n_atoms.tolist() == [9, 4, 7] and alone.n_atoms.tolist() == [3, 2, 5]
    assert ligand.ring_hist[:, 1].tolist() == [[0, 3, 0, 0, 0, 0, 0], [0, 0, 3, 0, 0, 0, 0], [0, 0, 0, 5, 0, 0, 0]]
    records = rings_to_host(ligand, alone)
    assert [tuple(r) for r in records] == [(1, 2, [0, 3, 0, 0, 0, 0, 0], 0), (0, 1, [0, 0, 3, 0, 0, 0, 0], 0), (1, 1, [0, 0, 0, 5, 0, 0, 0], 0)]
    scores = compute_rings(records)
    assert scores['rings_n'] == 2 / 3 and scores['small_ring'] == 2 / 3 and scores['ring_bonds_5'] == 5 / 11


def gentle_model(tmp_path, pockets):
    """The toy model and data set of ``test_gpu_metrics`` with a noise schedule that ends at alpha_T^2 = 0.05 instead of 1e-5,
    as ``test_gpu_shape`` sets it up: the untrained denoiser then leaves the linker atoms within some tens of A."""
    from difflinker_amd.noise import PredefinedNoiseSchedule
    from test_gpu_metrics import toy_model
    m = toy_model(tmp_path, pockets)
    m.edm.gamma = PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=0.05).to(DEV)
    return m


def check_scores(got, n_samples, with_true):
    from difflinker_amd.metrics import RING_NAMES
    assert set(RING_NAMES) <= set(got) and (('true_rings_n' in got) == ('rings_n_match' in got) == with_true)
    assert got['ring_molecules'] + got['ring_flagged'] == n_samples and type(got['ring_molecules']) is int
    if got['ring_molecules']:
        assert 0.0 <= got['ring_free'] <= 1.0 and 0.0 <= got['small_ring'] <= 1.0 and 0.0 <= got['macrocycle'] <= 1.0
        assert 0.0 <= got['rings_n'] <= got['rings_n_ligand'], 'a ring of the linker alone is a ring of the ligand'
        if with_true:
            assert got['true_rings_n'] == 0.0, 'the toy molecules are chains'
            assert got['rings_n_match'] == got['ring_free']
    json.dumps(got)


def test_sample_writes_the_ring_keys(tmp_path):
    from difflinker_amd.metrics import METRIC_NAMES, RING_NAMES
    from difflinker_amd.sample import sample
    m = gentle_model(tmp_path, False)
    ring_keys = set(RING_NAMES) | {'true_rings_n', 'rings_n_match'}
    out = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, rings=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == ring_keys, 'alone when metrics are not asked for'
    check_scores(got, 5 * 2, True)
    both = sample(m, str(tmp_path / 'both'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, rings=True)
    got = json.load(open(os.path.join(both, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | ring_keys
    check_scores(got, 5 * 2, True)
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}


def test_generate_writes_the_ring_keys(tmp_path):
    from difflinker_amd import DDPM
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import RING_NAMES
    from test_gpu_generate import IO_DIR, ddpm_hparams
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(False))
    frag = os.path.join(IO_DIR, 'frag.sdf')
    torch.manual_seed(11)
    generate(frag, ddpm, str(tmp_path / 'rings'), n_samples=3, n_steps=5, linker_size='4', rings=True)
    got = json.load(open(tmp_path / 'rings' / 'metrics.json'))
    assert set(got) == set(RING_NAMES), 'no true molecule here'
    check_scores(got, 3, False)
    torch.manual_seed(11)
    generate(frag, ddpm, str(tmp_path / 'plain'), n_samples=3, n_steps=5, linker_size='4')
    assert not os.path.exists(tmp_path / 'plain' / 'metrics.json')


def rings_by_hand(m):
    """The ring part of ``sample_and_analyze`` spelled out: the same chains in the same order, one bond perception per batch,
    the lists scored by ``rings_ref`` on the host."""
    from difflinker_amd.metrics import RingRecord, compute_rings
    from difflinker_amd.molecule_builder import perceive_all_bonds
    from test_gpu_metrics import DDPM_sample_chain

    def records(one_hot, x, node_mask, linker, drop):
        found = perceive_all_bonds(one_hot, x, node_mask, m.is_geom)
        B = len(x)
        flat = lambda t: None if t is None else t.reshape(B, -1).cpu().numpy()      # noqa: E731
        lists = (flat(node_mask), found.bonds.cpu().numpy(), found.n_bonds.cpu().numpy(), found.status.cpu().numpy())
        ligand = rings_ref.ring_scores(*lists, drop_mask=flat(drop), mark_mask=flat(linker))
        alone = rings_ref.ring_scores(*lists, drop_mask=1 - flat(linker))
        return [RingRecord(int(alone['n_rings'][b]), int(ligand['n_rings'][b]), ligand['ring_hist'][b, 1].tolist(),
                           int(ligand['status'][b] | alone['status'][b])) for b in range(B)]

    pred, true = [], []
    for data in m.val_dataloader():
        drop = data['pocket_mask'] if m.pockets else None
        true_batch = records(data['one_hot'][:, :, :m.num_classes], data['positions'], data['atom_mask'], data['linker_mask'], drop)
        for _ in range(m.n_stability_samples):
            chain, node_mask = DDPM_sample_chain(m, data)
            assert node_mask.shape == data['atom_mask'].shape, 'the true sizes: the template is as wide as the input'
            pred += records(chain[0][:, :, 3:3 + m.num_classes], chain[0][:, :, :3], node_mask, data['linker_mask'], drop)
            true += true_batch
    return compute_rings(pred, true), pred


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path, pockets):
    from difflinker_amd.metrics import METRIC_NAMES, RING_NAMES
    m = gentle_model(tmp_path, pockets)
    assert m.ring_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.ring_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(RING_NAMES) | {'true_rings_n', 'rings_n_match'}
    assert {k: got[k] for k in METRIC_NAMES} == plain
    check_scores(got, 5 * 3, True)
    m.edm.noise_seed = 5
    want, pred = rings_by_hand(m)
    assert {k: v for k, v in got.items() if k not in METRIC_NAMES} == want
    assert len(pred) == 5 * 3
