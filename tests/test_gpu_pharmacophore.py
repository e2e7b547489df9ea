"""``dl_pharmacophore_features`` and ``dl_feature_match`` on the GPU against ``tests/pharmacophore_ref.py``: every comparison is
bit for bit (floats by their bit patterns).  The kernels read the bond list, so the molecules here are lists with coordinates
drawn at random - no geometry has to make chemical sense.  Shapes are small: at most 64 molecules of at most 48 rows, except
where a limit of the kernel (256 kept atoms, 1024 rows, 64 rings) is what the test is about.  The stream contract of the two
wrappers is in ``tests/test_gpu_streams_pharmacophore.py``."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import input_forms as IF
import pharmacophore_ref as pr
import test_gpu_rings as RG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STALE = 0x5a
GARBAGE = (7, 7, 7)                              # what the list holds beyond n_bonds_in: never read
INPUTS = ('one_hot', 'x', 'node_mask', 'bonds', 'n_bonds_in', 'bond_aromatic', 'status_in')
MATCH_INPUTS = ('family', 'position', 'marked', 'n_features')


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def stale(shape, dtype=torch.int32):
    """An output buffer of ``shape`` whose every byte is 0x5a."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if t.numel():
        t.view(torch.uint8).fill_(STALE)
    return t


def tables():
    return dev(pr.FEATURE_CLASS, torch.int32), dev(pr.DEFAULT_VALENCE, torch.int32)


def launch(batch, Fcap, drop=None, mark=None):
    """The C entry on output buffers full of 0x5a bytes, on torch's current stream."""
    from difflinker_amd import _lib
    B, N = batch['node_mask'].shape
    capacity = batch['bonds'].shape[1]
    ins = {name: dev(batch[name], torch.float32 if batch[name].dtype == np.float32 else torch.int32) for name in INPUTS}
    if drop is not None:
        ins['drop_mask'] = dev(drop)
    if mark is not None:
        ins['mark_mask'] = dev(mark)
    ins['feature_class'], ins['default_valence'] = tables()
    out = {'family': stale((B, Fcap)), 'anchor': stale((B, Fcap)), 'position': stale((B, Fcap, 3), torch.float32),
           'marked': stale((B, Fcap)), 'n_features': stale((B,)), 'family_count': stale((B, pr.FAMILIES)), 'status': stale((B,))}
    pointers = {k: v.data_ptr() for k, v in {**ins, **out}.items() if v.numel()}
    args = _lib.DLPharmArgs(B=B, N=N, nf=batch['one_hot'].shape[2], capacity=capacity, Fcap=Fcap,
                            stream=torch.cuda.current_stream().cuda_stream, **pointers)
    _lib.check(_lib.load().dl_pharmacophore_features(ctypes.byref(args)), 'dl_pharmacophore_features')
    return out


def launch_match(a, b, radius2=6.25, marked_only=False):
    """``dl_feature_match`` of two dicts of numpy arrays (``MATCH_INPUTS``) on stale outputs."""
    from difflinker_amd import _lib
    B, Fa = a['family'].shape
    Fb = b['family'].shape[1]
    kind = lambda name: torch.float32 if name == 'position' else torch.int32      # noqa: E731
    ins = {f'{name}_{side}': dev(lists[name], kind(name)) for side, lists in (('a', a), ('b', b)) for name in MATCH_INPUTS}
    out = {'best_index': stale((B, Fb)), 'best_d2': stale((B, Fb), torch.float32), 'n_a': stale((B,)), 'n_b': stale((B,)),
           'n_matched': stale((B,))}
    pointers = {k: v.data_ptr() for k, v in {**ins, **out}.items() if v.numel()}
    args = _lib.DLFeatureMatchArgs(B=B, Fa=Fa, Fb=Fb, radius2=radius2, marked_only=int(marked_only),
                                   stream=torch.cuda.current_stream().cuda_stream, **pointers)
    _lib.check(_lib.load().dl_feature_match(ctypes.byref(args)), 'dl_feature_match')
    return out


def reference_match(a, b, radius2=6.25, marked_only=False):
    return pr.feature_match(*(a[name] for name in MATCH_INPUTS), *(b[name] for name in MATCH_INPUTS), radius2, marked_only)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_exact(got, want, fields, what=''):
    for name in fields:
        g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else np.asarray(got[name])
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, (what, name, g.shape, g.dtype)
        assert np.array_equal(bits(g), bits(want[name])), (what, name, np.argwhere(bits(g) != bits(want[name]))[:5].tolist())


def check(batch, Fcap, drop=None, mark=None, what=''):
    got = launch(batch, Fcap, drop, mark)
    want = pr.batch_features(batch, Fcap, drop, mark)
    assert_exact(got, want, pr.FIELDS, what)
    return want


# ---- molecules ----------------------------------------------------------------------------------------------------------------

def pack(rng, molecules, N, capacity=None, scatter=True):
    """``molecules``: ``(symbols, bonds)`` with bonds ``(i, j, order, aromatic)`` that may be any integers.  Real rows are
    scattered over ``N``; one-hot rows carry smaller garbage beside the 1, the list garbage beyond its length."""
    B = len(molecules)
    capacity = max(len(bonds) for _, bonds in molecules) + 3 if capacity is None else capacity
    out = {'one_hot': (rng.random((B, N, len(pr.TYPE))) * 0.5).astype(np.float32), 'x': rng.normal(0, 2, (B, N, 3)).astype(np.float32),
           'node_mask': np.zeros((B, N), np.float32), 'bonds': np.zeros((B, capacity, 3), np.int32),
           'n_bonds_in': np.zeros(B, np.int32), 'bond_aromatic': rng.integers(0, 2, (B, capacity)).astype(np.int32),
           'status_in': np.zeros(B, np.int32)}
    out['bonds'][:] = GARBAGE
    for b, (symbols, bonds) in enumerate(molecules):
        n = len(symbols)
        out['node_mask'][b] = RG.scattered_rows(rng, n, N) if scatter else (np.arange(N) < n)
        real = np.nonzero(out['node_mask'][b])[0]
        out['one_hot'][b, real, [pr.TYPE[s] for s in symbols]] = 1.0
        rows = bonds[:capacity]
        for e, (i, j, order, aromatic) in enumerate(rows):
            out['bonds'][b, e] = (i, j, order)
            out['bond_aromatic'][b, e] = aromatic
        out['n_bonds_in'][b] = len(bonds)
    return out


def row_mask(batch, atoms_per_molecule):
    """A ``[B,N]`` mask that is 1 on the rows of the given atom numbers and random on the rows that are no atoms."""
    rng = np.random.default_rng(5)
    mask = (rng.random(batch['node_mask'].shape) < 0.5).astype(np.float32)
    for b, atoms in enumerate(atoms_per_molecule):
        real = np.nonzero(batch['node_mask'][b])[0]
        mask[b, real] = 0
        mask[b, real[np.asarray(sorted(atoms), dtype=int)]] = 1
    return mask


def union(parts):
    symbols, bonds = [], []
    for part_symbols, part_bonds in parts:
        bonds += [(i + len(symbols), j + len(symbols), o, a) for i, j, o, a in part_bonds]
        symbols += part_symbols
    return symbols, bonds


def fuzz_molecule(rng):
    """Two to four hand-built molecules joined by random bonds, some orders and aromatic flags changed at random, some pocket
    atoms bonded on, the atoms renumbered and the list shuffled and re-oriented.  Returns ``(symbols, bonds, dropped atoms)``."""
    names = list(pr.EXAMPLES)
    symbols, bonds = union([pr.EXAMPLES[names[k]][:2] for k in rng.integers(0, len(names), rng.integers(2, 5))][:4])
    while len(symbols) > 40:
        symbols, bonds = union([pr.EXAMPLES[names[k]][:2] for k in rng.integers(0, len(names), 2)])
    n = len(symbols)
    pairs = {(min(i, j), max(i, j)) for i, j, _, _ in bonds}
    for _ in range(rng.integers(0, 4)):                                  # bonds between the parts, or chords
        i, j = (int(v) for v in rng.choice(n, 2, replace=False))
        if (min(i, j), max(i, j)) not in pairs:
            pairs.add((min(i, j), max(i, j)))
            bonds.append((i, j, int(rng.integers(1, 4)), int(rng.random() < 0.2)))
    bonds = [(i, j, int(rng.integers(1, 4)) if rng.random() < 0.08 else o, int(not a) if rng.random() < 0.05 else a)
             for i, j, o, a in bonds]
    n_pocket = int(rng.integers(0, 5))
    symbols = symbols + [str(s) for s in rng.choice(['C', 'N', 'O', 'S', 'P', 'F', 'Br'], n_pocket)]
    bonds += [(n + k, int(rng.integers(0, n)), int(rng.integers(1, 3)), int(rng.random() < 0.3)) for k in range(n_pocket)]
    perm = rng.permutation(len(symbols))                                 # old atom k becomes atom perm[k]
    renamed = [None] * len(symbols)
    for k, s in enumerate(symbols):
        renamed[perm[k]] = s
    bonds = [bonds[k] for k in rng.permutation(len(bonds))]
    bonds = [(int(perm[j]), int(perm[i]), o, a) if rng.random() < 0.5 else (int(perm[i]), int(perm[j]), o, a) for i, j, o, a in bonds]
    return renamed, bonds, sorted(int(perm[n + k]) for k in range(n_pocket))


def build_fuzz(seed=2024, B=64, N=48):
    """The fuzz batch, its drop and mark masks, and a second batch of the same graphs whose atoms are moved by about 0.6 A: the
    true molecules of the match."""
    rng = np.random.default_rng(seed)
    molecules = [fuzz_molecule(rng) for _ in range(B)]
    batch = pack(rng, [m[:2] for m in molecules], N)
    drop = row_mask(batch, [m[2] for m in molecules])
    mark = row_mask(batch, [rng.choice(len(m[0]), len(m[0]) // 2, replace=False) for m in molecules])
    moved = dict(batch, x=(batch['x'] + rng.normal(0, 0.6, batch['x'].shape)).astype(np.float32))
    return batch, drop, mark, moved


@pytest.fixture(scope='module')
def fuzz():
    batch, drop, mark, moved = build_fuzz()
    Fcap = 96
    return {'batch': batch, 'drop': drop, 'mark': mark, 'moved': moved, 'Fcap': Fcap,
            'a': pr.batch_features(batch, Fcap, drop, mark), 'b': pr.batch_features(moved, Fcap, drop, mark)}


def honeycomb(rows, columns):
    """A brick-wall patch of ``rows * columns`` six-rings, every atom a carbon and every bond aromatic."""
    width = 2 * columns + 2
    at = lambda r, c: r * width + c      # noqa: E731
    bonds = [(at(r, c), at(r, c + 1), 1, 1) for r in range(rows + 1) for c in range(width - 1)]
    bonds += [(at(r, c), at(r + 1, c), 1, 1) for r in range(rows) for c in range(r % 2, width, 2)]
    return ['C'] * ((rows + 1) * width), bonds


# ---- features -----------------------------------------------------------------------------------------------------------------

def test_hand_built_molecules():
    rng = np.random.default_rng(1)
    names = list(pr.EXAMPLES)
    batch = pack(rng, [pr.EXAMPLES[name][:2] for name in names], 16)
    want = check(batch, 24)
    for b, name in enumerate(names):
        n = int(want['n_features'][b])
        assert list(zip(want['family'][b, :n].tolist(), want['anchor'][b, :n].tolist())) == pr.EXAMPLES[name][2], name
    assert not want['status'].any()


def test_the_fuzz_is_exact_and_covers_every_family(fuzz):
    want = fuzz['a']
    assert (want['family_count'] > 0).sum(0).min() >= 10, 'every family occurs in at least 10 molecules'
    assert not (want['status'] & (pr.OVERFLOW | pr.TOO_LARGE)).any() and want['n_features'].max() <= fuzz['Fcap']
    got = launch(fuzz['batch'], fuzz['Fcap'], fuzz['drop'], fuzz['mark'])
    assert_exact(got, want, pr.FIELDS, 'with both masks')
    check(fuzz['batch'], fuzz['Fcap'], None, None, 'without masks')
    check(fuzz['batch'], fuzz['Fcap'], fuzz['drop'], None, 'without marks')


def test_a_molecule_does_not_depend_on_its_neighbours(fuzz):
    whole = launch(fuzz['batch'], fuzz['Fcap'], fuzz['drop'], fuzz['mark'])
    for rows in ([5], [63, 0, 17]):
        part = {name: fuzz['batch'][name][rows] for name in INPUTS}
        alone = launch(part, fuzz['Fcap'], fuzz['drop'][rows], fuzz['mark'][rows])
        for name in pr.FIELDS:
            assert torch.equal(alone[name].view(torch.int32), whole[name][rows].view(torch.int32)), name


def test_a_permuted_list_gives_identical_outputs(fuzz):
    rng = np.random.default_rng(9)
    batch = {name: fuzz['batch'][name].copy() for name in INPUTS}
    for b in range(batch['bonds'].shape[0]):
        order = rng.permutation(int(batch['n_bonds_in'][b]))
        batch['bonds'][b, :len(order)] = batch['bonds'][b, order][:, [1, 0, 2]]
        batch['bond_aromatic'][b, :len(order)] = batch['bond_aromatic'][b, order]
    got = launch(batch, fuzz['Fcap'], fuzz['drop'], fuzz['mark'])
    assert_exact(got, fuzz['a'], pr.FIELDS)


def test_no_kept_atom_one_row_and_an_empty_batch():
    from difflinker_amd import _lib
    rng = np.random.default_rng(2)
    batch = pack(rng, [([], []), (['N'], []), (['C', 'C'], [(0, 1, 1, 0)])], 4)
    drop = row_mask(batch, [[], [], [0, 1]])                             # the third molecule has atoms and keeps none
    want = check(batch, 3, drop)
    assert want['n_features'].tolist() == [0, 1, 0] and want['family'][1].tolist() == [pr.DONOR, -1, -1]
    one = pack(rng, [(['O'], [])], 1, capacity=0)
    assert check(one, 2)['family'][0].tolist() == [pr.DONOR, pr.ACCEPTOR]
    assert check(one, 0)['status'].tolist() == [pr.OVERFLOW], 'no list at all'
    empty = _lib.DLPharmArgs(B=0, N=4, nf=9, capacity=4, Fcap=4)
    assert _lib.load().dl_pharmacophore_features(ctypes.byref(empty)) == 0


def big_molecule(n_dropped):
    """42 benzene rings and one acetic acid: 256 atoms, with ``n_dropped`` more atoms bonded on that are dropped."""
    symbols, bonds = union([pr.EXAMPLES['benzene'][:2]] * 42 + [pr.EXAMPLES['acetic acid'][:2]])
    bonds += [(256 + k, 6 * k, 1, 0) for k in range(n_dropped)]
    return symbols + ['C'] * n_dropped, bonds


def test_256_kept_atoms_fit_and_257_do_not():
    rng = np.random.default_rng(3)
    fits, over = big_molecule(10), big_molecule(11)
    batch = pack(rng, [fits, over, pr.EXAMPLES['furan'][:2]], 1024)
    drop = row_mask(batch, [range(256, 266), range(257, 267), []])       # 256 and 257 kept atoms
    want = check(batch, 400, drop)
    assert want['status'].tolist() == [0, pr.TOO_LARGE, 0]
    assert want['family_count'][0].tolist() == [1, 2, 0, 1, 42 * 6 + 1, 42, 42] and want['n_features'][0] == 341
    assert want['n_features'][1] == 0 and (want['family'][1] == -1).all() and not want['family_count'][1].any()
    assert want['n_features'][2] == 3, 'the neighbour of a flagged molecule'


def test_a_ring_across_atoms_63_and_64():
    rng = np.random.default_rng(4)
    chain = (['C'] * 61, [(k, k + 1, 1, 0) for k in range(60)])
    symbols, bonds = union([chain, pr.EXAMPLES['pyridine'][:2], pr.EXAMPLES['acetamidine'][:2]])
    want = check(pack(rng, [(symbols, bonds + [(60, 61, 1, 0)])], 96), 128)
    n = int(want['n_features'][0])
    assert want['family'][0, n - 1] == pr.AROMATIC and want['anchor'][0, n - 1] == 61 and want['family_count'][0, pr.AROMATIC] == 1


def test_64_rings_are_listed_and_65_are_not():
    rng = np.random.default_rng(5)
    batch = pack(rng, [honeycomb(8, 8), honeycomb(5, 13)], 200)
    want = check(batch, 300)
    assert want['status'].tolist() == [0, pr.MANY_RINGS]
    assert want['family_count'][0, pr.AROMATIC:].tolist() == [64, 64] and want['family_count'][1, pr.AROMATIC:].tolist() == [0, 0]
    assert want['family_count'][1, pr.HYDROPHOBE] == want['n_features'][1] == 6 * 28, 'the atom features stay'
    rings = want['anchor'][0, 9 * 18:9 * 18 + 128:2].tolist()
    assert rings == sorted(rings) and len(set(rings)) == 64, 'rings in the order of their smallest atom'


def test_the_list_exactly_full_and_one_short():
    rng = np.random.default_rng(6)
    batch = pack(rng, [pr.EXAMPLES['naphthalene'][:2], pr.EXAMPLES['aniline'][:2]], 12)
    full = check(batch, 14)
    assert full['status'].tolist() == [0, 0] and full['n_features'].tolist() == [14, 8]
    short = check(batch, 13)
    assert short['status'].tolist() == [pr.OVERFLOW, 0] and short['n_features'].tolist() == [14, 8]
    assert np.array_equal(short['family'], full['family'][:, :13])


def test_bad_and_repeated_entries():
    rng = np.random.default_rng(7)
    symbols, bonds, _ = pr.EXAMPLES['acetic acid']
    bad = bonds + [(1, 2, 1, 1), (2, 1, 3, 1), (0, 0, 1, 0), (0, 4, 1, 0), (-1, 2, 1, 0), (0, 3, 0, 0), (0, 3, 4, 0)]
    late = [(2, 1, 1, 1)] + bonds                                       # here the first entry of the pair 1-2 says single, aromatic
    batch = pack(rng, [(symbols, bad), (symbols, late), (symbols, bonds)], 6)
    batch['n_bonds_in'][2] = 40                                          # more than the list holds: cut at its capacity
    batch['status_in'][:] = [0, 2, 0]
    want = check(batch, 8)
    assert want['status'].tolist() == [pr.BAD_BOND, pr.BAD_BOND | 2, pr.BONDS_OVERFLOW | pr.BAD_BOND]
    n = int(want['n_features'][0])
    assert list(zip(want['family'][0, :n].tolist(), want['anchor'][0, :n].tolist())) == pr.EXAMPLES['acetic acid'][2]
    assert pr.NEGATIVE not in want['family'][1].tolist(), 'no C=O left'


def test_a_nan_coordinate_is_flagged_and_listed():
    rng = np.random.default_rng(8)
    batch = pack(rng, [pr.EXAMPLES['aniline'][:2], pr.EXAMPLES['aniline'][:2]], 8, scatter=False)
    batch['x'][0, 6] = (np.nan, 1.0, np.inf)                             # the N: no ring atom, so no centroid sees it
    want = check(batch, 10)
    assert want['status'].tolist() == [pr.NONFINITE, 0] and want['n_features'].tolist() == [8, 8]
    assert np.isnan(want['position'][0, 5, 0]) and np.isinf(want['position'][0, 5, 2])


def test_drop_mask_removes_a_pocket():
    rng = np.random.default_rng(10)
    symbols, bonds, _ = pr.EXAMPLES['chlorobenzene']
    pocket = ['N', 'O', 'C', 'S'] * 5
    with_pocket = (pocket + symbols, [(i + 20, j + 20, o, a) for i, j, o, a in bonds] + [(k, 20 + k % 7, 1, 0) for k in range(20)]
                   + [(k, k + 1, 2, 1) for k in range(19)])
    batch = pack(rng, [with_pocket], 40)
    want = check(batch, 16, row_mask(batch, [range(20)]))
    n = int(want['n_features'][0])
    assert list(zip(want['family'][0, :n].tolist(), (want['anchor'][0, :n] - 20).tolist())) == pr.EXAMPLES['chlorobenzene'][2]
    assert check(batch, 64)['n_features'][0] != n, 'with the pocket the features differ'


# ---- the match ----------------------------------------------------------------------------------------------------------------

def lists(family, position, marked=None, n=None):
    family = np.asarray(family, np.int32)
    return {'family': family, 'position': np.asarray(position, np.float32).reshape(family.shape + (3,)),
            'marked': np.ones_like(family) if marked is None else np.asarray(marked, np.int32),
            'n_features': np.asarray([family.shape[1]] * family.shape[0] if n is None else n, np.int32)}


def check_match(a, b, radius2=6.25, marked_only=False, what=''):
    want = reference_match(a, b, radius2, marked_only)
    assert_exact(launch_match(a, b, radius2, marked_only), want, pr.MATCH_FIELDS, what)
    return want


def test_the_fuzz_matches_exactly(fuzz):
    a, b = fuzz['a'], fuzz['b']
    whole = check_match(a, b, what='whole')
    assert (whole['n_matched'] > 0).sum() * 2 >= len(whole['n_matched']), 'at least half of the pairs have a match'
    linker = check_match(a, b, marked_only=True, what='marked only')
    assert (linker['n_a'] <= whole['n_a']).all() and (linker['n_a'] < whole['n_a']).any()
    cut = lambda side, F: {name: side[name] if name == 'n_features' else side[name][:, :F] for name in MATCH_INPUTS}      # noqa: E731
    check_match(a, cut(b, 40), what='capacities differ, a count beyond its list')
    check_match(cut(a, 7), b, what='a short A list')


def test_the_cut_off_is_strict_and_a_tie_goes_to_the_lower_index():
    below = np.nextafter(np.float32(2), np.float32(0))
    assert np.float32(np.float32(1.5 * 1.5) + np.float32(below * below)) == np.nextafter(np.float32(6.25), np.float32(0))
    a = lists([[pr.DONOR, pr.DONOR, pr.ACCEPTOR, pr.ACCEPTOR, pr.AROMATIC, pr.AROMATIC, pr.AROMATIC]],
              [[0, 0, 0], [4, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0]])
    b = lists([[pr.DONOR, pr.ACCEPTOR, pr.AROMATIC, pr.DONOR, pr.HYDROPHOBE]],
              [[1.5, 2, 0], [1.5, below, 0], [0, 0, 0], [2, 0, 0], [0, 0, 0]])
    want = check_match(a, b)
    assert want['best_index'].tolist() == [[-1, 2, 4, 0, -1]]
    assert want['best_d2'][0, 1] == np.nextafter(np.float32(6.25), np.float32(0)) and want['best_d2'][0, 3] == 4.0
    assert (want['n_a'][0], want['n_b'][0], want['n_matched'][0]) == (7, 5, 3)
    wider = check_match(a, b, radius2=float(np.nextafter(np.float32(6.25), np.float32(7))))
    assert wider['best_index'][0, 0] == 0 and wider['best_d2'][0, 0] == 6.25


def test_empty_lists_marks_and_positions_that_are_no_numbers():
    a = lists([[pr.DONOR, pr.DONOR, -1, 7]], [[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0]], marked=[[0, 1, 1, 1]])
    b = lists([[pr.DONOR, pr.DONOR, pr.DONOR]], [[1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], marked=[[1, 0, 1]])
    want = check_match(a, b)
    assert want['best_index'].tolist() == [[0, -1, -1]] and (want['n_a'][0], want['n_b'][0]) == (2, 3)
    marked = check_match(a, b, marked_only=True)
    assert marked['best_index'].tolist() == [[-1, -1, -1]] and (marked['n_a'][0], marked['n_b'][0], marked['n_matched'][0]) == (1, 2, 0)
    for n_a, n_b in ((0, 3), (4, 0), (0, 0), (-3, 9)):
        got = check_match(dict(a, n_features=np.asarray([n_a], np.int32)), dict(b, n_features=np.asarray([n_b], np.int32)))
        assert (got['n_a'][0], got['n_b'][0]) == (min(max(n_a, 0), 2), min(max(n_b, 0), 3)) and got['n_matched'][0] == 0
    none = lists(np.zeros((2, 0), np.int32), np.zeros((2, 0, 3)))
    assert check_match(none, dict(b, **{k: np.repeat(b[k], 2, 0) for k in b}))['n_b'].tolist() == [3, 3]
    assert check_match(dict(a, **{k: np.repeat(a[k], 2, 0) for k in a}), none)['n_a'].tolist() == [2, 2]


def test_more_features_than_a_tile():
    """Lists longer than the 256 features a workgroup stages at a time, and than its 256 lanes."""
    rng = np.random.default_rng(11)
    a = lists(rng.integers(-1, 8, (3, 700)), rng.integers(-4, 5, (3, 700, 3)) * 0.5, rng.integers(0, 2, (3, 700)), [700, 257, 256])
    b = lists(rng.integers(-1, 8, (3, 300)), rng.integers(-4, 5, (3, 300, 3)) * 0.5, rng.integers(0, 2, (3, 300)), [300, 256, 1])
    want = check_match(a, b)
    assert (want['n_matched'] > 0).all()
    check_match(a, b, marked_only=True)


# ---- the wrappers -------------------------------------------------------------------------------------------------------------

def wrapped(fuzz, form=lambda h, device: h.to(device)):      # noqa: B008
    """``pharmacophore_features`` on both fuzz batches and ``feature_match`` of the two, every input through ``form``."""
    from difflinker_amd import metrics
    from difflinker_amd.molecule_builder import Bonds
    place = lambda a: form(torch.as_tensor(a), DEV)      # noqa: E731
    out = []
    for batch in (fuzz['batch'], fuzz['moved']):
        found = Bonds(place(batch['n_bonds_in']), place(batch['bonds']), None, None, None, place(batch['status_in']))
        out.append(metrics.pharmacophore_features(place(batch['one_hot']), place(batch['x']), place(batch['node_mask'][:, :, None]), found,
                                                  place(batch['bond_aromatic']), True, place(fuzz['drop']), place(fuzz['mark']),
                                                  capacity=fuzz['Fcap']))
    fa, fb = out
    reform = lambda f: f._replace(**{name: form(getattr(f, name).cpu(), DEV) for name in MATCH_INPUTS})      # noqa: E731
    return fa, fb, metrics.feature_match(reform(fa), reform(fb)), metrics.feature_match(reform(fa), reform(fb), 2.5, True)


def test_the_python_wrappers_give_the_same(fuzz):
    from difflinker_amd import metrics
    fa, fb, whole, linker = wrapped(fuzz)
    assert_exact(fa._asdict(), fuzz['a'], pr.FIELDS)
    assert_exact(fb._asdict(), fuzz['b'], pr.FIELDS)
    assert_exact(whole._asdict(), reference_match(fuzz['a'], fuzz['b']), pr.MATCH_FIELDS)
    assert_exact(linker._asdict(), reference_match(fuzz['a'], fuzz['b'], marked_only=True), pr.MATCH_FIELDS)
    d2, n_a, n_b = whole.best_d2.cpu().tolist(), whole.n_a.tolist(), whole.n_b.tolist()
    for row, na, nb in zip(d2, n_a, n_b):
        want = None if min(na, nb) == 0 else sum(math.exp(-d) for d in row if d != math.inf) / min(na, nb)
        assert metrics.feature_score(row, na, nb) == want
    default = metrics.pharmacophore_features(dev(fuzz['batch']['one_hot']), dev(fuzz['batch']['x']), dev(fuzz['batch']['node_mask']),
                                             bonds_of(fuzz['batch']), dev(fuzz['batch']['bond_aromatic'], torch.int32), True)
    assert default.family.shape == (64, 3 * 48) and torch.equal(default.n_features.cpu(), torch.from_numpy(
        pr.batch_features(fuzz['batch'], 144)['n_features']))
    empty = metrics.pharmacophore_features(dev(np.zeros((0, 5, 9))), dev(np.zeros((0, 5, 3))), dev(np.zeros((0, 5))),
                                           bonds_of({'n_bonds_in': np.zeros(0), 'bonds': np.zeros((0, 4, 3)), 'status_in': np.zeros(0)}),
                                           dev(np.zeros((0, 4)), torch.int32), True)
    assert empty.family.shape == (0, 16) and metrics.feature_match(empty, empty).best_d2.shape == (0, 16)


def bonds_of(batch):
    from difflinker_amd.molecule_builder import Bonds
    return Bonds(dev(batch['n_bonds_in'], torch.int32), dev(batch['bonds'], torch.int32), None, None, None,
                 dev(batch['status_in'], torch.int32))


@pytest.mark.parametrize('form', ['strided', 'sliced', 'wide'])
def test_the_wrappers_take_the_form(fuzz, form):
    """Strided and sliced views whose gaps hold poison, and int64 / fp64 / bool inputs: the same bits as from dense tensors."""
    fa, fb, whole, linker = wrapped(fuzz, IF.BY_NAME[form])
    assert_exact(fa._asdict(), fuzz['a'], pr.FIELDS, form)
    assert_exact(fb._asdict(), fuzz['b'], pr.FIELDS, form)
    assert_exact(whole._asdict(), reference_match(fuzz['a'], fuzz['b']), pr.MATCH_FIELDS, form)
    assert_exact(linker._asdict(), reference_match(fuzz['a'], fuzz['b'], marked_only=True), pr.MATCH_FIELDS, form)


# ---- the public path ------------------------------------------------------------------------------------------------------------

def test_analyze_pharmacophores_runs_the_whole_chain():
    """Benzoic acid against itself lifted by 1 A out of its plane, bonds perceived from the geometry: every feature of B finds
    its own counterpart at d2 = 1 exactly and the score is exp(-1) (host fp64: a sum of equal terms over their number); the
    linker (the acid group) alone likewise."""
    from difflinker_amd import metrics
    ring = [(1.39 * math.cos(k * math.pi / 3), 1.39 * math.sin(k * math.pi / 3), 0.0) for k in range(6)]
    acid = [(2.89, 0.0, 0.0), (3.50, 1.05, 0.0), (3.60, -1.15, 0.0)]      # C-C 1.50, C=O 1.21, C-O 1.35
    x = np.zeros((1, 12, 3), np.float32)
    x[0, :9] = ring + acid
    one_hot = np.zeros((1, 12, 8), np.float32)
    one_hot[0, :7, 0] = one_hot[0, 7:9, 1] = 1
    mask = (np.arange(12) < 9).astype(np.float32)[None, :, None]
    linker = ((np.arange(12) >= 6) & (np.arange(12) < 9)).astype(np.float32)[None, :, None]
    got = metrics.analyze_pharmacophores(dev(one_hot), dev(x), dev(mask), dev(linker), dev(one_hot), dev(x + np.float32([0, 0, 1])), dev(mask),
                                         dev(linker), is_geom=False)
    n = int(got.features_a.n_features[0])
    families = got.features_a.family[0, :n].tolist()
    assert got.status.tolist() == [0] and got.features_a.family_count[0].tolist() == [1, 2, 0, 1, 6, 1, 1]
    assert families == [pr.HYDROPHOBE] * 6 + [pr.NEGATIVE, pr.ACCEPTOR, pr.DONOR, pr.ACCEPTOR, pr.AROMATIC, pr.LUMPED]
    assert got.whole.n_matched.tolist() == [n] and got.linker.n_a.tolist() == [4]
    assert got.whole.best_d2[0, :n].tolist() == [1.0] * n
    whole, linker_records = metrics.pharmacophores_to_host(got)
    for record, count in ((whole[0], n), (linker_records[0], 4)):
        assert (record.n_a, record.n_b, record.n_matched, record.status) == (count, count, count, 0)
        assert abs(record.score - math.exp(-1.0)) < 1e-12
    scores = metrics.compute_pharmacophores(whole, linker_records)
    assert scores['feature_molecules'] == 1 and abs(scores['feature_similarity_linker'] - math.exp(-1.0)) < 1e-12


def test_sample_writes_the_pharmacophore_keys(tmp_path, monkeypatch):
    from difflinker_amd import metrics
    from difflinker_amd.metrics import METRIC_NAMES, PHARM_NAMES, PHARM_SC_NAMES, SHAPE_NAMES
    from difflinker_amd.sample import sample
    seen = {}
    compute = metrics.compute_pharmacophores
    monkeypatch.setattr(metrics, 'compute_pharmacophores', lambda *records: seen.update(records=records) or compute(*records))
    m = RG.gentle_model(tmp_path, False)
    out = sample(m, str(tmp_path / 'both'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, shape=True, pharmacophore=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == set(SHAPE_NAMES) | {'shape_tanimoto_linker'} | set(PHARM_NAMES) | set(PHARM_SC_NAMES)
    whole, linker, shapes = seen['records']
    assert len(whole) == len(linker) == len(shapes) == 5 * 2 and got['feature_molecules'] + got['feature_flagged'] <= 10
    both = [(p, s) for p, s in zip(whole, shapes) if metrics._pharm_scored(p) and metrics._shape_scored(s)]
    assert both and got['feature_molecules'] > 0, 'the toy molecules carry features'
    sc = [0.5 * p.score + 0.5 * (s.vol_min / s.vol_a) for p, s in both]
    assert got['sc_similarity'] == sum(sc) / len(sc)
    assert [got[f'sc_similarity_{k}'] for k in (7, 8, 9)] == [100.0 * sum(v > bar for v in sc) / len(sc) for bar in (0.7, 0.8, 0.9)]
    scored = [p.score for p in whole if metrics._pharm_scored(p)]
    assert got['feature_similarity'] == sum(scored) / len(scored) and 0.0 < got['feature_similarity'] <= 1.0
    alone = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, pharmacophore=True)
    assert set(json.load(open(os.path.join(alone, 'metrics.json')))) == set(PHARM_NAMES), 'no sc_similarity without the shapes'
    shape_only = sample(m, str(tmp_path / 'shape'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, shape=True)
    assert set(json.load(open(os.path.join(shape_only, 'metrics.json')))) == set(SHAPE_NAMES) | {'shape_tanimoto_linker'}
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}


def test_sample_and_analyze_adds_the_keys_only_when_switched_on(tmp_path):
    from difflinker_amd.metrics import METRIC_NAMES, PHARM_NAMES, PHARM_SC_NAMES, SHAPE_NAMES
    m = RG.gentle_model(tmp_path, True)
    assert m.pharmacophore_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.pharmacophore_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(PHARM_NAMES)
    assert {k: got[k] for k in METRIC_NAMES} == plain
    m.shape_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(PHARM_NAMES) | set(PHARM_SC_NAMES) | set(SHAPE_NAMES) | {'shape_tanimoto_linker',
                                                                                                       'shape_tanimoto_valid'}
    assert got['feature_molecules'] + got['feature_flagged'] <= 5 * 3
    json.dumps(got)
