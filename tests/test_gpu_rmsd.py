"""The symmetry-aware RMSD on the GPU (csrc/rmsd.hip) against the fp64 helper ``rmsd_ref`` (Kabsch by SVD over maps found by
plain recursion): degenerate point sets, a mirror image, map tables that cross a wave and a workgroup, flagged pairs next to
good ones, and ``analyze -> to_host -> compute_geometry`` on the case-study molecules.

All kernel cases go into ONE list of pairs of mixed atom counts (so padding and the ragged offsets are exercised), scored three
times by a module fixture: as it is, once more (the same bits), and without its flagged pairs (the same bits for the others).

BOUND.  The worst absolute error of ``rmsd`` against the helper over the cases of this file, measured on an MI355X, is
6.3e-8 A (the mirror-image pair, RMSD 2.0 A: half an fp32 ulp of the result there is 1.2e-7 A); the bound is 4 x that, rounded
up to one digit: 3e-7 A.  The margin is for other boxes and seeds; the helper is the ground truth, not the kernel.  It is far
inside the 5e-4 A that half a unit of the reference's printed third decimal allows, and self-alignments (true RMSD 0) fall under
the same bound.  Per-case errors: profiles/rmsd/README.md; the first test prints them again.
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

import rmsd_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 3e-7
HERE = os.path.dirname(os.path.abspath(__file__))


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))                              # proper


def moved(points, rng, shift=50.0, noise=0.0):
    """A rotated copy, translated by ``shift`` A (the scale of pocket coordinates), with per-atom noise; fp32 as the kernel
    reads it - the helper gets the same rounded numbers."""
    t = rng.normal(size=3)
    out = points @ rotation(rng).T + shift * t / np.linalg.norm(t) + noise * rng.normal(size=points.shape)
    return out.astype(np.float32)


def point_sets():
    rng = np.random.default_rng(7)
    angle = np.arange(6) * np.pi / 3
    return {'one': np.zeros((1, 3)), 'two': np.array([[0.0, 0, 0], [1.5, 0, 0]]),
            'collinear': np.array([[0.0, 0, 0], [1.5, 0, 0], [3.1, 0, 0]]),
            'ring': np.stack([1.39 * np.cos(angle), 1.39 * np.sin(angle), np.zeros(6)], 1),
            'generic': 2.0 * rng.normal(size=(7, 3)), 'chiral': 2.0 * rng.normal(size=(5, 3))}


RING_MAPS = [[(s * k + r) % 6 for k in range(6)] for s in (1, -1) for r in range(6)]      # the 12 symmetries of a six-ring


def build_cases():
    """``[(name, a, b, maps, planted)]``: fp32 ``[n,3]`` sets, the pair's maps, and the index ``best`` must name (or None)."""
    rng = np.random.default_rng(2024)
    sets = point_sets()
    cases = []
    for name in ('one', 'two', 'collinear', 'ring', 'generic'):
        a = sets[name].astype(np.float32)
        maps = RING_MAPS if name == 'ring' else [list(range(len(a)))]
        cases.append((f'{name}/self', a, moved(sets[name], rng), maps, None))
        cases.append((f'{name}/noise', a, moved(sets[name], rng, noise=0.3), maps, None))
    chiral = sets['chiral'].astype(np.float32)
    cases.append(('chiral/mirror', chiral, moved(sets['chiral'] * [1.0, 1.0, -1.0], rng), [list(range(5))], 0))
    # map tables over the 7 points: random permutations, the one true correspondence planted last
    generic = sets['generic']
    for size in (1, 12, 65, 257):
        true = rng.permutation(7).tolist()
        b = np.empty((7, 3), np.float32)
        b[true] = moved(generic, rng, noise=0.1)                      # atom k of a is atom true[k] of b
        wrong = []
        while len(wrong) < size - 1:
            perm = rng.permutation(7).tolist()
            if perm != true:
                wrong.append(perm)
        cases.append((f'table{size}', generic.astype(np.float32), b, wrong + [true], size - 1))
        early = max(0, (size - 1) // 2)                               # the same table with the true map also earlier
        cases.append((f'table{size}/twice', generic.astype(np.float32), b, wrong[:early] + [true] + wrong[early:] + [true], early))
    return cases


def launch(cases, n_max, extra=()):
    """One ``best_rmsd`` call over ``cases``; ``extra`` are ``(position, n_atoms, a, b, maps)`` rows put in as they are."""
    from difflinker_amd.metrics import best_rmsd, pack_maps
    rows = [(len(a), a, b, maps) for _, a, b, maps, _ in cases]
    for position, n, a, b, maps in sorted(extra, key=lambda e: e[0]):
        rows.insert(position, (n, a, b, maps))
    xa, xb = torch.zeros(len(rows), n_max, 3), torch.zeros(len(rows), n_max, 3)
    for p, (n, a, b, _) in enumerate(rows):
        xa[p, :len(a)], xb[p, :len(b)] = torch.from_numpy(a), torch.from_numpy(b)
    table, offsets = pack_maps([maps for _, _, _, maps in rows], n_max)
    n_atoms = torch.tensor([n for n, _, _, _ in rows], dtype=torch.int32)
    out = best_rmsd(xa.to(DEV), xb.to(DEV), n_atoms.to(DEV), table.to(DEV), offsets.to(DEV))
    return tuple(t.cpu() for t in out)


N_MAX = 9                                                             # wider than the widest molecule: padding is exercised
BAD_AT = {'no_map': 3, 'nan': 8, 'too_large': 14, 'nan_b': 22}        # positions of the flagged pairs in the full list


@pytest.fixture(scope='module')
def scored():
    cases = build_cases()
    want = [rmsd_ref.best_rmsd(a, b, maps) for _, a, b, maps, _ in cases]          # the reference, computed once
    seven = point_sets()['generic'].astype(np.float32)
    nan_a, nan_b = seven.copy(), seven.copy()
    nan_a[4, 1] = np.nan
    nan_b[6, 2] = np.inf
    ident = [list(range(7))]
    extra = [(BAD_AT['no_map'], 7, seven, seven, []), (BAD_AT['nan'], 7, nan_a, seven, ident),
             (BAD_AT['too_large'], N_MAX + 1, seven, seven, ident), (BAD_AT['nan_b'], 7, seven, nan_b, ident * 70)]
    full = launch(cases, N_MAX, extra)
    again = launch(cases, N_MAX, extra)
    clean = launch(cases, N_MAX)
    good = [p for p in range(len(cases) + len(extra)) if p not in BAD_AT.values()]
    return dict(cases=cases, want=want, full=full, again=again, clean=clean, good=good)


def test_every_case_within_the_bound_of_the_helper(scored):
    rmsd, best, status = scored['clean']
    assert rmsd.dtype == torch.float32 and best.dtype == torch.int32 and status.dtype == torch.int32
    assert status.tolist() == [0] * len(scored['cases'])
    worst = 0.0
    for p, ((name, a, _, maps, planted), (value, index)) in enumerate(zip(scored['cases'], scored['want'])):
        err = abs(float(rmsd[p]) - value)
        worst = max(worst, err)
        print(f'{name:18s} n {len(a)} maps {len(maps):3d}  helper {value:.9f} (map {index})  kernel {float(rmsd[p]):.9f} '
              f'(map {int(best[p])})  error {err:.2e}')
    print(f'worst absolute error {worst:.3e} A, bound {BOUND:.0e} A')
    assert worst <= BOUND


def test_self_alignment_scores_zero_and_a_mirror_image_does_not(scored):
    rmsd = scored['clean'][0]
    by_name = {case[0]: (float(rmsd[p]), scored['want'][p][0]) for p, case in enumerate(scored['cases'])}
    for name in ('one', 'two', 'collinear', 'ring', 'generic'):
        got, want = by_name[f'{name}/self']
        assert want < 1e-5 and abs(got - want) <= BOUND, 'a copy rotated and moved 50 A away: 0 up to the fp32 rounding of the input'
        got, want = by_name[f'{name}/noise']
        assert abs(got - want) <= BOUND and (name == 'one' or want > 0.01)
    got, want = by_name['chiral/mirror']
    assert want > 0.1 and abs(got - want) <= BOUND, 'a solver that allowed reflections would answer 0'


def test_planted_maps_win_and_ties_go_to_the_lowest_index(scored):
    rmsd, best, _ = scored['clean']
    seen = set()
    for p, (name, _, _, maps, planted) in enumerate(scored['cases']):
        if planted is None:
            continue
        value, index = scored['want'][p]
        assert index == planted, 'the helper agrees that the planted map is the best one (the first of equal ones)'
        assert int(best[p]) == planted, name
        assert abs(float(rmsd[p]) - value) <= BOUND
        seen.add(len(maps))
    assert {1, 12, 65, 257} <= seen and {13, 66, 258} <= seen, 'tables on both sides of a wave and of a 256-thread workgroup'
    by_name = {case[0]: p for p, case in enumerate(scored['cases'])}
    for size in (1, 12, 65, 257):
        assert float(rmsd[by_name[f'table{size}']]) == float(rmsd[by_name[f'table{size}/twice']]), 'the same map, the same bits'


def test_flagged_pairs_are_nan_and_leave_their_neighbours_alone(scored):
    from difflinker_amd import _lib
    rmsd, best, status = scored['full']
    want = {'no_map': _lib.DL_RMSD_NO_MAP, 'nan': _lib.DL_RMSD_NONFINITE, 'too_large': _lib.DL_RMSD_TOO_LARGE,
            'nan_b': _lib.DL_RMSD_NONFINITE}
    for name, p in BAD_AT.items():
        assert int(status[p]) == want[name] and np.isnan(float(rmsd[p])) and int(best[p]) == -1, name
    good = scored['good']
    assert status[good].tolist() == [0] * len(good)
    for got, clean in zip(scored['full'], scored['clean']):
        assert torch.equal(got[good], clean), 'bit-identical to a launch without the flagged pairs'


def test_two_launches_give_the_same_bits(scored):
    for first, second in zip(scored['full'], scored['again']):
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))     # as bits: NaN equals NaN


# ---- analyze -> to_host -> compute_geometry on the case-study molecules ------------------------------------------------

N_LINK, COPIES, JITTER = 3, 3, 0.02


def bond_rule(types, pos, table):
    """``get_bond_order`` over the numeric table on the CPU (as tests/test_bonds_host.py restates it): the bonds and, for every
    pair, how far in pm its distance is from the nearest threshold."""
    bonds, margin = [], np.inf
    for i in range(len(types)):
        for j in range(i):
            d = np.float32(100) * np.linalg.norm(pos[i].astype(np.float32) - pos[j].astype(np.float32))
            t = table[types[i]][types[j]]
            order = 0
            if d < t[0]:
                order = 1
                if d < t[1]:
                    order = 2
                    if d < t[2]:
                        order = 3
            margin = min([margin] + [abs(d - v) for v in t if v > 0])
            if order:
                bonds.append((i, j, order))
    return bonds, margin


def case_study_pieces():
    """The files hold fragment pairs and triples, and a true molecule in several pieces is dropped by the scores like any
    invalid one; so every connected piece of at least six atoms is taken as a molecule of its own."""
    from difflinker_amd import const
    from difflinker_amd.io import parse_molecule, read_molecule
    table = const.bond_threshold_table(True).numpy()
    pieces = []
    for path in sorted(glob.glob(os.path.join(HERE, 'golden', 'io', 'case_studies', '*.sdf'))):
        pos, one_hot, _ = parse_molecule(read_molecule(path), True)
        types = one_hot.argmax(1).tolist()
        bonds, _ = bond_rule(types, pos, table)
        label = list(range(len(types)))
        for _ in types:
            for i, j, _o in bonds:
                label[i] = label[j] = min(label[i], label[j])
        for root in sorted(set(label)):
            atoms = [k for k in range(len(types)) if label[k] == root]
            if len(atoms) >= 6:
                pieces.append(([types[k] for k in atoms], pos[atoms].astype(np.float32)))
    return pieces


def test_case_study_molecules_end_to_end():
    from difflinker_amd import const
    from difflinker_amd.metrics import analyze, compute_geometry, kept_positions, to_host
    pieces = case_study_pieces()
    assert len(pieces) >= 4
    table = const.bond_threshold_table(True).numpy()
    rng = np.random.default_rng(31)
    rows = []                                                          # (true types, true pos, pred types, pred pos, counted)
    for types, pos in pieces:
        bonds, margin = bond_rule(types, pos, table)
        count = len(rmsd_ref.isomorphisms(types, bonds, types, bonds, limit=65537))
        assert 1 <= count <= 65536 and margin > 0.05, 'checked on the CPU first: the enumeration is not cut'
        n = len(types)
        for _ in range(COPIES):
            perm = rng.permutation(n)                                  # atom k of the true molecule is atom perm[k] of the copy
            copy_types = [0] * n
            for k in range(n):
                copy_types[perm[k]] = types[k]
            expected = sorted((min(perm[i], perm[j]), max(perm[i], perm[j]), o) for i, j, o in bonds)
            for _attempt in range(100):                                # seeded noise, drawn again while it crosses a bond threshold
                noisy = pos.astype(np.float64)
                noisy[n - N_LINK:] += JITTER * rng.normal(size=(N_LINK, 3))        # the "linker": the last atoms
                copy_pos = np.empty((n, 3), np.float32)
                copy_pos[perm] = moved(noisy, rng, shift=20.0)
                again, margin = bond_rule(copy_types, copy_pos, table)
                if sorted((min(i, j), max(i, j), o) for i, j, o in again) == expected and margin > 0.01:
                    break
            else:
                raise AssertionError('no jitter keeps the bonds')
            rows.append((types, pos, copy_types, copy_pos, True))
    types, pos = pieces[0]
    other = list(types)
    other[0] = (other[0] + 1) % 3                                      # another element: a different molecule
    rows.append((types, pos, other, pos.copy(), False))

    B, N = len(rows), max(len(r[0]) for r in rows) + 2
    true_h, pred_h = torch.zeros(B, N, 9), torch.zeros(B, N, 9)
    true_x, pred_x, mask = torch.zeros(B, N, 3), torch.zeros(B, N, 3), torch.zeros(B, N, 1)
    for b, (tt, tp, pt, pp, _) in enumerate(rows):
        n = len(tt)
        true_h[b, torch.arange(n), torch.tensor(tt)] = 1
        pred_h[b, torch.arange(n), torch.tensor(pt)] = 1
        true_x[b, :n], pred_x[b, :n], mask[b, :n] = torch.from_numpy(tp), torch.from_numpy(pp), 1
    true_h, pred_h, true_x, pred_x, mask = (t.to(DEV) for t in (true_h, pred_h, true_x, pred_x, mask))
    true = to_host(analyze(true_h, true_x, mask, True), true_h, mask)
    pred = to_host(analyze(pred_h, pred_x, mask, True), pred_h, mask)
    assert all(m.n_over == 0 and m.n_components == 1 and m.status == 0 for m in true), 'the pieces are valid molecules'
    n_linker = [N_LINK] * B
    got = compute_geometry(pred, true, list(kept_positions(pred_x, mask)[0]), list(kept_positions(true_x, mask)[0]), n_linker)

    values, scale = [], 0.0
    for b, (tt, tp, pt, pp, counted) in enumerate(rows):
        if not counted:
            continue
        maps = rmsd_ref.isomorphisms(pred[b].graph.types, pred[b].graph.bonds, true[b].graph.types, true[b].graph.bonds)
        assert maps, 'a renumbered, moved and slightly jittered copy is the same molecule'
        values.append(rmsd_ref.best_rmsd(pp, tp, maps)[0] * np.sqrt(len(tt) / N_LINK))
        scale = max(scale, np.sqrt(len(tt) / N_LINK))
    want = float(np.mean(values))
    print(f'{len(values)} recovered copies of {len(pieces)} pieces: helper {want:.9f}, compute_geometry {got}')
    assert got['rmsd_molecules'] == len(values) == len(pieces) * COPIES and type(got['rmsd_molecules']) is int
    assert got['rmsd_truncated'] == 0 and type(got['rmsd']) is float
    assert 0.0 < want < 0.2 and abs(got['rmsd'] - want) <= BOUND * scale, 'every term is an rmsd times at most `scale`'
    # a cut enumeration is counted, and the pair is still scored over the maps found
    few = compute_geometry(pred[:1], true[:1], list(kept_positions(pred_x[:1], mask[:1])[0]),
                           list(kept_positions(true_x[:1], mask[:1])[0]), n_linker[:1], max_matches=1)
    full = len(rmsd_ref.isomorphisms(pred[0].graph.types, pred[0].graph.bonds, true[0].graph.types, true[0].graph.bonds))
    assert few['rmsd_molecules'] == 1 and few['rmsd_truncated'] == int(full > 1) and few['rmsd'] >= values[0] - BOUND * scale


# ---- the callers ------------------------------------------------------------------------------------------------------

def test_sample_writes_the_three_keys_only_when_asked(tmp_path):
    from difflinker_amd.metrics import GEOMETRY_NAMES, METRIC_NAMES
    from difflinker_amd.sample import sample
    from test_gpu_metrics import toy_model
    m = toy_model(tmp_path, False)
    out = sample(m, str(tmp_path / 'geo'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True, geometry=True)
    got = json.load(open(os.path.join(out, 'metrics.json')))
    assert set(got) == set(METRIC_NAMES) | {'molecules'} | set(GEOMETRY_NAMES) and got['molecules'] == 5 * 2
    assert type(got['rmsd_molecules']) is int and type(got['rmsd_truncated']) is int
    assert 0 <= got['rmsd_truncated'] <= got['rmsd_molecules'] <= 5 * 2
    assert (got['rmsd'] is None) == (got['rmsd_molecules'] == 0)
    assert got['rmsd'] is None or got['rmsd'] >= 0.0
    plain = sample(m, str(tmp_path / 'plain'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, metrics=True)
    assert set(json.load(open(os.path.join(plain, 'metrics.json')))) == set(METRIC_NAMES) | {'molecules'}
    alone = sample(m, str(tmp_path / 'alone'), 'zinc_final_test', 2, DEV, data=str(tmp_path), n_steps=5, geometry=True)
    assert not os.path.exists(os.path.join(alone, 'metrics.json')), 'geometry rides on --metrics'


@pytest.mark.parametrize('pockets', [False, True])
def test_sample_and_analyze_adds_the_keys_when_switched_on(tmp_path, pockets):
    from difflinker_amd.metrics import GEOMETRY_NAMES, METRIC_NAMES
    from test_gpu_metrics import toy_model
    m = toy_model(tmp_path, pockets)
    assert m.geometry_metrics is False
    m.edm.noise_seed = 5
    plain = m.sample_and_analyze(m.val_dataloader())
    assert set(plain) == set(METRIC_NAMES)
    m.geometry_metrics = True
    m.edm.noise_seed = 5
    got = m.sample_and_analyze(m.val_dataloader())
    assert set(got) == set(METRIC_NAMES) | set(GEOMETRY_NAMES) and {k: got[k] for k in METRIC_NAMES} == plain
    assert (got['rmsd'] is None) == (got['rmsd_molecules'] == 0) and type(got['rmsd_molecules']) is int
    json.dumps(got)
