"""Frame and numbering independence on the host (no GPU): the clearance condition of every fixed case, the restatements held to
the contract themselves - the check of the rules as written - the teeth of the comparison, and the transforms.  The cases,
transforms, bars and the cap are stated in ``tests/frame_cases.py``; ``tests/test_gpu_frames.py`` holds the kernels to the same."""
import math
import re

import numpy as np
import pytest

import aromatic_ref as ar
import clash_ref
import frame_cases as fc
import hydrogens_ref as hr

BASE = {}
CASES = [(e.name, c) for e in fc.ENTRIES + fc.CHAINS for c in e.case_names()]


def restatement(entry, inputs, run):
    return entry.reference(inputs, run)


# ---- 1. clearance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,case_name', CASES)
def test_every_decision_clears_its_threshold_under_every_transform(entry, case_name):
    e = fc.ENTRY_POINTS[entry]
    case, lowest = e.case(case_name), math.inf
    for T in [fc.IDENTITY] + list(e.transforms_of(case_name)):
        inputs = e.build(case, T)
        for run in e.runs_of(case_name):
            for what, margin in e.margins(inputs, run):
                assert margin >= fc.MARGIN, (entry, case_name, T.name, run, what, margin)
                lowest = min(lowest, margin)
    print(f'{entry} {case_name}: the closest decision is {lowest:.3e} A from its threshold')


def test_the_cap():
    """No case is dropped for a transform (``parameters`` is the full product); at most one case in three per entry point is
    compared by its frame-free content only, and the table names the header's sentences."""
    listed = fc.parameters()
    for e in fc.ENTRIES:
        names = e.case_names()
        assert 2 <= len(names) <= 3
        for c in names:
            want = {(e.name, c, T.name, run) for T in e.transforms_of(c) for run in e.runs_of(c)}
            assert want <= set(listed) and len(e.transforms_of(c)) == len(e.transforms)
        by_rule = fc.FRAME_DEPENDENT_BY_RULE.get(e.name, {}).get('cases', ())
        assert set(by_rule) <= set(names) and 3 * len(by_rule) <= len(names) and len(by_rule) < len(names)
        kinds = {T.kind for T in e.transforms}
        assert {'perm', 'mirror', 'shift', 'renumber'} <= kinds and (e.name == 'dl_shape_scores') == ('rot' not in kinds)
        assert sum(T.kind == 'perm' for T in e.transforms) == sum(T.kind == 'mirror' for T in e.transforms) == 24
    header = open(fc.__file__.replace('tests/frame_cases.py', 'include/difflinker_hip.h')).read()
    flat = ' '.join(re.sub(r'\n \* ?', ' ', header).split())
    assert set(fc.FRAME_DEPENDENT_BY_RULE) == {'dl_add_hydrogens'}
    for entry, row in fc.FRAME_DEPENDENT_BY_RULE.items():
        for sentence in row['header'] + tuple(s for site in row.get('sites', {}).values() for s in site['header']):
            assert ' '.join(sentence.split()) in flat, (entry, sentence)
    relax = fc.ENTRY_POINTS['dl_relax_molecules']
    assert all(relax.runs_of(c) == (0, 1, 40) for c in relax.case_names())
    assert len(fc.ENTRIES) == 13
    for e in fc.ENTRIES:
        for c in e.case_names():
            case = e.build(e.case(c), fc.IDENTITY)
            masks = [case[k] for k in ('mask', 'qm', 'mask_a', 'ligand_mask') if k in case]
            if masks:
                assert len(masks[0]) <= fc.MAX_B and masks[0].sum(1).max() <= fc.MAX_ATOMS, (e.name, c)


def test_hydrogen_cases_cover_every_kind_of_site():
    e = fc.ENTRY_POINTS['dl_add_hydrogens']
    seen = {}
    for c in e.case_names():
        inputs = e.build(e.case(c), fc.IDENTITY)
        seen[c] = {kind for b in range(len(inputs['mask'])) for kind in e.site_kinds(inputs, b).values()}
    assert 'arbitrary' not in seen['random'] | seen['hand'] and 'arbitrary' in seen['axes']
    assert {'full', 'handed', 'numbered'} <= seen['random'] | seen['hand'], seen
    assert set(fc.FRAME_DEPENDENT_BY_RULE['dl_add_hydrogens']['sites']) == {'handed', 'numbered'}
    for c in ('random', 'hand'):                      # a third or more of a case's parents are compared in full under EVERY transform
        inputs = e.build(e.case(c), fc.IDENTITY)
        kinds = [kind for b in range(len(inputs['mask'])) for kind in e.site_kinds(inputs, b).values()]
        print(c, {k: kinds.count(k) for k in set(kinds)})
        assert 3 * kinds.count('full') >= len(kinds), (c, kinds)


# ---- 2. the rules as written -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,case_name,transform,run', fc.parameters() + fc.parameters(fc.CHAINS))
def test_restatement_is_frame_and_numbering_free(entry, case_name, transform, run):
    fc.check(restatement, entry, case_name, transform, run, BASE)


def test_restatement_deviations_are_those_written_down():
    """``relax_ref.relax`` on every case and transform: the constants of ``frame_cases`` are the largest deviations, rounded up."""
    e = fc.ENTRY_POINTS['dl_relax_molecules']
    for run in e.runs:
        top = {}
        for c in e.case_names():
            if run not in e.runs_of(c):
                continue
            case = e.case(c)
            in0 = e.build(case, fc.IDENTITY)
            out0 = e.reference(in0, run)
            for T in e.transforms_of(c):
                in1 = e.build(case, T)
                for name, value in e.deviations(T, in0, out0, in1, e.reference(in1, run)).items():
                    if value > top.get(name, (-1.0,))[0]:
                        top[name] = (value, c, T.name)
        print(f'steps {run}: {top}')
        for name, (value, _, _) in top.items():
            written = fc.RELAX_DEVIATION[run][name]
            assert 0.8 * written <= value <= written, (run, name, value, written)


def test_relax_f_is_a_length():
    """The regression case of what this suite found in the rule of ``dl_relax_molecules``: ``f`` was the largest force
    COMPONENT, which a rotation changes by up to sqrt(3), and with it ``f_max`` and the step at which a run meets ``f_tol``.
    It is the largest |F| of an atom now, in the header, the restatement and the kernel together.  One movable atom pulled
    by one bond with |F| = 20, along the diagonal and along x: the two agree at every ``f_tol``, where an ``f_tol`` between
    |F| / sqrt(3) and |F| used to end the diagonal one alone."""
    import relax_ref as rr
    far = 1.54 + 0.1
    diagonal = fc.molecule_of([0, 0], [(0, 0, 0), (far / np.sqrt(3),) * 3], [(1, 0, 1)], marked=[1])
    along_x = fc.molecule_of([0, 0], [(0, 0, 0), (far, 0, 0)], [(1, 0, 1)], marked=[1])
    batch = fc.pack([fc.moved(m, fc.IDENTITY, b) for b, m in enumerate((diagonal, along_x))], 4, 1)
    force = 2 * rr.DEFAULTS['k_bond'] * 0.1
    for f_tol, steps in ((0.5 * force, [1, 1]), (0.8 * force, [1, 1]), (1.2 * force, [0, 0])):
        got = rr.reference(batch, steps=1, f_tol=f_tol)
        assert got['steps_done'].tolist() == steps and np.allclose(got['f_max'], force, rtol=1e-4), (f_tol, got['steps_done'], got['f_max'])


# ---- 3. teeth ----------------------------------------------------------------------------------------------------------------------
def test_an_axis_error_fails_the_rotation(monkeypatch):
    """A plane fit that ignores z calls the chair of cyclohexane flat in the frame it was built in and nowhere else."""
    original = ar.ring_plane
    monkeypatch.setattr(ar, 'ring_plane', lambda points: original([(p[0], p[1], 0.0) for p in points]))
    fc.check(restatement, 'dl_aromatic_rings', 'hand', 'shift_0', None, {})
    with pytest.raises(AssertionError):
        fc.check(restatement, 'dl_aromatic_rings', 'hand', 'rot_11', None, {})


def test_a_handedness_error_fails_the_mirror(monkeypatch):
    """The hydrogen of a three-neighbour atom pushed along ``u1 x u2``: a pseudovector added to a vector.  Every proper motion
    still passes; a mirror does not."""
    original = hr.directions

    def skewed(a, pos, adj, cls, d, decisions=None):
        found = original(a, pos, adj, cls, d, decisions)
        if d == 3 and len(found) == 1:
            u1, u2 = (hr.unit(hr.sub(pos[t], pos[a])) for t in adj[a][:2])
            found = [hr.unit(hr.add(found[0], hr.scale(0.2, hr.cross(u1, u2))))]
        return found

    monkeypatch.setattr(hr, 'directions', skewed)
    fc.check(restatement, 'dl_add_hydrogens', 'hand', 'rot_11', None, {})
    fc.check(restatement, 'dl_add_hydrogens', 'hand', 'perm_yzx+++', None, {})
    with pytest.raises(AssertionError):
        fc.check(restatement, 'dl_add_hydrogens', 'hand', 'mirror_xyz++-', None, {})


def test_an_index_order_error_fails_the_renumbering(monkeypatch):
    """The first query row of a molecule measured with half its distances: a row index that leaks into the result.  (The
    one-hot rows of these cases have one largest entry, so ``first_maximum`` taking the last maximum would change nothing.)"""
    original = clash_ref.dist2

    def leaking(q, t):
        d2 = original(q, t)
        d2[:1] *= np.float32(0.25)
        return d2

    monkeypatch.setattr(clash_ref, 'dist2', leaking)
    fc.check(restatement, 'dl_clash_scores', 'own_targets', 'perm_yzx+++', None, {})
    with pytest.raises(AssertionError):
        fc.check(restatement, 'dl_clash_scores', 'own_targets', 'renumber_5', None, {})


def test_swapped_cross_components_fail_the_rotation(monkeypatch):
    """The issue's own example of a shared formula error: a cross product with two components swapped."""
    monkeypatch.setattr(hr, 'cross', lambda a, b: (a[1] * b[2] - a[2] * b[1], a[0] * b[1] - a[1] * b[0], a[2] * b[0] - a[0] * b[2]))
    with pytest.raises(AssertionError):
        fc.check(restatement, 'dl_add_hydrogens', 'random', 'rot_12', None, {})


# ---- 4. the transforms -------------------------------------------------------------------------------------------------------------
def test_signed_permutations_are_exact_in_fp32():
    rng = np.random.default_rng(0)
    x = (300.0 * rng.normal(size=(200, 3))).astype(np.float32)
    assert len(fc.PERMS) == len(fc.MIRRORS) == 24 and len({T.name for T in fc.ALL}) == len(fc.ALL)
    seen = set()
    for T in fc.PERMS + fc.MIRRORS:
        assert round(np.linalg.det(T.R)) == (1 if T.kind == 'perm' else -1) and T.exact
        assert np.array_equal(np.abs(T.R).sum(0), np.ones(3)) and np.array_equal(np.abs(T.R).sum(1), np.ones(3))
        y = T.apply(x)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y), 'no rounding'
        assert np.array_equal(np.sort(np.abs(y), 1), np.sort(np.abs(x.astype(np.float64)), 1)), 'the same numbers'
        assert np.array_equal(T.undo(y), x.astype(np.float64))
        seen.add(T.R.tobytes())
    assert len(seen) == 48


def test_rotations_are_proper_and_orthogonal_and_translations_are_as_long_as_they_say():
    for T in fc.ROTATIONS:
        assert np.abs(T.R.T @ T.R - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(T.R) - 1.0) <= 1e-15 and not T.exact
        assert np.abs(np.abs(T.R) - np.eye(3)).max() > 0.1, 'no axis stays where it was'
    lengths = [float(np.linalg.norm(T.t)) for T in fc.SHIFTS]
    assert lengths[0] == 0.0 and abs(lengths[1] - 100.0) < 0.5 and abs(lengths[2] - 300.0) < 0.5
    assert fc.SHIFTS[0].exact and not fc.SHIFTS[1].exact
    for T in fc.LATTICE_SHIFTS:
        assert np.array_equal(T.t * 2, np.round(T.t * 2)), 'a multiple of the lattice spacing'


def test_undo_of_a_renumbering_is_the_identity_on_a_labelled_array():
    T = fc.RENUMBERINGS[0]
    m = fc.molecule_of([0, 1, 2, 0, 2], [(k, 2.0 * k, -k) for k in range(5)], [(1, 0, 1), (4, 2, 2), (3, 1, 1)], planar=[4], marked=[0, 3],
                       dropped=[2], aromatic=[1])
    new = fc.moved(m, T, 0)
    sigma = new['sigma']
    assert sorted(sigma.tolist()) == list(range(5)) and sigma.tolist() != list(range(5))
    labels = np.arange(5) * 10
    moved_labels = np.empty(5, int)
    moved_labels[sigma] = labels                                         # the label travels with its atom
    assert np.array_equal(fc.by_atom(moved_labels, sigma), labels)
    assert fc.renamed_back(new['entries'], sigma) == sorted(m['entries']) and [e[2] for e in new['entries']] == [e[2] for e in m['entries']]
    assert np.array_equal(fc.by_atom(new['points'], sigma), m['points']) and fc.by_atom(new['types'], sigma).tolist() == m['types']
    for key in ('planar', 'marked', 'dropped'):
        assert sorted(int(np.argsort(sigma)[k]) for k in new[key]) == m[key]
    assert new['aromatic'] == m['aromatic'], 'bond_aromatic goes with the entries, which keep their order'
    packed0, packed1 = fc.pack([fc.moved(m, fc.IDENTITY, 0)], 9, 1), fc.pack([new], 9, 1 + T.seed)
    assert packed0['rows'][0].tolist() != packed1['rows'][0].tolist(), 'a new scatter among the padding rows'
    other = T.sigma(5, 0, salt=1)
    assert other.tolist() != sigma.tolist(), 'protein and target atoms are permuted independently'
