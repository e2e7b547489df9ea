"""The interaction score without a GPU: the constants, the two C entries (exported where the header says, struct layouts,
argument checks, ABI unchanged), every refusal of the Python layer, ``compute_interactions`` on hand-written records, and the
numpy restatement ``interaction_ref`` on residues, ligands and pairs worked by hand."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import interaction_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, O, N, CL = R.C, R.O, R.N, R.CL
H, D, A = R.HYDROPHOBIC, R.DONOR, R.ACCEPTOR
ONE = 2 ** 32


def test_constants():
    from difflinker_amd import const
    assert const.XS_RADII == (1.9, 1.7, 1.8, 1.5, 2.0, 1.8, 2.0, 2.2, 2.1), 'C O N F S Cl Br I P'
    assert const.INTERACTION_WEIGHTS == (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439), 'the published weights, no rotor term'
    geom, zinc = const.xs_radius_table(True), const.xs_radius_table(False)
    assert geom.dtype == torch.float64 and geom.tolist() == list(const.XS_RADII) and zinc.tolist() == list(const.XS_RADII[:8])
    assert [const.GEOM_IDX2ATOM[k] for k in range(9)] == ['C', 'O', 'N', 'F', 'S', 'Cl', 'Br', 'I', 'P']
    assert (R.C, R.O, R.N, R.F_, R.S, R.CL, R.BR, R.I, R.P) == tuple(const.GEOM_ATOM2IDX[s] for s in
                                                                  ('C', 'O', 'N', 'F', 'S', 'Cl', 'Br', 'I', 'P'))


def declared_fields(header, name):
    body = header.split('typedef struct %s {' % name)[1].split('} %s;' % name)[0]
    return [part.strip(' *') for line in body.splitlines() if ';' in line
            for part in line.split(';')[0].split(None, 1 + line.strip().startswith('const'))[-1].split(',')]


def test_exports_declared_checked_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    assert 'int32_t dl_interaction_types(const dl_interact_types_args* args);' in header
    assert 'int32_t dl_interaction_scores(const dl_interact_args* args);' in header
    assert hasattr(lib, 'dl_interaction_types') and hasattr(lib, 'dl_interaction_scores')
    assert {'dl_interaction_types', 'dl_interaction_scores'} <= set(_lib.EXPORTS) and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    assert ' *   dl_interaction_types / dl_interaction_scores' in header.split('#ifndef DIFFLINKER_HIP_H')[0]
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7 and '#define DL_ABI_VERSION 7' in header
    for name, value in (('DL_XS_HYDROPHOBIC', 16), ('DL_XS_DONOR', 32), ('DL_XS_ACCEPTOR', 64), ('DL_INTERACT_TERMS', 5),
                        ('DL_INTERACT_NONFINITE', 1), ('DL_INTERACT_TOO_LARGE', 2), ('DL_INTERACT_BAD_TYPE', 4),
                        ('DL_INTERACT_UNTYPED', 8)):
        assert f'#define {name} {value} ' in header and getattr(_lib, name) == value
    assert (R.HYDROPHOBIC, R.DONOR, R.ACCEPTOR) == (16, 32, 64)
    assert (R.NONFINITE, R.TOO_LARGE, R.BAD_TYPE, R.UNTYPED) == (1, 2, 4, 8)
    assert _lib.DLInteractTypesArgs._fields_[-1][0] == 'stream' == _lib.DLInteractArgs._fields_[-1][0], 'the stream is the last field'
    assert declared_fields(header, 'dl_interact_types_args') == [name for name, _ in _lib.DLInteractTypesArgs._fields_]
    assert declared_fields(header, 'dl_interact_args') == [name for name, _ in _lib.DLInteractArgs._fields_]
    for words in ('NOT AutoDock Vina', 'no hydrogens, no PDBQT typing, no search or pose', 'no intramolecular term and no rotor normalisation',
                  'pyridine or nitrile N', 'histidine', 'pocket boundary', 'stays below 2^63'):
        assert words in ' '.join(header.split()).replace(' * ', ' '), words
    # no GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1) before any device work
    one = ctypes.c_void_p(16)                    # never dereferenced
    assert lib.dl_interaction_types(None) == -1 and lib.dl_interaction_scores(None) == -1
    required = ('x', 'one_hot', 'group', 'table', 'xs_type', 'status')
    ok = dict(B=2, N=8, nf=9, **{k: one for k in required})
    for bad in [dict(B=-1), dict(N=0), dict(nf=0), dict(nf=17)] + [{k: None} for k in required]:
        assert lib.dl_interaction_types(ctypes.byref(_lib.DLInteractTypesArgs(**dict(ok, **bad)))) == -1, bad
    assert lib.dl_interaction_types(ctypes.byref(_lib.DLInteractTypesArgs(B=0, N=8, nf=9))) == _lib.DL_OK
    assert lib.dl_interaction_types(ctypes.byref(_lib.DLInteractTypesArgs(B=0, N=0, nf=9))) == -1
    required = ('x', 'xs_type', 'query_mask', 'radius', 'n_query', 'n_target', 'n_pairs', 'n_hbonds', 'n_hydrophobic', 'terms',
                'status', 'atom_terms')
    ok = dict(B=2, N=8, nf=9, M=3, target_mask=one, target_x=one, target_xs=one, **{k: one for k in required})
    refusals = [dict(B=-1), dict(N=0), dict(nf=0), dict(nf=17), dict(M=-1), dict(target_x=None), dict(target_xs=None)]
    for bad in refusals + [{k: None} for k in required]:
        assert lib.dl_interaction_scores(ctypes.byref(_lib.DLInteractArgs(**dict(ok, **bad)))) == -1, bad
    assert lib.dl_interaction_scores(ctypes.byref(_lib.DLInteractArgs(B=0, N=8, nf=9))) == _lib.DL_OK
    for field, value in (('N', 0), ('nf', 17), ('M', -1)):
        worse = _lib.DLInteractArgs(B=0, N=8, nf=9)
        setattr(worse, field, value)
        assert lib.dl_interaction_scores(ctypes.byref(worse)) == -1, 'the sizes are checked before the empty batch'


def test_the_python_layer_refuses_before_any_launch():
    from difflinker_amd import _lib, metrics
    one_hot, x, mask = torch.zeros(1, 4, 9), torch.zeros(1, 4, 3), torch.ones(1, 4)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.analyze_interactions(one_hot, x, mask, mask)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.interaction_types(one_hot, x, mask.int())
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        metrics.protein_types(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32))

    class OnDevice(torch.Tensor):                # a CPU tensor that says it is on the device: the shape checks come next
        is_cuda = True

    dev = lambda t: t.as_subclass(OnDevice)      # noqa: E731
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.analyze_interactions(dev(one_hot), dev(torch.zeros(1, 5, 3)), dev(mask), dev(mask))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.analyze_interactions(dev(one_hot), dev(x), dev(torch.ones(1, 3)), dev(mask))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.analyze_interactions(dev(one_hot), dev(x), dev(mask), dev(torch.ones(2, 4)))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.analyze_interactions(dev(one_hot), dev(x), dev(mask), dev(mask), target_mask=dev(torch.ones(1, 5)))
    with pytest.raises(ValueError, match=r'\(positions, types, xs_types\)'):
        metrics.analyze_interactions(dev(one_hot), dev(x), dev(mask), dev(mask), protein=(dev(torch.zeros(2, 3)), dev(torch.zeros(2))))
    with pytest.raises(ValueError, match='atom types'):
        metrics.analyze_interactions(dev(torch.zeros(1, 4, 7)), dev(x), dev(mask), dev(mask))
    with pytest.raises(ValueError, match='not \\[B,N,nf\\]'):
        metrics.analyze_interactions(dev(torch.zeros(4, 9)), dev(x), dev(mask), dev(mask))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.interaction_types(dev(one_hot), dev(x), dev(torch.ones(1, 5).int()))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.interaction_types(dev(one_hot), dev(torch.zeros(1, 4, 2)), dev(mask.int()))
    with pytest.raises(ValueError, match='shapes disagree'):
        metrics.protein_types(dev(torch.zeros(3, 3)), dev(torch.zeros(4, dtype=torch.int32)))


def record(n_query=4, n_pairs=50, n_hbonds=0, n_hydrophobic=0, terms=(0, 0, 0, 0, 0), status=0):
    from difflinker_amd.metrics import InteractionRecord, interaction_score
    return InteractionRecord(n_query, 30, n_pairs, n_hbonds, n_hydrophobic, list(terms), interaction_score(terms), status,
                             [0.0] * n_query)


def test_compute_interactions_on_hand_written_records():
    from difflinker_amd import const
    from difflinker_amd.metrics import INTERACTION_NAMES, INTERACTION_TRUE_NAMES, compute_interactions, interaction_score
    w = const.INTERACTION_WEIGHTS
    assert interaction_score([ONE, 0, 0, 0, 0]) == w[0] and interaction_score([0, 0, 2 * ONE, 0, ONE // 2]) == 2 * w[2] + 0.5 * w[4]
    pred = [record(terms=(10 * ONE, 40 * ONE, ONE // 2, 3 * ONE, 2 * ONE), n_hbonds=2, n_hydrophobic=4),
            record(n_query=6, terms=(4 * ONE, 20 * ONE, 0, ONE, 0), n_hydrophobic=1),
            record(n_query=0, n_pairs=0),                                                # nothing to score: counts as a zero
            record(terms=(ONE, ONE, ONE, ONE, ONE), n_hbonds=9, status=1),               # flagged: out of everything
            record(terms=(ONE, ONE, ONE, ONE, ONE), n_hbonds=9, status=2),
            record(terms=(ONE, ONE, ONE, ONE, ONE), n_hbonds=9, status=8)]
    got = compute_interactions(pred)
    assert tuple(got) == INTERACTION_NAMES
    s0 = 10 * w[0] + 40 * w[1] + 0.5 * w[2] + 3 * w[3] + 2 * w[4]
    s1 = 4 * w[0] + 20 * w[1] + 0.0 * w[2] + 1 * w[3] + 0.0 * w[4]
    assert got['interaction_molecules'] == 3 and got['interaction_flagged'] == 3
    assert got['interaction_score'] == pytest.approx((s0 + s1) / 3, rel=1e-14)
    assert got['interaction_gauss1'] == 14 / 3 and got['interaction_gauss2'] == 20.0 and got['interaction_repulsion'] == 0.5 / 3
    assert got['interaction_hydrophobic'] == 4 / 3 and got['interaction_hbond'] == 2 / 3
    assert got['hbonds_per_molecule'] == 2 / 3 and got['hydrophobic_contacts_per_molecule'] == 5 / 3
    assert got['interaction_score_per_atom'] == pytest.approx((s0 + s1) / 10, rel=1e-14)
    skipped_only = compute_interactions([record(status=4, n_hbonds=1)])
    assert skipped_only['interaction_molecules'] == 1 and skipped_only['interaction_flagged'] == 0, 'a skipped atom does not void the rest'
    true = [record(terms=(8 * ONE, 0, 0, 0, ONE), n_hbonds=1), record(status=1), record(n_hbonds=3), record(), record(), record()]
    with_true = compute_interactions(pred, true)
    assert tuple(with_true) == INTERACTION_NAMES + INTERACTION_TRUE_NAMES and {k: with_true[k] for k in INTERACTION_NAMES} == got
    t0 = 8 * w[0] + w[4]
    assert with_true['true_interaction_score'] == pytest.approx(t0 / 2, rel=1e-14), 'positions 0 and 2: both scored'
    assert with_true['true_hbonds_per_molecule'] == 2.0
    assert with_true['interaction_excess'] == pytest.approx((s0 - t0) / 2, rel=1e-14)
    nothing = compute_interactions([])
    assert nothing == dict({k: 0.0 for k in INTERACTION_NAMES}, interaction_molecules=0, interaction_flagged=0)
    assert compute_interactions([], [])['interaction_excess'] == 0.0
    with pytest.raises(ValueError):
        compute_interactions(pred, true[:2])


# ---- the reference's typing on residues and ligands built by hand -----------------------------------------------------------
# a backbone in a plane: C(prev) - N - CA - C(=O), zigzag steps of (1.25, +-0.7, 0): bonds of 1.43 A, 1-3 distances of 2.5 A
BACKBONE = [('Cp', C, (0.0, 0.0, 0.0)), ('N', N, (1.25, 0.7, 0.0)), ('CA', C, (2.5, 0.0, 0.0)), ('C', C, (3.75, 0.7, 0.0)),
            ('O', O, (3.75, 1.93, 0.0))]
CB = ('CB', C, (2.5, -0.9, 1.2))


def typed(atoms, group=None):
    from difflinker_amd import const
    names = [a[0] for a in atoms]
    assert len(set(names)) == len(names)
    one_hot = np.eye(9, dtype=np.float32)[[a[1] for a in atoms]][None]
    x = np.float32([a[2] for a in atoms])[None]
    group = np.ones((1, len(atoms)), np.int32) if group is None else np.asarray(group)[None]
    xs, status = R.interaction_types(x, one_hot, group, const.bond_threshold_table(True)[..., 0].numpy())
    assert status.tolist() == [0]
    return dict(zip(names, xs[0].tolist()))


def test_reference_typing_of_residues():
    ser = typed(BACKBONE + [CB, ('OG', O, (2.5, -1.9, 2.2))])
    assert ser['N'] == N | D, 'a backbone N with two neighbours is a donor'
    assert ser['OG'] == O | A | D, 'a hydroxyl: its one neighbour at 1.41 A, d2 = 2.0 >= 1.6875'
    assert ser['O'] == O | A, 'the carbonyl O at 1.23 A: acceptor only'
    assert ser['CA'] == C and ser['C'] == C and ser['CB'] == C, 'carbons next to N or O are not hydrophobic'
    assert ser['Cp'] == C, 'bonded to N'
    pro = typed(BACKBONE + [CB, ('CD', C, (1.25, 1.6, 1.15))])
    assert pro['N'] == N, 'three neighbours: no donor'
    assert pro['CB'] == C | H, 'its one neighbour is CA'
    asp = typed(BACKBONE + [CB, ('CG', C, (2.5, -1.9, 2.3)), ('OD1', O, (3.5, -2.65, 2.3)), ('OD2', O, (1.5, -2.65, 2.3))])
    assert asp['OD1'] == O | A and asp['OD2'] == O | A, 'carboxylate oxygens at 1.25 A (d2 = 1.5625): acceptors only'
    assert asp['CG'] == C and asp['CB'] == C | H
    # Phe: CG and a regular hexagon of 1.39 A in the plane spanned by the CB-CG direction and the x axis
    cg = np.array([2.5, -1.9, 2.3])
    u = (cg - np.array(CB[2])) / np.linalg.norm(cg - np.array(CB[2]))
    centre = cg + 1.39 * u
    ring = [centre + 1.39 * (-math.cos(k * math.pi / 3) * u + math.sin(k * math.pi / 3) * np.array([1.0, 0, 0])) for k in range(6)]
    assert np.allclose(ring[0], cg)
    phe = typed(BACKBONE + [CB] + [(f'R{k}', C, tuple(p)) for k, p in enumerate(ring)])
    assert all(phe[f'R{k}'] == C | H for k in range(6)) and phe['CB'] == C | H, 'ring carbons and CB: carbon neighbours only'
    assert phe['CA'] == C, 'CA is bonded to N'
    assert typed([('W', O, (5.0, 5.0, 5.0))]) == {'W': O | A | D}, 'a lone O is a water'


def test_reference_typing_of_ligands_and_groups():
    # Cl-C-C(=O)-N-C-O(H) along the zigzag, the carbonyl O above its carbon
    lig = [('Cl', CL, (-1.5, 0.9, 0.0)), ('C1', C, (0.0, 0.0, 0.0)), ('C2', C, (1.25, 0.7, 0.0)), ('O2', O, (1.25, 1.93, 0.0)),
           ('N3', N, (2.5, 0.0, 0.0)), ('C4', C, (3.75, 0.7, 0.0)), ('O5', O, (5.0, 0.0, 0.0))]
    got = typed(lig)
    assert got == {'Cl': CL | H, 'C1': C, 'C2': C, 'O2': O | A, 'N3': N | D, 'C4': C, 'O5': O | A | D}
    # the same atoms in two groups: the alcohol's carbon is in the other group, so the O is a water and C4 sees only N3
    split = typed(lig, group=[1, 1, 1, 1, 1, 1, 2])
    assert split['O5'] == O | A | D and split['C4'] == C and split['Cl'] == CL | H
    # group 0 is not typed and is nobody's neighbour: C1 and C2 see each other alone
    part = typed(lig, group=[0, 1, 1, 0, 0, 0, 0])
    assert part == {'Cl': -1, 'C1': C | H, 'C2': C | H, 'O2': -1, 'N3': -1, 'C4': -1, 'O5': -1}
    # a nitrile N (one neighbour) is a donor: a known misreading
    assert typed([('C', C, (0, 0, 0)), ('N', N, (1.16, 0, 0))])['N'] == N | D
    # a non-finite typed row flags the molecule; in group 0 it is never read
    from difflinker_amd import const
    table = const.bond_threshold_table(True)[..., 0].numpy()
    x = np.zeros((2, 2, 3), np.float32)
    x[:, 1, 0] = np.nan
    one_hot = np.eye(9, dtype=np.float32)[[[0, 0], [0, 0]]]
    xs, status = R.interaction_types(x, one_hot, [[1, 1], [1, 0]], table)
    assert status.tolist() == [R.NONFINITE, 0] and xs.tolist() == [[-1, -1], [C | H, -1]]


# ---- the reference's terms at distances worked by hand -------------------------------------------------------------------------
def pair(r, qs, ts, radius):
    x = np.float32([[[0, 0, 0], [r, 0, 0]]])
    return R.interaction_scores(x, [[qs, ts]], [[1, 0]], radius, [[0, 1]])


def test_reference_terms_of_a_carbon_pair():
    """Radii of 1.5 A so that r = 3, 3.5, 4, 4.5 (exact in fp32) are s = 0, 0.5, 1, 1.5 exactly."""
    radius = [1.5] * 9
    want = {0.0: (ONE, round(math.exp(-2.25) * ONE), 0, ONE, 0, 1),
            0.5: (round(math.exp(-1.0) * ONE), round(math.exp(-1.5625) * ONE), 0, ONE, 0, 1),       # 1.5 - 0.5 = 1
            1.0: (round(math.exp(-4.0) * ONE), round(math.exp(-1.0) * ONE), 0, ONE // 2, 0, 1),
            1.5: (round(math.exp(-9.0) * ONE), round(math.exp(-0.5625) * ONE), 0, 0, 0, 0)}        # the ramp has reached 0
    for s, (g1, g2, rep, hyd, hb, n_hyd) in want.items():
        got = pair(3.0 + s, C | H, C | H, radius)
        assert got['terms'][0].tolist() == [g1, g2, rep, hyd, hb], s
        assert (got['n_pairs'][0], got['n_hydrophobic'][0], got['n_hbonds'][0], got['status'][0]) == (1, n_hyd, 0, 0), s
        assert got['atom_terms'][0].tolist() == [[g1, g2, rep, hyd, hb], [0] * 5], 'the query row alone'
        assert pair(3.0 + s, C | H, C, radius)['terms'][0].tolist() == [g1, g2, rep, 0, 0], 'one of them not hydrophobic'


def test_reference_terms_of_a_donor_acceptor_pair():
    """r = 2.5; the radius sums 3.2, 2.85 and 2.5 put s at -0.7, -0.35 and 0 to within an fp64 rounding: the ramp gives 1, 0.5
    and 0, and a rounding of s moves the fixed point by less than 2^-20 of a unit."""
    for r_sum, s, hb, n_hb in ((3.2, -0.7, ONE, 1), (2.85, -0.35, ONE // 2, 1), (2.5, 0.0, 0, 0)):
        radius = [1.0, r_sum - 1.0, 1.0] + [1.0] * 6                   # N (query) 1.0, O (target) the rest
        got = pair(2.5, N | D, O | A, radius)
        rep = int(np.rint((2.5 - (1.0 + (r_sum - 1.0))) ** 2 * ONE)) if s < 0 else 0
        assert got['terms'][0][2:].tolist() == [rep, 0, hb] and got['n_hbonds'][0] == n_hb, s
        assert got['terms'][0][0] == int(np.rint(math.exp(-((2 * (2.5 - (1.0 + (r_sum - 1.0)))) ** 2)) * ONE))
        swapped = pair(2.5, O | A, N | D, [1.0, 1.0, r_sum - 1.0] + [1.0] * 6)
        assert swapped['terms'][0][4] == hb, 'an acceptor query facing a donor target'
        assert pair(2.5, N | D, N | D, [1.0, 1.0, r_sum - 1.0] + [1.0] * 6)['terms'][0][4] == 0, 'two donors'
        assert pair(2.5, O | A, O | A, [1.0, r_sum / 2, 1.0] + [1.0] * 6)['terms'][0][4] == 0, 'two acceptors'


def test_reference_cut_flags_and_score():
    from difflinker_amd import const
    radius = list(const.XS_RADII)
    assert pair(8.0, C | H, C | H, radius)['n_pairs'][0] == 0 and not pair(8.0, C | H, C | H, radius)['terms'].any(), '64 < 64 is false'
    near = pair(7.75, C | H, C | H, radius)
    assert near['n_pairs'][0] == 1 and near['terms'][0][1] > 0
    assert pair(1.0, -1, C, radius)['status'][0] == R.UNTYPED and pair(1.0, C, 9, radius)['status'][0] == R.UNTYPED
    assert pair(float('nan'), C, C, radius)['status'][0] == R.NONFINITE
    shared = R.interaction_scores(np.zeros((1, 1, 3), np.float32), [[C]], [[1]], radius, None, [[3, 0, 0], [4, 0, 0]], [C, -1])
    assert (shared['status'][0], shared['n_target'][0], shared['n_pairs'][0]) == (R.BAD_TYPE, 1, 1)
    terms = np.array([[ONE, 2 * ONE, 0, 0, ONE // 2]])
    w = const.INTERACTION_WEIGHTS
    assert R.score(terms, w)[0] == (w[0] * ONE + w[1] * (2 * ONE) + w[2] * 0.0 + w[3] * 0.0 + w[4] * (ONE // 2)) / ONE
    from difflinker_amd.metrics import interaction_score
    assert interaction_score(terms[0].tolist()) == R.score(terms, w)[0]


def test_drivers_parse_the_interactions_flag(monkeypatch, capsys):
    from difflinker_amd import generate, sample, train
    seen = []
    monkeypatch.setattr(sample, 'sample', lambda *a, **kw: seen.append(kw))
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--interactions'])
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p'])
    assert seen == [{'interactions': True}, {}], 'without the flag the call is what it was'
    calls = []
    monkeypatch.setattr(generate, 'generate_with_pocket', lambda *a, **kw: calls.append(kw) or [])
    monkeypatch.setattr(generate, 'generate_with_protein', lambda *a, **kw: calls.append(kw) or [])
    common = ['--fragments', 'f.sdf', '--model', 'm.ckpt', '--linker_size', '5']
    generate.main(common + ['--pocket', 'p.pdb', '--interactions'])
    generate.main(common + ['--protein', 'p.pdb', '--interactions'])
    generate.main(common + ['--pocket', 'p.pdb'])
    assert [kw.get('interactions') for kw in calls] == [True, True, None]
    with pytest.raises(SystemExit):
        train.main(['--help'])
    assert '--interactions' in capsys.readouterr().out


def test_generate_interactions_needs_a_protein(tmp_path):
    """Raised before the model is loaded: the checkpoint named here does not exist."""
    from difflinker_amd import generate
    argv = ['--fragments', 'frag.sdf', '--model', str(tmp_path / 'missing.ckpt'), '--linker_size', '5',
            '--output', str(tmp_path / 'out'), '--interactions']
    with pytest.raises(ValueError, match='--pocket or --protein'):
        generate.main(argv)
    assert not (tmp_path / 'out').exists()
