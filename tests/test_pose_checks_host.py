"""Host side of the internal-geometry checks (``dl_pose_checks``): the plain-Python rule of ``tests/pose_checks_ref.py`` on
molecules whose answer is known by hand, on ties placed on coordinates that are exact in fp32, and on the committed case-study
ligands; the export and its declaration; the three ``const`` tables; ``compute_pose_checks`` on hand-made records; the
command lines.  No GPU: the kernel is compared with the same reference in ``tests/test_gpu_pose_checks.py``."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import aromatic_ref as ar
import pose_checks_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = pr.default_tables()
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h
BAD = (pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES)


def run(m, tables=TABLES, detail=None, **more):
    """``(counts, flags, status)`` of a molecule dict by the reference, its planar / marked / dropped atoms applied."""
    n = len(m['types'])
    rows = lambda atoms: np.isin(np.arange(n), atoms).astype(np.float32)      # noqa: E731
    return pr.molecule(np.asarray(m['points'], dtype=np.float32).reshape(n, 3), m['types'], np.ones(n), m['entries'],
                       more.pop('n_bonds_in', len(m['entries'])), *tables, drop=rows(m['dropped']), mark=rows(m['marked']),
                       planar=rows(m['planar']), detail=detail, **more)


@pytest.mark.parametrize('name', sorted(pr.HAND))
def test_counts_of_every_hand_made_molecule(name):
    counts, flags, status = run(pr.hand_molecule(name))
    assert counts[0] == pr.HAND[name][4] and counts[1] == [0] * 8 and status == 0, 'nothing is marked'
    if name in pr.CLEAN:
        assert not any(flags) and not any(counts[0][k] for k in BAD)


def test_ideal_molecules_are_clean():
    assert {'butane', 'benzene', 'propyne', 'sulfone'} <= set(pr.CLEAN)
    detail = {}
    run(pr.hand_molecule('sulfone'), detail=detail)
    assert [b[4] for b in detail['bonds']] == ['ok', 'ok', 'untabled', 'untabled'], 'the bond table has no S=O length'
    assert {a[3] for a in detail['angles']} == {pr.TETRAHEDRAL}, 'four neighbours: tetrahedral, not the hydrogens\' class rule'
    run(pr.hand_molecule('benzene'), detail=detail)
    assert {a[3] for a in detail['angles']} == {pr.TRIGONAL} and not detail['pairs'], 'para atoms are three bonds apart'
    run(pr.hand_molecule('propyne'), detail=detail)
    assert [(a[3], a[4]) for a in detail['angles']] == [(pr.LINEAR, -1.0)]


@pytest.mark.parametrize('name', sorted(pr.ties()))
def test_ties_at_the_bound_and_one_ulp_inside(name):
    m, tables, want = pr.ties()[name]
    assert np.array_equal(np.asarray(m['points'], np.float32).astype(np.float64), np.asarray(m['points'])), 'exact in fp32'
    counts, flags, status = run(m, tables)
    assert counts[0] == want and status == 0
    assert bool(any(flags)) == bool(any(want[k] for k in BAD))


def test_ring_angles_are_exempt_and_open_chains_are_not():
    for name in ('cyclopropane', 'cyclobutane'):
        assert run(pr.hand_molecule(name))[0][0][pr.ANGLES] == 0
    opened = pr.hand_molecule('cyclobutane')
    opened['entries'] = opened['entries'][:3]                      # the same four atoms as a chain: two right angles, checked
    assert run(opened)[0][0][pr.ANGLES] == 2
    assert run(pr.hand_molecule('folded_short_chain'))[0][0][pr.ANGLES:pr.ANGLES + 2] == [2, 0], '90 degrees is within 25 of 109.5'


def test_a_bent_nitrile_and_a_sharp_carbon_are_flagged():
    for name in ('bent_nitrile', 'sharp_carbon'):
        counts, flags, _ = run(pr.hand_molecule(name))
        assert counts[0][pr.BAD_ANGLES] == 1 and flags == [0, pr.FLAG_ANGLE, 0], 'the centre carries the flag'


def test_far_pairs_start_four_bonds_apart():
    detail = {}
    counts, flags, _ = run(pr.hand_molecule('folded_chain'), detail=detail)
    assert [(a, b, clash) for a, b, _, clash in detail['pairs']] == [(0, 4, True)] and abs(math.sqrt(detail['pairs'][0][2]) - 1.54) < 1e-6
    assert flags == [pr.FLAG_CLASH, 0, 0, 0, pr.FLAG_CLASH]
    counts, flags, _ = run(pr.hand_molecule('folded_short_chain'), detail=detail)
    assert not detail['pairs'] and not any(flags), 'the same distance three bonds apart is no pair at all'
    ends = np.asarray(pr.hand_molecule('folded_short_chain')['points'])
    assert abs(np.linalg.norm(ends[0] - ends[3]) - 1.54) < 1e-6
    assert run(pr.hand_molecule('two_pieces_overlapping'))[0][0][pr.PAIRS:] == [4, 4]
    assert run(pr.hand_molecule('two_pieces_apart'))[0][0][pr.PAIRS:] == [4, 0]


def test_centres_with_four_and_five_neighbours():
    detail = {}
    assert run(pr.hand_molecule('four_bonded_C'), detail=detail)[0][0][pr.ANGLES:pr.ANGLES + 2] == [6, 2]
    assert sorted(round(math.degrees(math.acos(a[4]))) for a in detail['angles']) == [90] * 4 + [180] * 2
    assert run(pr.hand_molecule('five_bonded_C'))[0][0][pr.ANGLES] == 0, 'more than four neighbours: not checked'


def test_marked_counts_follow_the_mark_mask():
    m = pr.hand_molecule('folded_chain')
    for marked, want in (([0], [1, 0, 0, 0, 1, 0, 1, 1]), ([2], [2, 0, 0, 0, 3, 0, 0, 0]), ([0, 1, 2, 3, 4], pr.HAND['folded_chain'][4])):
        counts, _, _ = run(dict(m, marked=marked))
        assert counts[0] == pr.HAND['folded_chain'][4] and counts[1] == want, marked
    m = pr.hand_molecule('stretched_bond')
    assert run(dict(m, marked=[1]))[0][1] == [1, 0, 0, 1, 0, 0, 0, 0]


def test_drops_bad_entries_and_limits():
    m = pr.hand_molecule('folded_chain')
    counts, flags, status = run(dict(m, dropped=[2]))               # two pieces of two atoms: four far pairs, a side of the
    assert counts[0] == [2, 0, 0, 0, 0, 0, 4, 4] and flags == [4, 4, 0, 4, 4] and status == 0      # pentagon and three diagonals (2.49 A)
    bad = [(0, 0, 1), (0, 1, 0), (0, 1, 4), (1, 0, 3), (0, 5, 1), (-1, 2, 1)]
    counts, _, status = run(dict(m, entries=m['entries'] + bad))
    assert status == pr.BAD_BOND and counts[0] == pr.HAND['folded_chain'][4], 'a repeated pair counts once, with its first order'
    counts, _, status = run(dict(m, entries=[(1, 0, 3)] + m['entries']))
    assert status == pr.BAD_BOND and counts[0][:4] == [4, 0, 0, 1], 'as a triple bond 1.54 A is long'
    assert run(m, n_bonds_in=9, status_in=2)[2] == 2 | pr.BONDS_OVERFLOW
    assert run(m, n_bonds_in=-3)[0][0] == [0, 0, 0, 0, 0, 0, 10, 10], 'no bonds: every pair is far, and closer than 2.55 A'
    points = [list(p) for p in m['points']]
    points[4][1] = float('nan')
    counts, flags, status = run(dict(m, points=points))
    assert status == pr.NONFINITE and counts == [[0] * 8] * 2 and not any(flags)
    assert run(dict(m, points=points, dropped=[4]))[2] == 0, 'a dropped atom\'s coordinates are not looked at'
    big = pr.chain(257)
    counts, flags, status = run(dict(big, entries=big['entries'] + [(5, 5, 1)]))
    assert status == pr.TOO_LARGE and counts == [[0] * 8] * 2 and not any(flags), 'the list is not looked at'
    counts, _, status = run(pr.chain(256))
    assert status == 0 and counts[0][pr.CHECKED] == 255 and counts[0][pr.PAIRS] == 256 * 255 // 2 - 255 - 254 - 253


def test_invariance_under_list_order_and_orientation():
    rng = np.random.default_rng(5)
    for m in [pr.random_molecule(rng) for _ in range(20)]:
        base = run(m)
        order = rng.permutation(len(m['entries']))
        turned = [(m['entries'][k][1], m['entries'][k][0], m['entries'][k][2]) for k in order]
        assert run(dict(m, entries=turned)) == base


# ---- the committed ligands ---------------------------------------------------------------------------------------------------
def ligand(path):
    """A case-study ligand as the drivers see it: bonds from the distance table, orders refined by ``aromatic_ref``, checked at
    the defaults with ``atom_aromatic`` as the planar flags."""
    from difflinker_amd import const
    from difflinker_amd.io import read_sdf_molecules
    mol = read_sdf_molecules(os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies', path))[0][0]
    types = [const.ATOM2IDX[s] for s in mol.symbols]
    x = np.asarray(mol.positions, dtype=np.float32)
    n = len(types)
    entries = pr.perceive(types, x)
    got = ar.molecule(x, types, [1.0] * n, entries, len(entries), ar.ring_class_table(const.ATOM2IDX))
    refined = [(i, j, order) for (i, j, _), order in zip(entries, got['order_out'])]
    detail = {}
    counts, flags, status = pr.molecule(x, types, np.ones(n), refined, len(refined), *TABLES, status_in=got['status'],
                                        planar=got['atom_aromatic'], detail=detail)
    return mol, types, counts, flags, status, detail


def measures(types, detail):
    from difflinker_amd import const
    ratios = [math.sqrt(d2) / (const.BOND_LENGTHS[order - 1][types[a]][types[j]] / 100.0) for a, j, order, d2, _ in detail['bonds']]
    contact = min(math.sqrt(d2) / (const.VDW_RADII[types[a]] + const.VDW_RADII[types[b]]) for a, b, d2, _ in detail['pairs'])
    off = max(abs(math.degrees(math.acos(c)) - pr.IDEALS[cls]) for _, _, _, cls, c, _ in detail['angles'])
    return min(ratios), max(ratios), contact, off


@pytest.mark.parametrize('path', ['hsp90/3hz1_ligand_obabel.sdf', 'impdh/5ou2_fragments_input.sdf'])
def test_crystal_ligands_pass_with_room(path):
    mol, types, counts, flags, status, detail = ligand(path)
    assert status == 0 and not any(flags) and not any(counts[0][k] for k in BAD) and counts[0][pr.UNTABLED] == 0
    assert counts[0][pr.CHECKED] == len(detail['bonds']) > 20 and counts[0][pr.ANGLES] > 30 and counts[0][pr.PAIRS] > 150
    low, high, contact, off = measures(types, detail)
    print(f'{path}: length ratios {low:.3f} to {high:.3f}, closest far contact {contact:.3f} of the radii sum, worst angle '
          f'{off:.1f} degrees from its ideal')
    assert 0.875 < low and high < 1.102 and contact > 0.88 and off < 19.6, 'five degrees and more of room under the defaults'


def test_3fi3_is_flagged_for_its_long_bond_and_its_wide_nitrogen():
    """The file bonds N19 to C26 at 1.70 A, which the distance table does not take as a bond (N-C: below 1.57 A).  The two atoms
    are then far from each other and clash at 0.52 of their radii sum, and so do C17 (bonded to N19) and C26 at 2.545 A against
    2.55 A.  The bridging N20 has its two carbons 138 degrees apart, 28.6 from the tetrahedral ideal.  Nothing else fires."""
    mol, types, counts, flags, status, detail = ligand('jnk/3fi3_ligand.sdf')
    assert status == 0 and counts[0] == [41, 0, 0, 0, 56, 1, 548, 2]
    assert (19, 26, 1) in [(min(i, j), max(i, j), o) for i, j, o in mol.bonds] and mol.symbols[19] == 'N' and mol.symbols[26] == 'C'
    assert not any({a, j} == {19, 26} for a, j, *_ in detail['bonds']), 'no bond for the distance table'
    clashes = {(a, b): math.sqrt(d2) for a, b, d2, clash in detail['pairs'] if clash}
    assert sorted(clashes) == [(17, 26), (19, 26)] and abs(clashes[(19, 26)] - 1.700) < 1e-3 and 2.54 < clashes[(17, 26)] < 2.55
    assert any({a, j} == {17, 19} for a, j, *_ in detail['bonds'])
    bad = [(j, a, k, cls, math.degrees(math.acos(c))) for j, a, k, cls, c, is_bad in detail['angles'] if is_bad]
    assert [(j, a, k, cls) for j, a, k, cls, _ in bad] == [(25, 20, 30, pr.TETRAHEDRAL)] and mol.symbols[20] == 'N'
    assert abs(bad[0][4] - 138.1) < 0.1
    assert [k for k, f in enumerate(flags) if f] == [17, 19, 20, 26] and flags[20] == pr.FLAG_ANGLE and flags[26] == pr.FLAG_CLASH
    low, high, contact, off = measures(types, detail)
    assert 0.875 < low and high < 1.11 and abs(contact - 0.523) < 1e-3 and abs(off - 28.6) < 0.05


# ---- declarations, tables, scores --------------------------------------------------------------------------------------------
def test_export_declaration_and_constants():
    import __graft_entry__ as g
    from difflinker_amd import _lib
    at = _lib.EXPORTS.index('dl_perceive_bonds')
    assert _lib.EXPORTS[at + 1:at + 3] == ('dl_pose_checks', 'dl_interaction_types') and _lib.ABI_VERSION == 7
    assert _lib.EXPORTS[-1] == 'dl_best_rmsd'
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_pose_checks(const dl_pose_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert ' *   dl_pose_checks ' in header[:header.index('#ifndef DIFFLINKER_HIP_H')], 'listed in the opening comment'
    section = header[header.index('pose_checks.hip'):]
    for words in ('NOT PoseBusters', 'no hydrogens', 'no energy', 'contraction off', 'three-ring', 'four-ring',
                  'NaN that no comparison flags', 'tests/pose_checks_ref.py', 'plain stores only'):
        assert words in section, words
    for name, value in (('MAX_ATOMS', 256), ('TOO_LARGE', 4), ('BAD_BOND', 8), ('NONFINITE', 64), ('COUNTS', 8)):
        assert re.search(rf'#define DL_POSE_{name} {value}\b', header) and getattr(_lib, f'DL_POSE_{name}') == value
    assert (pr.MAX_ATOMS, pr.TOO_LARGE, pr.BAD_BOND, pr.NONFINITE, pr.BONDS_OVERFLOW) == (
        _lib.DL_POSE_MAX_ATOMS, _lib.DL_POSE_TOO_LARGE, _lib.DL_POSE_BAD_BOND, _lib.DL_POSE_NONFINITE, _lib.DL_BONDS_OVERFLOW)
    assert (_lib.DL_POSE_TOO_LARGE, _lib.DL_POSE_BAD_BOND, _lib.DL_POSE_NONFINITE) == (
        _lib.DL_HYDRO_TOO_LARGE, _lib.DL_HYDRO_BAD_BOND, _lib.DL_HYDRO_NONFINITE)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'pose_checks.hip') in g.HIP_SOURCES
    fields = [f[0] for f in _lib.DLPoseArgs._fields_]
    struct = header[header.index('typedef struct dl_pose_args {'):header.index('} dl_pose_args;')]
    declared = re.findall(r'(\w+)\s*(?:,|;)', re.sub(r'/\*.*?\*/', '', struct))
    assert declared == fields, 'the ctypes structure lists the header\'s members in order'
    assert fields[-1] == 'stream', 'the entry point takes the structure alone, the stream as its last field'
    assert ctypes.sizeof(_lib.DLPoseArgs) == 152        # LP64: 16 + 9 * 8 + 8 + 3 * 8 + 3 * 8 + 8 (an int32 before a pointer is padded)
    g.build()
    assert hasattr(_lib.load(), 'dl_pose_checks') and _lib.load().dl_abi_version() == 7


def test_argument_checks_come_before_device_work():
    from difflinker_amd import _lib
    lib = _lib.load()
    call = lambda a: int(lib.dl_pose_checks(ctypes.byref(a)))      # noqa: E731
    ok = dict(B=2, N=40, nf=8, capacity=8)
    assert int(lib.dl_pose_checks(None)) == BAD_ARG
    assert call(_lib.DLPoseArgs(**ok)) == BAD_ARG                   # null pointers
    assert call(_lib.DLPoseArgs(**dict(ok, capacity=0))) == BAD_ARG  # also when the list may be null
    for wrong in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(capacity=-1)):
        assert call(_lib.DLPoseArgs(**{**ok, 'B': 0, **wrong})) == BAD_ARG, wrong
    assert call(_lib.DLPoseArgs(**dict(ok, B=0))) == _lib.DL_OK, 'an empty batch is looked at no further than its sizes'
    assert call(_lib.DLPoseArgs(**dict(ok, B=0, N=1024, capacity=0))) == _lib.DL_OK


def test_the_three_tables_against_hand_values():
    from difflinker_amd import const
    C, O, N, S, Cl, I, P = (const.GEOM_ATOM2IDX[s] for s in ('C', 'O', 'N', 'S', 'Cl', 'I', 'P'))
    for is_geom, n in ((False, 8), (True, 9)):
        bounds = const.length_bounds_table(is_geom)
        assert bounds.dtype == torch.float64 and bounds.shape == (n, n, 3, 2) and torch.equal(bounds, bounds.transpose(0, 1))
        assert bounds[C, C, 0].tolist() == [(0.75 * 1.54) * (0.75 * 1.54), (1.25 * 1.54) * (1.25 * 1.54)]
        assert bounds[C, N, 2].tolist() == [(0.75 * 1.16) * (0.75 * 1.16), (1.25 * 1.16) * (1.25 * 1.16)]
        assert bounds[O, C, 1].tolist() == [(0.75 * 1.2) * (0.75 * 1.2), (1.25 * 1.2) * (1.25 * 1.2)]
        assert bounds[S, O, 1].tolist() == [0.0, 0.0] and bounds[Cl, I].tolist() == [[0.0, 0.0]] * 3, 'no typical length'
        assert bounds.tolist() == pr.length_bounds2(n)
        clash = const.internal_clash_table(is_geom)
        assert clash.dtype == torch.float64 and clash.shape == (n, n) and clash.tolist() == pr.clash2(n)
        assert clash[C, C].item() == (0.75 * 3.4) * (0.75 * 3.4) and abs(clash[N, O].item() - (0.75 * 3.07) ** 2) < 1e-12
    assert const.length_bounds_table(True)[P, O, 1].tolist() == [(0.75 * 1.5) * (0.75 * 1.5), (1.25 * 1.5) * (1.25 * 1.5)]
    wide = const.length_bounds_table(False, 0.5, 2.0)
    assert wide[C, C, 0].tolist() == [0.77 * 0.77, 3.08 * 3.08]
    assert const.internal_clash_table(False, 1.0)[C, C].item() == 3.4 * 3.4
    cosines = const.angle_cos_table()
    assert cosines.dtype == torch.float64 and cosines.shape == (3, 2) and cosines.tolist() == pr.angle_cos()
    deg = lambda v: math.degrees(math.acos(v))                      # noqa: E731
    assert cosines[0, 0].item() == -2.0 and abs(deg(cosines[0, 1].item()) - 155.0) < 1e-9
    assert abs(deg(cosines[1, 0].item()) - 145.0) < 1e-9 and abs(deg(cosines[1, 1].item()) - 95.0) < 1e-9
    assert abs(deg(cosines[2, 0].item()) - 134.4712206) < 1e-6 and abs(deg(cosines[2, 1].item()) - 84.4712206) < 1e-6
    assert const.angle_cos_table(80.0)[:, 0].tolist() == [-2.0, -2.0, -2.0]
    assert const.angle_cos_table(125.0)[1:, 1].tolist() == [2.0, 2.0] and const.angle_cos_table(125.0)[0, 1].item() < 1.0
    assert const.ATOM2IDX == pr.ATOM2IDX and pr.IDEALS == const.ANGLE_IDEALS


def record(short=0, long_=0, angles=0, clashes=0, linker=(0, 0, 0, 0), status=0):
    from difflinker_amd.metrics import PoseRecord
    row = lambda s, lg, a, c: (9, 1, s, lg, 12, a, 30, c)           # noqa: E731
    return PoseRecord(row(short, long_, angles, clashes), row(*linker), 0, status)


def test_compute_pose_checks():
    from difflinker_amd.metrics import POSE_COUNTS, POSE_NAMES, compute_pose_checks
    assert POSE_COUNTS == ('bonds_checked', 'bonds_untabled', 'bonds_short', 'bonds_long', 'angles_checked', 'angles_bad',
                           'pairs_checked', 'clashes')
    pred = [record(), record(short=1, long_=1), record(angles=3, clashes=1, linker=(0, 0, 1, 0)), record(status=8)]
    got = compute_pose_checks(pred)
    assert list(got) == list(POSE_NAMES)
    assert got == {'bond_lengths_valid': 0.5, 'bond_angles_valid': 0.5, 'internal_clash_free': 0.5, 'pose_valid': 0.25,
                   'bond_lengths_valid_linker': 0.75, 'bond_angles_valid_linker': 0.5, 'internal_clash_free_linker': 0.75,
                   'pose_valid_linker': 0.5, 'bad_bonds_per_molecule': 2 / 3, 'bad_angles_per_molecule': 1.0,
                   'internal_clashes_per_molecule': 1 / 3}
    true = [record()] * 3 + [record(clashes=2, linker=(0, 0, 0, 2))]
    both = compute_pose_checks(pred, true)
    assert list(both) == list(POSE_NAMES) + ['true_' + name for name in POSE_NAMES]
    assert {k: both[k] for k in POSE_NAMES} == got
    assert both['true_pose_valid'] == both['true_internal_clash_free_linker'] == 0.75 and both['true_bond_angles_valid'] == 1.0
    assert both['true_internal_clashes_per_molecule'] == 0.5 and both['true_bad_bonds_per_molecule'] == 0.0
    assert set(compute_pose_checks([]).values()) == {None}
    assert compute_pose_checks([record(status=64)])['bad_bonds_per_molecule'] is None
    with pytest.raises(ValueError, match='2 predictions, 1 true'):
        compute_pose_checks(pred[:2], true[:1])


def test_python_callers_refuse_the_cpu():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import analyze_pose_checks, pose_checks
    from difflinker_amd.molecule_builder import Bonds
    found = Bonds(*(torch.zeros(s, dtype=torch.int32) for s in ((1,), (1, 4, 3), (1, 6), (1,), (1, 6), (1,))))
    one_hot, x, mask = torch.zeros(1, 6, 8), torch.zeros(1, 6, 3), torch.ones(1, 6, 1)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        pose_checks(one_hot, x, mask, found, False)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_pose_checks(one_hot, x, mask, False, mask)


def test_command_lines_keep_their_defaults(monkeypatch):
    """Without the new switch ``generate``, ``sample`` and the model are called exactly as before; with it the keyword appears."""
    import inspect
    from difflinker_amd import DDPM, generate as gen, sample as smp
    for function in (gen.generate, gen.generate_with_pocket, gen.generate_with_protein, gen._sample_and_save, smp.sample):
        assert inspect.signature(function).parameters['pose_checks'].default is False
    seen = {}
    for name in ('generate', 'generate_with_pocket', 'generate_with_protein'):
        monkeypatch.setattr(gen, name, lambda *a, **k: seen.update(k) or [])
    for more in ([], ['--pocket', 'p.pdb'], ['--protein', 'p.pdb']):
        seen.clear()
        gen.main(['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3'] + more)
        assert 'pose_checks' not in seen
        gen.main(['--fragments', 'f.sdf', '--model', 'm', '--linker_size', '3', '--pose_checks'] + more)
        assert seen['pose_checks'] is True
    seen.clear()
    monkeypatch.setattr(smp, 'sample', lambda *a, **k: seen.update(k) or 'out')
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p'])
    assert 'pose_checks' not in seen
    smp.main(['--checkpoint', 'c', '--samples', 's', '--prefix', 'p', '--pose_checks'])
    assert seen['pose_checks'] is True
    from test_gpu_generate import ddpm_hparams
    assert DDPM(**ddpm_hparams(False)).pose_metrics is False
    from difflinker_amd import train
    assert '--pose_checks' in inspect.getsource(train.main) and 'model.pose_metrics = bool(a.pose_checks)' in inspect.getsource(train.main)
