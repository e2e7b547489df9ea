"""Host tests of the stereo feature: the restatement ``tests/stereo_ref.py`` against molecules with analytically placed atoms
whose labels are stated from first principles, the string writer ``molecule_builder.smiles`` with stereo against the reader
``stereo_ref.read_stereo`` (a round trip over hand-built and seeded random molecules), the stereo-aware codes through
``canon_ref`` on the widened types, the declarations, and ``metrics.compute_stereo``.  No GPU anywhere in this file."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import canon_cases
import canon_ref
import stereo_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
ROUND_TRIP_SEEDS = (200, 206, 212, 222, 226, 241, 249, 254)          # eight molecules each; what they hold is asserted below


def labels(m, **kwargs):
    r = sr.perceive_one(m, **kwargs)
    n = len(m['types'])
    atoms = {k: s for k, s in enumerate(r["atom_stereo"][:n]) if s > 0}
    bonds = {(min(i, j), max(i, j)): s for (i, j, _), s in zip(m['entries'], r['bond_stereo']) if s}
    return atoms, bonds, r


# ---- the rule on molecules whose answer is known -------------------------------------------------------------------------------
def test_tet_has_the_hand_the_expectations_assume():
    t = np.array(sr.TET, dtype=float)
    assert np.linalg.det(t[1:] - t[0]) == pytest.approx(-16) and np.linalg.det(t[1:]) == pytest.approx(-4) and sr.TET_SIGN == -1
    assert sr.V_IDEAL4 == pytest.approx(16 / 3 ** 1.5) and sr.V_IDEAL3 == pytest.approx(4 / 3 ** 1.5)
    assert abs(np.linalg.det((t[1:] - t[0]) / math.sqrt(3))) == pytest.approx(sr.V_IDEAL4)


@pytest.mark.parametrize('name', sorted(sr.CENTRES))
def test_centres_from_first_principles(name):
    m = sr.HAND[name]
    atoms, bonds, r = labels(m)
    want = {c: sr.expected_centre(r['atom_class'], on, 1 if name == 'ammonium' else None) for c, on in sr.CENTRES[name].items()}
    assert atoms == want and not bonds and r['counts'] == [[len(want), 0, 0, 0], [0, 0, 0, 0]] and r['status'] == 0


def test_the_two_hands_of_chfclbr_get_the_two_labels():
    a, b = labels(sr.HAND['chfclbr_a'])[0], labels(sr.HAND['chfclbr_b'])[0]
    assert sorted([a[0], b[0]]) == [1, 2]
    mirrored = dict(sr.HAND['chfclbr_a'], points=[(-x, y, z) for x, y, z in sr.HAND['chfclbr_a']['points']])
    assert labels(mirrored)[0] == b


@pytest.mark.parametrize('name', sorted(sr.DOUBLE_BONDS))
def test_double_bonds_from_first_principles(name):
    atoms, bonds, r = labels(sr.HAND[name])
    assert bonds == sr.DOUBLE_BONDS[name] and not atoms and r['counts'][0] == [0, 0, len(bonds), 0]


@pytest.mark.parametrize('name', sr.NOTHING)
def test_what_the_rule_does_not_perceive(name):
    atoms, bonds, r = labels(sr.HAND[name])
    assert not atoms and not bonds and r['counts'] == [[0] * 4] * 2, name


def test_benzene_needs_its_flags_and_a_ring_of_eight_is_the_first_with_a_label():
    unflagged = dict(sr.HAND['benzene'], aromatic=[], planar=[])
    assert not labels(unflagged)[1], 'a ring of six: none either way'
    big = dict(sr.ring(8, (0, 2, 4, 6)), aromatic=[0, 2])
    assert sorted(labels(big)[1]) == [(4, 5), (6, 7)], 'the flagged first entries are left out, the others are cis in the ring'
    assert [len(labels(sr.ring(n))[1]) for n in (5, 6, 7, 8, 9)] == [0, 0, 0, 1, 1]


def test_tartaric_skeletons_meso_has_opposite_labels():
    for name, same in (('tartaric_meso_12', False), ('tartaric_meso_21', False), ('tartaric_chiral_a', True), ('tartaric_chiral_b', True)):
        atoms = labels(sr.HAND[name])[0]
        assert sorted(atoms) == [1, 2] and (atoms[1] == atoms[2]) == same, name
    assert labels(sr.HAND['tartaric_chiral_a'])[0][1] != labels(sr.HAND['tartaric_chiral_b'])[0][1]


def test_a_flattened_centre_is_undetermined_exactly_below_the_bar():
    seen = set()
    for height in (1.0, 0.5, 0.3, 0.2, 0.15, 0.1, 0.05, 0.0, -0.05, -0.15, -0.3, -1.0):
        # F, Cl, Br at 120 degrees around the z axis, lifted by `height`: V = det of the three unit vectors
        arms = [(math.cos(a), math.sin(a), height) for a in (0.0, 2 * math.pi / 3, 4 * math.pi / 3)]
        m = sr.mol([sr.C, sr.F, sr.CL, sr.BR], [(0, 0, 0)] + arms, [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
        atoms, _, r = labels(m)
        units = np.array(arms) / np.linalg.norm(arms[0])
        order = sorted((1, 2, 3), key=lambda k: r['atom_class'][k])
        V = float(np.linalg.det(units[[k - 1 for k in order]]))
        assert abs(abs(V) - sr.FLAT * sr.V_IDEAL3) > 1e-6
        want = 3 if abs(V) <= sr.FLAT * sr.V_IDEAL3 else 1 if V > 0 else 2
        assert atoms == {0: want}, height
        assert r['counts'][0][:2] == ([0, 1] if want == 3 else [1, 0])
        seen.add(want)
    assert seen == {1, 2, 3}
    touching = sr.mol([sr.C, sr.F, sr.CL, sr.BR], [(0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 1), (0, 2, 1), (0, 3, 1)])
    assert labels(touching)[0] == {0: 3}, 'a neighbour at zero distance'
    assert labels(sr.HAND['chfclbr_a'], flat=3.9)[0] == {0: 3} and labels(sr.HAND['chfclbr_a'], flat=0.0)[0][0] in (1, 2)


def test_a_twisted_double_bond_is_undetermined_between_60_and_120_degrees():
    for degrees, want in ((0, 1), (59, 1), (61, 3), (90, 3), (119, 3), (121, 2), (180, 2)):
        assert labels(sr.olefin([sr.F], [sr.F], cis=True, twist_degrees=degrees))[1] == {(0, 1): want}, degrees
    linear = sr.mol([sr.C, sr.C, sr.F, sr.F], [(0, 0, 0), (1.3, 0, 0), (-1.3, 0.05, 0), (2.0, 1.0, 0)], [(0, 1, 2), (0, 2, 1), (1, 3, 1)])
    assert labels(linear)[1] == {(0, 1): 3}, 'an arm of less than 0.1 A off the axis'


def test_two_substituents_the_reference_is_the_higher_class():
    m = sr.olefin([sr.F, sr.C], [sr.CL, sr.C], cis=True)             # F and Cl up on the same side
    _, bonds, r = labels(m)
    cls = r['atom_class']
    left, right = max((2, 3), key=lambda k: cls[k]), max((4, 5), key=lambda k: cls[k])
    assert bonds == {(0, 1): 1 if (left == 2) == (right == 4) else 2}


def test_drops_marks_bad_entries_and_limits():
    m = sr.HAND['l_alanine']
    assert labels(dict(m, dropped=[2]))[0] == {}, 'without its methyl the centre has two neighbours'
    assert labels(dict(m, planar=[1]))[0] == {}
    assert labels(dict(m, marked=[5]))[2]['counts'] == [[1, 0, 0, 0], [0, 0, 0, 0]]
    assert labels(dict(m, marked=[2]))[2]['counts'] == [[1, 0, 0, 0], [1, 0, 0, 0]]
    z = sr.HAND['z_butene']
    assert labels(dict(z, marked=[3]))[2]['counts'][1] == [0, 0, 1, 0]
    r = labels(dict(z, entries=z['entries'] + [(1, 0, 1), (0, 0, 1)]))[2]
    assert r['status'] == sr.BAD_BOND and r['bond_stereo'] == [1, 0, 0, 0, 0], 'the first entry gives the pair its order'
    r = labels(dict(z, entries=[(1, 0, 1)] + z['entries']))[2]
    assert r['status'] == sr.BAD_BOND and not any(r['bond_stereo'])
    points = [list(p) for p in z['points']]
    points[3][2] = float('inf')
    r = labels(dict(z, points=points))[2]
    assert r['status'] == sr.NONFINITE and not any(r['bond_stereo']) and r['atom_class'] == [0, 0, 2, 2]
    assert labels(dict(z, points=points, dropped=[3]))[2]['status'] == 0


def test_invariance_under_list_order_orientation_and_renumbering():
    rng = np.random.default_rng(3)
    for m in sr.random_molecules(77, 24):
        base = labels(m)
        order = [int(v) for v in rng.permutation(len(m['entries']))]
        turned = dict(m, entries=[(m['entries'][e][1], m['entries'][e][0], m['entries'][e][2]) for e in order],
                      aromatic=[order.index(e) for e in m['aromatic']])
        assert labels(turned)[:2] == base[:2] and labels(turned)[2]['counts'] == base[2]['counts']
        other, sigma = sr.renumbered(m, rng)
        atoms, bonds, r = labels(other)
        assert atoms == {sigma[k]: s for k, s in base[0].items()} and r['counts'] == base[2]['counts']
        assert bonds == {(min(sigma[a], sigma[b]), max(sigma[a], sigma[b])): s for (a, b), s in base[1].items()}


# ---- codes ------------------------------------------------------------------------------------------------------------------------
def codes(m):
    r = sr.perceive_one(m)
    n = len(m['types'])
    return tuple(canon_ref.canonical_ranks(sr.wide_types(m['types'], m['entries'], r['atom_stereo'][:n], r['bond_stereo'], mirror),
                                           m['entries'])['code'] for mirror in (False, True))


def test_codes_of_the_tartaric_skeletons_and_the_hexadienes():
    a, b, meso, other = (codes(sr.HAND[f'tartaric_{k}']) for k in ('chiral_a', 'chiral_b', 'meso_12', 'meso_21'))
    assert len({a[0], b[0], meso[0]}) == 3, 'three stereoisomers'
    assert a[0] == b[1] and a[1] == b[0] and a[0] != a[1], 'the enantiomers are each other\'s mirror codes'
    assert meso[0] == meso[1], 'meso is its own mirror image: not chiral'
    assert meso == other, 'built as (1, 2) and as (2, 1): one code'
    rng = np.random.default_rng(4)
    assert codes(sr.renumbered(sr.HAND['tartaric_chiral_a'], rng)[0]) == a
    dienes = [codes(sr.HAND[f'hexadiene_{k}']) for k in ('ee', 'ez', 'zz')]
    assert len({c[0] for c in dienes}) == 3 and all(c[0] == c[1] for c in dienes)
    alanine = sr.HAND['l_alanine']
    plain = canon_ref.canonical_ranks(alanine['types'], alanine['entries'])['code']
    assert plain not in codes(alanine), 'the widened types are another vocabulary: stereo codes compare with stereo codes only'


def test_stereo_types_on_the_host_are_the_restatements():
    from difflinker_amd import metrics
    from difflinker_amd.molecule_builder import Bonds
    names = ['tartaric_chiral_a', 'hexadiene_ez', 'l_alanine']
    batch = sr.as_batch([sr.HAND[name] for name in names], 12, scatter=False)
    want = sr.perceive(batch['x'], batch['one_hot'], batch['node_mask'], batch['bonds'], batch['n_bonds_in'])
    found = Bonds(torch.as_tensor(batch['n_bonds_in']), torch.as_tensor(batch['bonds']), None, None, None, None)
    for mirror in (False, True):
        wide = metrics.stereo_types(torch.as_tensor(batch['one_hot']), torch.as_tensor(batch['node_mask']), found,
                                    torch.as_tensor(want['atom_stereo']), torch.as_tensor(want['bond_stereo']), mirror)
        assert wide.shape == (3, 12, 128) and wide.dtype == torch.float32
        for b, name in enumerate(names):
            m = sr.HAND[name]
            n = len(m['types'])
            assert wide[b, :n].argmax(dim=1).tolist() == sr.wide_types(m['types'], m['entries'], want['atom_stereo'][b][:n],
                                                                       want['bond_stereo'][b], mirror), (name, mirror)
    with pytest.raises(ValueError):
        metrics.stereo_types(torch.zeros(1, 4, 17), torch.ones(1, 4), found, torch.zeros(1, 4), torch.zeros(1, 1))


# ---- strings ------------------------------------------------------------------------------------------------------------------------
def isomeric(m):
    """``(string, labels the string states, labels perceived)`` of a molecule without dropped atoms."""
    from difflinker_amd.molecule_builder import smiles
    atoms, bonds, r = labels(m)
    n = len(m['types'])
    ranked = canon_ref.canonical_ranks(sr.wide_types(m['types'], m['entries'], r['atom_stereo'][:n], r['bond_stereo']), m['entries'])
    assert ranked['status'] == 0
    text = smiles(m['types'], m['entries'], ranked['rank'], r['atom_class'][:n], r['atom_stereo'][:n], r['bond_stereo'])
    read = sr.read_stereo(text)
    bare = lambda t: re.sub(r'@+H?\]', ']', t).translate({ord(c): None for c in '/\\[]'})     # noqa: E731
    assert bare(text) == bare(smiles(m['types'], m['entries'], ranked['rank'])), 'the plain string but for the stereo marks'
    order = sr.written_order(n, m['entries'], ranked['rank'])
    assert [m['types'][k] for k in order] == read['types']
    assert sorted((min(order[i], order[j]), max(order[i], order[j]), o) for i, j, o in read['bonds']) == \
        sorted((min(i, j), max(i, j), o) for i, j, o in m['entries'])
    stated = sr.stated_labels(read, order, r['atom_class'], n, {(min(i, j), max(i, j)): o for i, j, o in m['entries']})
    perceived = ([atoms.get(k, 0) if atoms.get(k) in (1, 2) else 0 for k in range(n)], {p: s for p, s in bonds.items() if s in (1, 2)})
    return text, stated, perceived


@pytest.mark.parametrize('name', sorted(sr.HAND))
def test_round_trip_of_the_hand_built_molecules(name):
    text, stated, perceived = isomeric(sr.HAND[name])
    assert stated == perceived, text
    again, sigma = sr.renumbered(sr.HAND[name], np.random.default_rng(len(name)))
    assert isomeric(again)[0] == text, 'the same string under a renumbering'


def test_the_strings_of_the_named_molecules():
    text = {name: isomeric(sr.HAND[name])[0] for name in sr.HAND}
    assert text['e_butene'] == 'C/C=C/C' and text['z_butene'] == 'C/C=C\\C'
    assert text['e_difluoroethene'] == 'F/C=C/F' and text['z_difluoroethene'] == 'F/C=C\\F'
    assert text['oxime_z'] == 'C/C=N\\O' and text['oxime_e'] == 'C(=N\\O)/C'
    assert text['cyclohexene'] == 'C1=CCCCC1' and text['cyclooctene'] == 'C/1=C/CCCCCC\\1' and text['benzene'] == 'C1=CC=CC=C1'
    assert len({text['hexadiene_ee'], text['hexadiene_ez'], text['hexadiene_zz']}) == 3
    assert text['tartaric_meso_12'] == text['tartaric_meso_21'] and '@' in text['tartaric_meso_12']
    assert len({text['tartaric_meso_12'], text['tartaric_chiral_a'], text['tartaric_chiral_b']}) == 3
    assert {text['chfclbr_a'], text['chfclbr_b']} == {'F[C@H](Br)Cl', 'F[C@@H](Br)Cl'}
    for name in sr.NOTHING:
        assert not set(text[name]) & set('@/\\'), name


def alanine_hand(text):
    """The sign of the determinant in the order (N, H, methyl, acid) that a string of alanine states."""
    read = sr.read_stereo(text)
    (centre, (around, sign)), = read['centres'].items()
    near = {k: [j if i == k else i for i, j, _ in read['bonds'] if k in (i, j)] for k in range(len(read['types']))}
    role = {}
    for t in around:
        role[t] = 'H' if t == -1 else 'N' if read['types'][t] == sr.N else 'acid' if len(near[t]) == 3 else 'methyl'
    return sign * sr.parity([('N', 'H', 'methyl', 'acid').index(role[t]) for t in around])


def test_l_alanine_is_written_as_the_configuration_of_its_usual_string():
    # L-alanine is (S): with the H away from the viewer, N -> COOH -> CH3 runs anticlockwise, so det[N, COOH, CH3] > 0 about
    # the centre.  HAND places N, CH3, COOH on TET[1], TET[2], TET[3]: det[TET1, TET3, TET2] = +4.  Its usual string is
    # N[C@@H](C)C(O)=O; this project's canonical spelling starts at the hydroxyl O and states the same configuration
    t = np.array(sr.TET, dtype=float)
    assert np.linalg.det(t[[1, 3, 2]]) == pytest.approx(4)
    text = isomeric(sr.HAND['l_alanine'])[0]
    assert text == 'OC([C@H](C)N)=O'
    assert alanine_hand(text) == alanine_hand('N[C@@H](C)C(O)=O') == 1
    assert alanine_hand('N[C@H](C)C(O)=O') == -1
    mirrored = dict(sr.HAND['l_alanine'], points=[(x, y, -z) for x, y, z in sr.HAND['l_alanine']['points']])
    assert isomeric(mirrored)[0] == 'OC([C@@H](C)N)=O'


def test_the_reader_on_strings_written_by_hand():
    read = sr.read_stereo('F/C=C/F')
    assert read['double_bonds'] == [(1, 2, 0, 3, False)] and sr.read_stereo('F/C=C\\F')['double_bonds'][0][4]
    assert sr.read_stereo('F\\C=C\\F')['double_bonds'][0][4] is False and sr.read_stereo('C(\\F)=C/F')['double_bonds'][0][4] is False
    assert sr.read_stereo('C/1=C/CCCCCC\\1')['double_bonds'] == [(0, 1, 7, 2, True)]
    assert sr.read_stereo('C/1=C/CCCCCC1')['double_bonds'] == [(0, 1, 7, 2, True)], 'the opening digit alone'
    assert sr.read_stereo('C1=C/CCCCCC\\1')['double_bonds'] == [(0, 1, 7, 2, True)], 'the closing digit alone'
    assert sr.read_stereo('[C@H]1(F)CC1')['centres'] == {0: ([-1, 3, 1, 2], -1)}, 'H, the ring digit, then the children'
    assert sr.read_stereo('Cl[C@@](F)(Br)I')['centres'] == {1: ([0, 2, 3, 4], 1)}
    for broken in ('C/1=C/CCCCCC/1', 'F/C(\\Cl)=C/F', '[C@H](F)Cl', 'C1CC', 'C/=C', '[Xe]'):
        with pytest.raises(ValueError):
            sr.read_stereo(broken)
    types, bonds, bracketed, _ = canon_cases.parse_smiles('FC(Br)Cl'.replace('Cl', 'F').replace('Br', 'S'))
    assert len(types) == 4 and len(bonds) == 3, 'the graph reader of the canon tests reads the stripped strings'


def test_round_trip_of_seeded_random_molecules():
    centres = double_bonds = ring_symbols = centre_digits = 0
    rng = np.random.default_rng(9)
    for seed in ROUND_TRIP_SEEDS:
        for m in sr.random_molecules(seed, 8, margin=2e-3):
            m = dict(m, dropped=[])                  # a string is of the kept molecule; the perception runs on all of it here
            text, stated, perceived = isomeric(m)
            assert stated == perceived, (seed, text)
            assert isomeric(sr.renumbered(m, rng)[0])[0] == text, (seed, text)
            centres += sum(1 for s in perceived[0] if s)
            double_bonds += len(perceived[1])
            ring_symbols += len(re.findall(r'[/\\]%?\d', text))
            centre_digits += len(re.findall(r'@H?\][/\\]?%?\d', text))
    assert centres >= 10 and double_bonds >= 3 and ring_symbols >= 1 and centre_digits >= 1, (centres, double_bonds, ring_symbols,
                                                                                           centre_digits)


def test_without_labels_the_string_is_the_plain_one():
    from difflinker_amd.molecule_builder import smiles
    for name, (types, bonds, *_) in canon_cases.NAMED.items():
        rank = canon_ref.canonical_ranks(types, bonds)['rank']
        plain = smiles(types, bonds, rank)
        assert smiles(types, bonds, rank, None, None, None) == plain
        assert smiles(types, bonds, rank, rank, [0] * len(types), [0] * len(bonds)) == plain, name
        assert smiles(types, bonds, rank, rank, [3] * len(types), [3] * len(bonds)) == plain, 'label 3 writes nothing'


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_export_declaration_and_constants():
    import __graft_entry__ as g
    from difflinker_amd import _lib, const
    assert 'dl_stereo_perceive' in _lib.EXPORTS and _lib.EXPORTS[-1] == 'dl_best_rmsd' and _lib.ABI_VERSION == 7
    assert _lib.STEREO_ENTRY_POINTS == {'dl_stereo_perceive': _lib.DLStereoArgs}
    assert _lib.entry_struct('dl_stereo_perceive') is _lib.DLStereoArgs and 'dl_stereo_perceive' not in _lib.STRUCT_ENTRY_POINTS
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_stereo_perceive(const dl_stereo_args* args);' in header and '#define DL_ABI_VERSION 7' in header
    assert ' *   dl_stereo_perceive ' in header[:header.index('#ifndef DIFFLINKER_HIP_H')], 'listed in the opening comment'
    section = header[header.index('stereo.hip'):]
    for words in ("THE RULE BELOW IS THIS PROJECT'S OWN", "NOT RDKit's stereo perception and NOT CIP", '1-WL', 'contraction off',
                  'tests/stereo_ref.py', 'plain stores only', 'no R/S', 'trivalent N', 'allenes', 'amide'):
        assert words in ' '.join(section.split()).replace('* ', ''), words
    for name, value in (('MAX_ATOMS', 256), ('MAX_BONDS', 2048), ('TOO_LARGE', 4), ('BAD_BOND', 8), ('NONFINITE', 64), ('COUNTS', 4)):
        assert re.search(rf'#define DL_STEREO_{name} {value}\b', header) and getattr(_lib, f'DL_STEREO_{name}') == value
    assert (sr.MAX_ATOMS, sr.MAX_BONDS, sr.TOO_LARGE, sr.BAD_BOND, sr.NONFINITE, sr.BONDS_OVERFLOW) == (
        _lib.DL_STEREO_MAX_ATOMS, _lib.DL_STEREO_MAX_BONDS, _lib.DL_STEREO_TOO_LARGE, _lib.DL_STEREO_BAD_BOND,
        _lib.DL_STEREO_NONFINITE, _lib.DL_BONDS_OVERFLOW)
    assert (_lib.DL_STEREO_TOO_LARGE, _lib.DL_STEREO_BAD_BOND, _lib.DL_STEREO_NONFINITE) == (
        _lib.DL_POSE_TOO_LARGE, _lib.DL_POSE_BAD_BOND, _lib.DL_POSE_NONFINITE)
    assert (_lib.DL_STEREO_TOO_LARGE, _lib.DL_STEREO_BAD_BOND) == (_lib.DL_CANON_TOO_LARGE, _lib.DL_CANON_BAD_BOND)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'stereo.hip') in g.HIP_SOURCES
    fields = [f[0] for f in _lib.DLStereoArgs._fields_]
    struct = header[header.index('typedef struct dl_stereo_args {'):header.index('} dl_stereo_args;')]
    declared = re.findall(r'(\w+)\s*(?:,|;)', re.sub(r'/\*.*?\*/', '', struct))
    assert declared == fields, 'the ctypes structure lists the header\'s members in order'
    assert fields[-1] == 'stream', 'the entry point takes the structure alone, the stream as its last field'
    assert ctypes.sizeof(_lib.DLStereoArgs) == 192       # LP64: 16 + 7 * 8 + 8 + 4 * 8 + 4 * 8 + 6 * 8 (an int32 before a pointer is padded)
    assert const.STEREO_DEFAULTS == {'flat': 0.25, 'twist': 0.5} == {'flat': sr.FLAT, 'twist': sr.TWIST}
    assert const.STEREO_V_IDEAL == (sr.V_IDEAL4, sr.V_IDEAL3)
    assert const.default_valence_table(True).tolist() == list(sr.DEFAULT_VALENCE)
    g.build()
    assert hasattr(_lib.load(), 'dl_stereo_perceive') and _lib.load().dl_abi_version() == 7


def test_argument_checks_come_before_device_work():
    from difflinker_amd import _lib
    lib = _lib.load()
    call = lambda a: int(lib.dl_stereo_perceive(ctypes.byref(a)))    # noqa: E731
    ok = dict(B=2, N=40, nf=8, capacity=8, flat=0.25, twist=0.5, v_ideal4=sr.V_IDEAL4, v_ideal3=sr.V_IDEAL3)
    assert int(lib.dl_stereo_perceive(None)) == BAD_ARG
    assert call(_lib.DLStereoArgs(**ok)) == BAD_ARG                 # null pointers
    assert call(_lib.DLStereoArgs(**dict(ok, capacity=0))) == BAD_ARG
    for wrong in (dict(B=-1), dict(N=0), dict(N=1025), dict(nf=0), dict(nf=257), dict(capacity=-1), dict(flat=-1.0),
                  dict(twist=float('nan')), dict(v_ideal4=0.0), dict(v_ideal3=float('nan'))):
        assert call(_lib.DLStereoArgs(**{**ok, 'B': 0, **wrong})) == BAD_ARG, wrong
    assert call(_lib.DLStereoArgs(**dict(ok, B=0))) == _lib.DL_OK, 'an empty batch is looked at no further than its sizes'


def test_the_python_layer_has_no_cpu_fallback():
    from difflinker_amd import _lib, metrics
    from difflinker_amd.molecule_builder import Bonds
    batch = sr.as_batch([sr.HAND['z_butene']], 8, scatter=False)
    found = Bonds(torch.as_tensor(batch['n_bonds_in']), torch.as_tensor(batch['bonds']), None, None, None, None)
    one_hot, x, mask = (torch.as_tensor(batch[k]) for k in ('one_hot', 'x', 'node_mask'))
    with pytest.raises(_lib.HipLibraryError):
        metrics.stereo(one_hot, x, mask, found, True)
    result = {'atom_stereo': torch.zeros(1, 8), 'bond_stereo': torch.zeros(1, 3), 'counts': torch.zeros(1, 2, 4)}
    with pytest.raises(_lib.HipLibraryError):
        metrics.stereo_codes(result, one_hot, mask, found)


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def record(centres=0, linker=0, bonds=0, bonds_linker=0, undetermined=0, code='a', stereo='s', mirror='s', text=''):
    from difflinker_amd import metrics
    return metrics.StereoRecord(centres, linker, bonds, bonds_linker, undetermined, centres + bonds + undetermined, code, stereo, mirror,
                                int(stereo != mirror), int(undetermined == 0), text)


def test_compute_stereo_on_hand_written_rows(tmp_path):
    from difflinker_amd import metrics
    good = metrics.Molecule(0, 0, 1, 0, None)
    broken = metrics.Molecule(0, 1, 1, 0, None)
    empty = metrics.compute_stereo([], [])
    assert set(empty) == set(metrics.STEREO_NAMES) and not any(empty.values())
    assert set(metrics.compute_stereo([], [], true=[], true_rows=[])) == set(metrics.STEREO_NAMES + metrics.STEREO_TRUE_NAMES)
    rows = [record(2, 1, 1, 0, 1, stereo='r', mirror='s'), record(2, 1, 1, 1, 0, stereo='s', mirror='r'),
            record(0, 0, 0, 0, 0, code='b', stereo='m', mirror='m'), record(2, 0, 0, 0, 0, stereo='r', mirror='s')]
    out = metrics.compute_stereo(rows, [good, good, good, broken])
    assert out == {'stereocentres_per_molecule': 1.5, 'stereocentres_per_molecule_linker': 0.5, 'stereo_bonds_per_molecule': 0.5,
                   'stereo_bonds_per_molecule_linker': 0.25, 'stereo_undetermined': 1 / 9, 'chiral_fraction': 0.75,
                   'stereo_uniqueness': 1.0}
    assert metrics.compute_stereo(rows, [good] * 4)['stereo_uniqueness'] == 0.75
    truth = [record(2, 1, 1, 0, 0, stereo='r', mirror='s')] * 4
    out = metrics.compute_stereo(rows, [good] * 4, [good] * 4, truth, input_index=[0, 0, 1, 2])
    # three samples have the true plain code: one recovered (and the broken one: recovery asks for the code alone), one mirrored
    assert out['stereo_recovery'] == 2 / 3 and out['stereo_mirror'] == 1 / 3 and out['stereo_recovered_inputs'] == 2 / 3
    none = metrics.compute_stereo(rows, [good] * 4, [good] * 4, [record(code='z')] * 4)
    assert none['stereo_recovery'] == none['stereo_mirror'] == none['stereo_recovered_inputs'] == 0.0
    assert metrics.compute_stereo(rows, [good] * 4, [broken] * 4, truth)['stereo_uniqueness'] == 0.0
    with pytest.raises(ValueError):
        metrics.compute_stereo(rows, [good] * 4, [good] * 4, truth[:2])
    path = tmp_path / 'stereo.json'
    metrics.write_stereo_json(path, ['a.sdf', 'b.sdf'], rows[:2])
    import json
    written = json.load(open(path))
    assert [w['file'] for w in written] == ['a.sdf', 'b.sdf'] and set(written[0]) == {'file'} | set(metrics.STEREO_JSON)
    assert written[0]['stereo_code'] == 'r' and written[0]['centres'] == 2 and written[1]['double_bonds_linker'] == 1
