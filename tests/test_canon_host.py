"""The canonical labelling on the host: the declarations of ``dl_canonical_ranks``, the properties of the rule as
``tests/canon_ref.py`` states it - which the kernel inherits through bit equality (``tests/test_gpu_canon.py``) - and the
SMILES writer ``molecule_builder.smiles``."""
import ctypes
import inspect
import itertools
import os
import random
import re
import sys

import pytest

import canon_cases as cc
import canon_ref as cr
import mol_keys_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM, N_RENUMBERINGS = 100, 5


def graph(types, bonds):
    from difflinker_amd.metrics import Graph
    return Graph(list(types), list(bonds), None)


def labelled(types, bonds, **kwargs):
    """``(form, code, string, leaves, budget, rank)`` of one molecule under the reference."""
    from difflinker_amd.molecule_builder import smiles
    rank, code, leaves, budget = cr.search(types, bonds, **kwargs)
    return cr.form(types, bonds, rank), code, smiles(types, bonds, rank), leaves, budget, rank


@pytest.fixture(scope='module')
def molecules():
    """name -> (types, bonds) of the named cases and the seeded random graphs, with their labelling computed once."""
    out = {name: (types, bonds) for name, (types, bonds, _) in cc.NAMED.items()}
    out.update({f'random_{seed}': cc.random_graph(seed) for seed in range(N_RANDOM)})
    return {name: (types, bonds, labelled(types, bonds)) for name, (types, bonds) in out.items()}


# ---- declarations --------------------------------------------------------------------------------------------------------------
def test_export_declaration_and_constants():
    import __graft_entry__ as g
    from difflinker_amd import _lib
    at = _lib.EXPORTS.index('dl_bonds_workspace_bytes')
    assert _lib.EXPORTS[at + 1:at + 3] == ('dl_canonical_ranks', 'dl_perceive_bonds') and _lib.ABI_VERSION == 7
    assert _lib.CANON_ENTRY_POINTS == {'dl_canonical_ranks': _lib.DLCanonArgs}
    assert not any('dl_canonical_ranks' in t for t in (_lib.STRUCT_ENTRY_POINTS, _lib.SELECT_ENTRY_POINTS, _lib.RELAX_ENTRY_POINTS))
    assert _lib.entry_struct('dl_canonical_ranks') is _lib.DLCanonArgs and _lib._stream_is_field(_lib.DLCanonArgs)
    assert _lib.entry_struct('dl_relax_molecules') is _lib.DLRelaxArgs
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_canonical_ranks(const dl_canon_args* args);' in header
    assert ' *   dl_canonical_ranks ' in header[:header.index('#ifndef DIFFLINKER_HIP_H')], 'listed in the opening comment'
    section = header[header.index('(canon.hip)'):]
    for words in ('NOT RDKit', 'tests/canon_ref.py', 'exactly n rounds', 'strictly smaller', 'twins', 'earlier leaf stays',
                  'DL_CANON_MAX_DEPTH (32)', 'plain stores only', '2 * rank[i] + (i == v ? 0 : 1)'):
        assert words in section, words
    for name, value in (('MAX_ATOMS', 256), ('MAX_BONDS', 2048), ('MAX_DEPTH', 32), ('MAX_LEAVES', 65536), ('TOO_LARGE', 4),
                        ('BAD_BOND', 8), ('BUDGET', 256)):
        assert re.search(rf'#define DL_CANON_{name} {value}\b', header) and getattr(_lib, f'DL_CANON_{name}') == value
    assert (cr.MAX_ATOMS, cr.MAX_BONDS, cr.MAX_DEPTH, cr.MAX_LEAVES, cr.TOO_LARGE, cr.BAD_BOND, cr.BUDGET) == (
        _lib.DL_CANON_MAX_ATOMS, _lib.DL_CANON_MAX_BONDS, _lib.DL_CANON_MAX_DEPTH, _lib.DL_CANON_MAX_LEAVES,
        _lib.DL_CANON_TOO_LARGE, _lib.DL_CANON_BAD_BOND, _lib.DL_CANON_BUDGET)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'canon.hip') in g.HIP_SOURCES
    struct = header[header.index('typedef struct dl_canon_args {'):header.index('} dl_canon_args;')]
    body = re.sub(r'/\*.*?\*/', '', struct[struct.index('{') + 1:])
    declared, kinds = [], []
    for statement in body.split(';'):
        if not statement.strip():
            continue
        kind = 'pointer' if '*' in statement else statement.split()[0]
        names = re.findall(r'(\w+)\s*(?:,|$)', statement.strip())
        declared += names
        kinds += [kind] * len(names)
    fields = _lib.DLCanonArgs._fields_
    assert declared == [f[0] for f in fields], 'the ctypes structure lists the header\'s members in order'
    assert [{'pointer': ctypes.c_void_p, 'int32_t': ctypes.c_int32}[k] for k in kinds] == [f[1] for f in fields]
    lib = _lib.load()
    assert hasattr(lib, 'dl_canonical_ranks')
    bad = _lib.DLCanonArgs(B=1, N=4, nf=8, capacity=0, max_leaves=0)
    assert lib.dl_canonical_ranks(ctypes.byref(bad)) == -1, 'max_leaves below 1 is an argument error, before any device work'
    bad.max_leaves = _lib.DL_CANON_MAX_LEAVES + 1
    assert lib.dl_canonical_ranks(ctypes.byref(bad)) == -1
    assert lib.dl_canonical_ranks(ctypes.byref(_lib.DLCanonArgs(B=0, N=4, nf=8, capacity=0, max_leaves=256))) == 0, \
        'an empty batch is DL_OK without a launch'


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def test_the_form_the_code_and_the_string_do_not_depend_on_the_numbering(molecules):
    for name, (types, bonds, (form, code, text, leaves, budget, rank)) in molecules.items():
        assert sorted(rank) == list(range(len(types))) and not budget, name
        rng = random.Random(name)
        for _ in range(N_RENUMBERINGS):
            t2, b2 = cc.renumber(types, bonds, rng)
            again = labelled(t2, b2)
            assert again[:4] == (form, code, text, leaves), name


def test_equal_codes_exactly_for_the_same_molecule(molecules):
    """Against the project's own identity, the exact graph match of ``metrics.same_molecule``: the random graphs and every
    pair of named cases; the renumbered copy of each random graph supplies the equal pairs."""
    from difflinker_amd.metrics import same_molecule
    names = list(molecules)
    copies = {}
    rng = random.Random(7)
    for name in names:
        if name.startswith('random_'):
            t2, b2 = cc.renumber(*molecules[name][:2], rng)
            copies[name + '_copy'] = (t2, b2, labelled(t2, b2))
    everything = {**molecules, **copies}
    equal = 0
    for a, b in itertools.combinations(everything, 2):
        same = same_molecule(graph(*everything[a][:2]), graph(*everything[b][:2]))
        assert (everything[a][2][1] == everything[b][2][1]) == same, (a, b)
        equal += same
    assert equal >= N_RANDOM


def test_the_code_tells_what_the_key_cannot(molecules):
    key = lambda name: kr.colours_and_key(*molecules[name][:2])[1]           # noqa: E731
    code = lambda name: molecules[name][2][1]                                # noqa: E731
    assert key('cubane') == key('cuneane') and code('cubane') != code('cuneane')
    assert code('benzene') != code('six_ring')


def test_leaf_counts_of_the_named_cases(molecules):
    for name, (_, _, leaves) in cc.NAMED.items():
        if leaves is not None:
            assert molecules[name][2][3] == leaves, name


def test_branching_matters_for_cuneane():
    """The variant that never branches gives different forms under renumbering: the search is needed, not decoration."""
    types, bonds, _ = cc.NAMED['cuneane']
    rng = random.Random(3)
    forms = set()
    for _ in range(20):
        t2, b2 = cc.renumber(types, bonds, rng)
        forms.add(cr.form(t2, b2, cr.search(t2, b2, branch=False)[0]))
    assert len(forms) > 1


def test_the_leaf_budget():
    types, bonds, _ = cc.NAMED['cubane']
    for max_leaves, leaves, budget in ((1, 1, True), (4, 4, True), (47, 47, True), (48, 48, False), (256, 48, False)):
        rank, _, got, flagged = cr.search(types, bonds, max_leaves=max_leaves)
        assert (got, flagged) == (leaves, budget) and sorted(rank) == list(range(8)), max_leaves
    out = cr.canonical_ranks(types, bonds, max_leaves=4, status_in=2)
    assert out['status'] == 2 | cr.BUDGET and out['n_leaves'] == 4


def test_the_depth_budget():
    """33 separate two-atom pieces: every branching level individualises one atom of one more piece, so the first path has 33
    branching levels; the 33rd does not branch and sets the bit.  One piece fewer stays within the limit."""
    pieces = lambda k: ([cc.C] * (2 * k), [(2 * i, 2 * i + 1, 1) for i in range(k)])       # noqa: E731
    rank, _, leaves, budget = cr.search(*pieces(cr.MAX_DEPTH + 1), max_leaves=2)
    assert budget and leaves == 2 and sorted(rank) == list(range(2 * cr.MAX_DEPTH + 2))
    rank, _, leaves, budget = cr.search(*pieces(3), max_leaves=2, max_depth=3)
    assert budget and leaves == 2, 'the leaf budget alone'
    rank, _, leaves, budget = cr.search(*pieces(3), max_leaves=65536, max_depth=3)
    assert not budget and leaves == 6 * 4 * 2
    assert cr.search(*pieces(3), max_leaves=65536, max_depth=2)[3]


def test_bad_entries_and_limits():
    types, bonds = [cc.C] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1)]
    clean = cr.canonical_ranks(types, bonds)
    assert clean['status'] == 0 and sorted(clean['rank']) == [0, 1, 2, 3]
    assert cr.canonical_ranks(types, bonds + [(0, 4, 1)])['status'] == cr.BAD_BOND
    assert cr.canonical_ranks(types, bonds + [(2, 2, 1)])['status'] == cr.BAD_BOND
    assert cr.canonical_ranks(types, bonds + [(0, 1, 4)])['status'] == cr.BAD_BOND
    assert cr.canonical_ranks(types, bonds + [(1, 0, 1)])['status'] == cr.BAD_BOND, 'a repeated pair, in either orientation'
    dropped = cr.canonical_ranks(types, bonds, keep=[True, False, True, True])
    assert dropped['rank'][1] == -1 and sorted(dropped['rank']) == [-1, 0, 1, 2]
    assert dropped['code'] == cr.canonical_ranks([cc.C] * 3, [(1, 2, 1)])['code']
    assert cr.canonical_ranks([], [])['code'] == kr.mix2(kr.mix2(kr.SEED_KEY, 0), 0)
    big = cr.canonical_ranks(*cc.chain(257))
    assert big == dict(rank=[-1] * 257, code=0, n_leaves=0, status=cr.TOO_LARGE)


# ---- the writer ----------------------------------------------------------------------------------------------------------------
def test_the_string_fixtures(molecules):
    for name, text in cc.STRINGS.items():
        assert molecules[name][2][2] == text, name


def test_every_string_reads_back_as_its_molecule(molecules):
    from difflinker_amd.metrics import same_molecule
    for name, (types, bonds, (_, _, text, *_)) in molecules.items():
        t2, b2, _, _ = cc.parse_smiles(text)
        if name.startswith('chain'):
            assert sorted(t2) == sorted(types) and len(b2) == len(bonds) and text.count('C') == len(types), name
        else:
            assert same_molecule(graph(types, bonds), graph(t2, b2)), (name, text)


def test_ring_numbers_are_reused_and_overvalent_atoms_bracketed(molecules):
    for name in ('spiro', 'decalin'):
        text = molecules[name][2][2]
        assert cc.parse_smiles(text)[3] == 2, (name, text)
    for name, element in (('nitromethane', cc.N), ('sulfone', cc.S)):
        types, _, bracketed, _ = cc.parse_smiles(molecules[name][2][2])
        assert [types[k] for k in bracketed] == [element], name
    assert '[' not in molecules['acetic_acid'][2][2]


def test_a_long_chain_needs_no_recursion(molecules):
    from difflinker_amd.molecule_builder import smiles
    types, bonds, (_, _, text, *_rest) = molecules['chain_256']
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(len(inspect.stack()) + 60)
    try:
        assert smiles(types, bonds, _rest[2]) == text
    finally:
        sys.setrecursionlimit(limit)
    assert text.count('C') == 256


def test_more_than_99_open_closures_give_none():
    """A ladder walked down one rail and back up the other: every rung is open until the way back reaches it."""
    from difflinker_amd.molecule_builder import smiles

    def ladder(n):
        rails = [(i, i + 1, 1) for i in range(n - 1)] + [(n - 1, 2 * n - 1, 1)] + [(n + i, n + i + 1, 1) for i in range(n - 1)]
        return [cc.C] * (2 * n), rails + [(i, n + i, 1) for i in range(n - 1)], list(range(2 * n))
    assert smiles(*ladder(101)) is None, '100 rungs open at once'
    text = smiles(*ladder(100))
    assert text is not None and '%99' in text and cc.parse_smiles(text)[3] == 99
