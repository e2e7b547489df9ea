"""The substructure search on the host: the pattern compiler (``difflinker_amd/patterns.py``), the restatement of the rule
(``tests/substructure_ref.py``) against the hand-derived table of ``tests/substructure_cases.py`` - which the kernel inherits
through bit equality (``tests/test_gpu_substructure.py``) - the budget arithmetic, and the declarations of
``dl_substructure_match``."""
import ctypes
import functools
import os
import re

import pytest

import substructure_cases as sc
import substructure_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_LIST = os.environ.get('DIFFLINKER_PAINS_LIST', '')         # the path of the reference's wehi_pains.csv, where there is one


def P():
    from difflinker_amd import patterns
    return patterns


def restated(symbols, bonds, aromatic, **more):
    from difflinker_amd import const
    return sr.Molecule([P().ATOMIC_NUMBER[s] for s in symbols], [const.DEFAULT_VALENCE[s] for s in symbols], bonds,
                       [k in aromatic for k in range(len(bonds))], **more)


def tokens(compiled, atom):
    off, n = compiled.atoms[atom, 2].item(), compiled.atoms[atom, 3].item()
    return compiled.preds[off:off + n].tolist()


# ---- the compiler ------------------------------------------------------------------------------------------------------------------
def test_accepted_forms_compile_to_the_three_level_form():
    p = P()
    one = p.compile_patterns([('[#6,#7;!R;D2&H1]', 'x')])
    assert (one.n_sub, one.n_top, one.names, one.level_end) == (0, 1, ['x'], [])
    assert tokens(one, 0) == [p.token(p.P_ELEM, 6) | p.END_AND, p.token(p.P_ELEM, 7) | p.END_AND | p.END_OR,
                              p.token(p.P_RING, 0, True) | p.END_AND | p.END_OR,
                              p.token(p.P_D, 2), p.token(p.P_H, 1) | p.END_AND | p.END_OR]
    # `!` binds to the primitive, juxtaposition is `&`, `&` binds tighter than `,`, `,` tighter than `;`
    assert tokens(p.compile_patterns(['[!CH2,N]']), 0) == [p.token(p.P_ELEM_ALIPH, 6, True), p.token(p.P_H, 2) | p.END_AND,
                                                         p.token(p.P_ELEM_ALIPH, 7) | p.END_AND | p.END_OR]
    for text, want in (('C', p.token(p.P_ELEM_ALIPH, 6)), ('c', p.token(p.P_ELEM_AROM, 6)), ('Cl', p.token(p.P_ELEM_ALIPH, 17)),
                       ('[Br]', p.token(p.P_ELEM_ALIPH, 35)), ('*', p.token(p.P_TRUE)), ('a', p.token(p.P_AROM)),
                       ('A', p.token(p.P_AROM, 0, True)), ('[H]', p.token(p.P_H, 1)), ('[h]', p.token(p.P_HMIN, 1)),
                       ('[h2]', p.token(p.P_H, 2)), ('[D]', p.token(p.P_D, 1)), ('[X4]', p.token(p.P_X, 4)), ('[v3]', p.token(p.P_V, 3)),
                       ('[R]', p.token(p.P_RING)), ('[R0]', p.token(p.P_RING, 0, True)), ('[r]', p.token(p.P_RING)),
                       ('[r6]', p.token(p.P_RSIZE, 6)), ('[x2]', p.token(p.P_XRING, 2)), ('[x]', p.token(p.P_RING)),
                       ('[+]', p.token(p.P_TRUE, 0, True)), ('[+0]', p.token(p.P_TRUE)), ('[-2]', p.token(p.P_TRUE, 0, True)),
                       ('[--]', p.token(p.P_TRUE, 0, True)), ('[!+]', p.token(p.P_TRUE)), ('[#16]', p.token(p.P_ELEM, 16))):
        assert tokens(p.compile_patterns([text]), 0) == [want | p.END_AND | p.END_OR], text
    assert p.compile_patterns(['C', 'N']).names == ['0', '1'], 'the name defaults to the row number'


def test_bonds_compile_to_masks_over_the_twelve_states():
    p = P()
    state = p.bond_state
    single, double, triple = (sum(1 << state(o, 0, r) for r in (0, 1)) for o in (1, 2, 3))
    aromatic = sum(1 << state(o, 1, r) for o in (1, 2, 3) for r in (0, 1))
    ring = sum(1 << state(o, a, 1) for o in (1, 2, 3) for a in (0, 1))
    for text, want in (('CC', single | aromatic), ('C-C', single), ('C=C', double), ('C#C', triple), ('C:C', aromatic),
                       ('C~C', p.ANY_BOND), ('C@C', ring), ('C!@C', p.ANY_BOND & ~ring), ('C-,:C', single | aromatic),
                       ('C=,:C', double | aromatic), ('C-;!@C', single & ~ring), ('C-@C', single & ring), ('C!-C', p.ANY_BOND & ~single),
                       ('C=,#;@C', (double | triple) & ring)):
        compiled = p.compile_patterns([text])
        assert compiled.atoms[1].tolist()[:2] == [0, want], text
    closed = p.compile_patterns(['C=1CCC1', 'C1CCC=1', 'C:1CC:1', 'C%12CC%12'])
    assert closed.closures.tolist() == [[0, double], [0, double], [0, aromatic], [0, single | aromatic]]
    assert closed.atoms[3].tolist()[4:] == [0, 1] and closed.atoms[0].tolist()[:2] == [-1, single | aromatic]
    # a closure is a check on the LATER atom against the earlier one, whichever of the two the digit closes on
    early = p.compile_patterns(['C(CC=3)3', 'C(C3)C3'])
    assert early.closures.tolist() == [[0, double], [1, single | aromatic]]
    assert early.atoms[:, 5].tolist() == [0, 0, 1, 0, 0, 1] and early.atoms[:, 0].tolist() == [-1, 0, 1, -1, 0, 0]


def test_the_search_order_is_the_order_written():
    compiled = P().compile_patterns(['C(N)(O1)SC1F'])
    assert compiled.atoms[:, 0].tolist() == [-1, 0, 0, 0, 3, 4], 'every atom hangs off the atom it was written after'
    assert compiled.atoms[:, 5].tolist() == [0, 0, 0, 0, 1, 0] and compiled.closures.tolist()[0][0] == 2


def test_the_hydrogen_merge():
    p = P()
    merged = p.compile_patterns(['[#7](-[#1])-[#1]', '[#1][#6]([#1])=O', 'c:1:c(:c-[#1]):c:c:c:1'])
    assert merged.pat[:, 1].tolist() == [1, 2, 6]
    assert tokens(merged, 0) == [p.token(p.P_ELEM, 7) | p.END_AND | p.END_OR, p.token(p.P_HMIN, 2) | p.END_AND | p.END_OR]
    assert tokens(merged, 1)[-1] == p.token(p.P_HMIN, 2) | p.END_AND | p.END_OR and merged.atoms[1:3, 0].tolist() == [-1, 0], \
        'a hydrogen written first leaves the next atom as the root'
    assert merged.atoms[3:9, 0].tolist() == [-1, 0, 1, 1, 3, 4], 'parents renumbered past the removed leaf'
    assert tokens(p.compile_patterns(['[!#1]']), 0) == [p.token(p.P_ELEM, 1, True) | p.END_AND | p.END_OR], 'no atom, a primitive'


@pytest.mark.parametrize('smarts,construct', [
    ('C[C@H](N)O', 'stereo'), ('C[C@@](N)(O)F', 'stereo'), ('C/C=C/C', 'stereo'), ('C\\C=C', 'stereo'),
    ('[13C]', 'isotope'), ('[C:1]', 'atom map'), ('[C^2]', '^n'), ('C.C', '. components'), ('[R2]', 'R<n>'), ('[R1]', 'R<n>'),
    ('', 'zero-atom'), ('[#1]', 'hydrogen'), ('[#1]=C', 'hydrogen'), ('C[#1]C', 'hydrogen'), ('[#1,#6]', 'hydrogen'),
    ('[#1][#1]', 'hydrogen'), ('C' * 49, 'pattern atoms'), ('[' + 'C' * 33 + ']', 'primitives'),
    ('[$([$([$([$([$(C)])])])])]', 'nesting levels'), ('C1CC', 'ring closure'), ('C(C', 'unclosed ('), ('[C', 'unclosed ['),
    ('C)', 'unbalanced )'), ('[$(C]', 'unclosed $('), ('C=', 'bond without an atom'), ('[Qq]', 'atom primitive'), ('C11', 'one atom'),
    ('[D256]', 'above 255'), ('[H65536]', 'above 255'), ('[x300]', 'above 255'), ('[r65536]', 'above 255'), ('[v999;X2]', 'above 255'),
    ('C1C1', 'two bonds'), ('C(C1)1', 'two bonds'), ('C12CC12', 'two bonds'), ('N[$([' + 'C' * 33 + '])]', 'primitives'),
])
def test_every_rejection_names_the_construct(smarts, construct):
    p = P()
    with pytest.raises(p.PatternError) as caught:
        p.compile_patterns([('C', 'fine'), (smarts, 'bad')])
    assert caught.value.row == 1 and construct in caught.value.construct and isinstance(caught.value.column, int)
    assert 'row 1' in str(caught.value) and construct in str(caught.value)


def test_rejections_point_at_the_column():
    p = P()
    for smarts, column in (('CC[C@H]', 4), ('CCC.C', 3), ('C[$(C[13C])]', 6), ('CC/C', 2)):
        with pytest.raises(p.PatternError) as caught:
            p.compile_patterns([smarts])
        assert caught.value.column == column, smarts


def test_too_many_sub_patterns():
    p = P()
    rows = [f'[$([#{2 + k % 100}][D{k // 100}])]' for k in range(p.MAX_SUBPATTERNS)]
    assert p.compile_patterns(rows).n_sub == p.MAX_SUBPATTERNS
    with pytest.raises(p.PatternError) as caught:
        p.compile_patterns(rows[:40] + ['[$(CO)]'] + rows[40:])
    assert 'sub-patterns' in caught.value.construct and caught.value.row == p.MAX_SUBPATTERNS


def test_sub_patterns_are_shared_and_ordered_by_level():
    p = P()
    compiled = p.compile_patterns(['[$(c:[$(c[OH])])]', '[$(c[OH]),$(C=O)]', '[C;!$(C=O)]N', '[$([$([$([$(CF)])])])]'])
    assert compiled.sub_texts == ['c[OH]', 'C=O', 'CF', 'c:[$(c[OH])]', '[$(CF)]', '[$([$(CF)])]', '[$([$([$(CF)])])]']
    assert compiled.sub_levels == [0, 0, 0, 1, 1, 2, 3] and compiled.level_end == [3, 5, 6, 7]
    assert (compiled.n_sub, compiled.n_top) == (7, 4) and compiled.pat[:, 2].tolist() == [0, 0, 0, 1, 1, 2, 3, 4, 4, 4, 4]
    assert tokens(compiled, compiled.pat[7, 0].item()) == [p.token(p.P_REC, 3) | p.END_AND | p.END_OR]
    first = compiled.pat[8, 0].item()
    assert tokens(compiled, first) == [p.token(p.P_REC, 0) | p.END_AND, p.token(p.P_REC, 1) | p.END_AND | p.END_OR]
    assert tokens(compiled, compiled.pat[9, 0].item())[1] == p.token(p.P_REC, 1, True) | p.END_AND | p.END_OR
    assert tokens(compiled, compiled.pat[3, 0].item() + 1) == [p.token(p.P_REC, 0) | p.END_AND | p.END_OR], 'a body reads lower levels'


def test_the_screen_counts_the_elements_a_pattern_needs():
    p = P()
    compiled = p.compile_patterns(['ClC(Cl)C(=O)[N,n]', '[#6,#7]O', '[!#6]'])
    assert compiled.pat[0, 3:7].tolist() == [17 | 2 << 8, 8 | 1 << 8, 7 | 1 << 8, 6 | 2 << 8]
    assert compiled.pat[1, 3:7].tolist() == [8 | 1 << 8, 0, 0, 0] and compiled.pat[2, 3:7].tolist() == [0, 0, 0, 0]


def test_the_pattern_file_format(tmp_path):
    p = P()
    path = tmp_path / 'list.csv'
    path.write_text('# a comment\n"[#6](=O)[Cl,Br]","<regId=acyl(3)>"\n\nC=O\n"c1ccccc1",ring,more\n')
    rows = p.read_pattern_file(str(path))
    assert rows == [('[#6](=O)[Cl,Br]', '<regId=acyl(3)>'), ('C=O', '1'), ('c1ccccc1', 'ring')]
    assert p.compile_patterns(rows).names == ['<regId=acyl(3)>', '1', 'ring']


def test_the_basic_catalogue():
    p = P()
    rows = p.read_pattern_file(p.basic_catalogue_path())
    compiled = p.load_catalogue('basic')
    assert compiled.names == list(sc.ALERTS) and len(rows) >= 16 and len(set(compiled.names)) == len(rows)
    for name in ('acyl_halide', 'aldehyde', 'peroxide', 'azide', 'epoxide', 'isocyanate', 'michael_acceptor', 'thiol', 'disulfide',
                 'sulfonyl_halide', 'nitroso', 'hydrazine'):
        assert name in compiled.names


@pytest.mark.skipif(not os.path.exists(REFERENCE_LIST), reason='DIFFLINKER_PAINS_LIST does not name the reference\'s pattern list')
def test_every_row_of_the_reference_list_compiles():
    p = P()
    rows = p.read_pattern_file(REFERENCE_LIST)
    compiled = p.compile_patterns(rows)
    assert len(rows) == compiled.n_top == 480 and len(compiled.level_end) == 2
    assert sum(1 for smarts, _ in rows if '$(' in smarts) == 61
    assert compiled.pat[:, 1].max().item() <= p.MAX_PATTERN_ATOMS and compiled.atoms[:, 3].max().item() <= p.MAX_PRED


# ---- the restatement against the hand-derived table ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.MOLECULES))
def test_the_restatement_gives_the_hand_derived_roots(name):
    expected = sc.EXPECTED[name]
    compiled = P().compile_patterns([smarts for smarts, _ in expected])
    out = sr.Matcher(compiled).match(restated(*sc.MOLECULES[name]))
    assert out['status'] == 0
    for p, (smarts, want) in enumerate(expected):
        assert out['roots'][p] == want, (name, smarts)
        assert out['first_root'][p] == (min(want) if want else -1), (name, smarts)
    assert out['n_hits'] == sum(1 for _, want in expected if want) and out['n_hits_marked'] == 0


def test_the_table_covers_every_primitive_true_and_negated():
    p = P()
    seen = set()
    for name, expected in sc.EXPECTED.items():
        compiled = p.compile_patterns([smarts for smarts, _ in expected])
        seen |= {(t & 0xFF, bool(t & p.NEG)) for t in compiled.preds.tolist()}
    assert seen == {(op, neg) for op in range(14) for neg in (False, True)}, 'every op of the table, plain and under !'


def test_every_alert_has_a_molecule_that_hits_and_one_that_does_not():
    compiled = P().load_catalogue('basic')
    matcher = sr.Matcher(compiled)
    for k, (name, (hit, miss)) in enumerate(sc.ALERTS.items()):
        assert matcher.match(restated(*sc.parse(hit)))['first_root'][k] >= 0, (name, hit)
        assert matcher.match(restated(*sc.parse(miss)))['first_root'][k] == -1, (name, miss)


def test_marks_keep_a_root_searching():
    """Phenol with the oxygen marked: ``cc`` from atom 1 maps (1, 0) first, which touches no marked atom; only ``ccO``-like maps
    do.  ``c:c-O`` from atom 1: the one map is (1, 0, 6)."""
    compiled = P().compile_patterns(['cc', 'c:c-O', 'c:c:c', 'O'])
    symbols, bonds, aromatic = sc.MOLECULES['phenol']
    out = sr.Matcher(compiled).match(restated(symbols, bonds, aromatic, marked=[k == 6 for k in range(7)]), with_marks=True)
    assert out['roots'] == [set(range(6)), {1, 5}, set(range(6)), {6}]
    assert out['roots_marked'] == [set(), {1, 5}, set(), {6}] and out['first_root_marked'] == [-1, 1, -1, 6]
    assert (out['n_hits'], out['n_hits_marked']) == (4, 2)


# ---- the budget ----------------------------------------------------------------------------------------------------------------------
def cubane(max_steps, smarts, marks):
    compiled = P().compile_patterns([smarts])
    mol = restated(*sc.MOLECULES['cubane'], marked=[False] * 8 if marks else None)
    return sr.Matcher(compiled).match(mol, max_steps=max_steps, with_marks=marks)


def test_budget_arithmetic_on_cubane():
    """``CC`` from any atom of cubane: the root is step 1, its lowest neighbour step 2 and the map is complete.  With marks and
    nothing marked the search goes on over the other two neighbours: 4 steps, and the finding stands when they run out."""
    assert set(cubane(4096, 'CC', False)['steps'].values()) == {2} and set(cubane(4096, 'CC', True)['steps'].values()) == {4}
    exact, short = cubane(2, 'CC', False), cubane(1, 'CC', False)
    assert exact['status'] == 0 and exact['first_root'] == [0]
    assert short['status'] == sr.BUDGET and short['first_root'] == [-1], 'the root alone used the budget up'
    exact, short = cubane(4, 'CC', True), cubane(3, 'CC', True)
    assert exact['status'] == 0 and exact['first_root'] == [0] and exact['first_root_marked'] == [-1]
    assert short['status'] == sr.BUDGET and short['first_root'] == [0] and short['first_root_marked'] == [-1], 'the finding stands'
    full = cubane(4096, 'C1CCC1', True)
    needed = max(full['steps'].values())
    assert needed > 20 and full['status'] == 0
    assert cubane(needed, 'C1CCC1', True)['status'] == 0
    short = cubane(needed - 1, 'C1CCC1', True)
    assert short['status'] == sr.BUDGET and short['first_root'] == [0] and short['roots'] == [set(range(8))]


def test_a_sub_pattern_out_of_budget_counts_as_no_match():
    compiled = P().compile_patterns(['[$(C1CCC1)]'])
    mol = restated(*sc.MOLECULES['cubane'])
    matcher = sr.Matcher(compiled)
    assert matcher.match(mol)['roots'] == [set(range(8))]
    out = matcher.match(mol, max_steps=3)
    assert out['roots'] == [set()] and out['status'] == sr.BUDGET


def test_status_bits_of_the_graph():
    compiled = P().compile_patterns(['CC'])
    matcher = sr.Matcher(compiled)
    z, dv = [6] * 4, [4] * 4
    chain = [(0, 1, 1), (1, 2, 1), (2, 3, 1)]
    assert matcher.match(sr.Molecule(z, dv, chain))['status'] == 0
    for extra in ((0, 4, 1), (2, 2, 1), (0, 1, 0), (0, 1, 4), (1, 0, 2)):
        assert matcher.match(sr.Molecule(z, dv, chain + [extra]))['status'] == sr.BAD_BOND, extra
    first = sr.Molecule(z, dv, [(0, 1, 2), (1, 0, 1)])
    assert first.bond(0, 1)[0] == 2, 'the first entry of a repeated pair gives the pair its order'
    big = matcher.match(sr.Molecule([6] * 257, [4] * 257, [(k, k + 1, 1) for k in range(256)]), status_in=2)
    assert big['status'] == 2 | sr.TOO_LARGE and big['first_root'] == [-1] and big['n_hits'] == 0
    kept = matcher.match(sr.Molecule([6] * 257, [4] * 257, [(k, k + 1, 1) for k in range(256)], keep=[k != 7 for k in range(257)]))
    assert kept['status'] == 0 and kept['first_root'] == [0]


# ---- the random batch of the GPU comparison ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_reference():
    molecules, smarts = sc.random_batch()
    compiled = P().compile_patterns(smarts)
    matcher = sr.Matcher(compiled)
    return molecules, smarts, compiled, [matcher.match(restated(*m)) for m in molecules]


def test_the_random_batch_is_neither_vacuous_nor_cut_short():
    molecules, smarts, compiled, results = random_reference()
    assert len(molecules) == 64 and 50 <= len(smarts) <= 70 and {len(m[0]) for m in molecules} >= {1, 2, 24}
    sizes = compiled.pat[compiled.n_sub:, 1].tolist()
    assert min(sizes) == 1 and max(sizes) >= 10 and compiled.n_sub >= 5 and len(compiled.level_end) >= 2
    assert compiled.closures.shape[0] >= 5, 'rings among the patterns'
    pairs = len(molecules) * len(smarts)
    hits = sum(out['n_hits'] for out in results)
    assert hits >= pairs / 4 and pairs - hits >= pairs / 4, (hits, pairs)
    assert not any(out['status'] for out in results), 'no budget bit, no bad bond'
    assert max(max(out['steps'].values(), default=0) for out in results) < 4096 / 8


# ---- the declarations ----------------------------------------------------------------------------------------------------------------
def test_export_declaration_and_constants():
    import __graft_entry__ as g
    from difflinker_amd import _lib, patterns
    at = _lib.EXPORTS.index('dl_size_train_backward')
    assert _lib.EXPORTS[at + 1] == 'dl_substructure_match' and _lib.ABI_VERSION == 7
    assert _lib.SUBSTRUCTURE_ENTRY_POINTS == {'dl_substructure_match': _lib.DLSubstructureArgs}
    assert not any('dl_substructure_match' in t for t in (_lib.STRUCT_ENTRY_POINTS, _lib.SELECT_ENTRY_POINTS,
                                                          _lib.RELAX_ENTRY_POINTS, _lib.CANON_ENTRY_POINTS))
    assert _lib.entry_struct('dl_substructure_match') is _lib.DLSubstructureArgs and _lib._stream_is_field(_lib.DLSubstructureArgs)
    assert _lib.DLSubstructureArgs._fields_[-1][0] == 'stream'
    assert _lib.entry_struct('dl_canonical_ranks') is _lib.DLCanonArgs
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    assert 'int32_t dl_substructure_match(const dl_substructure_args* args);' in header
    assert ' *   dl_substructure_match ' in header[:header.index('#ifndef DIFFLINKER_HIP_H')], 'listed in the opening comment'
    section = header[header.index('(substructure.hip)'):]
    for words in ('NOT RDKit', 'tests/substructure_ref.py', 'EVERY CANDIDATE TESTED IS ONE STEP', 'ascending kept', 'not induced',
                  'what it found stands', 'level by level', 'plain stores only', '(order - 1) + 3 * aromatic + 6 * ring',
                  'counts as no match'):
        assert words in section, words
    for name, value in (('MAX_ATOMS', 256), ('MAX_BONDS', 2048), ('MAX_PATTERN_ATOMS', patterns.MAX_PATTERN_ATOMS),
                        ('MAX_SUBPATTERNS', patterns.MAX_SUBPATTERNS), ('MAX_LEVELS', patterns.MAX_LEVELS),
                        ('MAX_PRED', patterns.MAX_PRED), ('TOO_LARGE', 4), ('BAD_BOND', 8), ('BUDGET', 512)):
        assert re.search(rf'#define DL_SUB_{name} {value}\b', header) and getattr(_lib, f'DL_SUB_{name}') == value, name
    assert (_lib.DL_SUB_TOO_LARGE, _lib.DL_SUB_BAD_BOND) == (_lib.DL_CANON_TOO_LARGE, _lib.DL_CANON_BAD_BOND)
    assert (sr.TOO_LARGE, sr.BAD_BOND, sr.BUDGET, sr.MAX_ATOMS, sr.MAX_BONDS) == (
        _lib.DL_SUB_TOO_LARGE, _lib.DL_SUB_BAD_BOND, _lib.DL_SUB_BUDGET, _lib.DL_SUB_MAX_ATOMS, _lib.DL_SUB_MAX_BONDS)
    assert os.path.join(ROOT, 'difflinker_amd', 'csrc', 'substructure.hip') in g.HIP_SOURCES
    struct = header[header.index('typedef struct dl_substructure_args {'):header.index('} dl_substructure_args;')]
    body = re.sub(r'/\*.*?\*/', '', struct[struct.index('{') + 1:])
    declared, kinds = [], []
    for statement in body.split(';'):
        if not statement.strip():
            continue
        kind = 'pointer' if '*' in statement else 'array' if '[' in statement else statement.split()[0]
        names = re.findall(r'(\w+)(?:\[\w+\])?\s*(?:,|$)', statement.strip())
        declared += names
        kinds += [kind] * len(names)
    fields = _lib.DLSubstructureArgs._fields_
    assert declared == [f[0] for f in fields], 'the ctypes structure lists the header\'s members in order'
    kinds_of = {'pointer': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'array': ctypes.c_int32 * _lib.DL_SUB_MAX_LEVELS}
    assert [kinds_of[k] for k in kinds] == [f[1] for f in fields]
    assert declared[-1] == 'stream'


def test_arguments_are_checked_before_any_device_work():
    from difflinker_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, 'dl_substructure_match')

    def call(**changed):
        values = dict(B=1, N=4, nf=8, capacity=0, n_sub=0, n_top=1, n_levels=0, max_steps=4096)
        values.update(changed)
        level_end = values.pop('level_end', ())
        args = _lib.DLSubstructureArgs(**values)
        for k, v in enumerate(level_end):
            args.level_end[k] = v
        return lib.dl_substructure_match(ctypes.byref(args))
    for bad in (dict(max_steps=0), dict(N=0), dict(N=1025), dict(nf=0), dict(nf=257), dict(capacity=-1), dict(B=-1),
                dict(n_sub=-1), dict(n_sub=_lib.DL_SUB_MAX_SUBPATTERNS + 1, n_levels=1, level_end=(_lib.DL_SUB_MAX_SUBPATTERNS + 1,)),
                dict(n_top=-1), dict(n_levels=_lib.DL_SUB_MAX_LEVELS + 1), dict(n_sub=2, n_levels=1, level_end=(1,)),
                dict(n_sub=2, n_levels=2, level_end=(2, 1)), dict(n_sub=1), dict(n_preds=-1), dict()):
        assert call(**bad) == -1, bad                                         # (the last: null pointers with B and n_top above 0)
    assert call(B=0) == 0 and call(n_top=0) == 0, 'an empty batch or an empty catalogue is DL_OK without a launch'
    assert call(B=0, n_sub=2, n_levels=2, level_end=(1, 2)) == 0


def test_compute_filters():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import FilterRecord, compute_filters
    records = [FilterRecord([], [], 0), FilterRecord(['thiol'], [], 0), FilterRecord(['thiol', 'azo'], ['azo'], 0),
               FilterRecord([], [], _lib.DL_SUB_BUDGET)]
    assert compute_filters(records) == {'filters_passed': 0.25, 'filters_passed_linker': 0.5, 'filter_hits_per_molecule': 0.75,
                                        'filters_budget': 0.25}
    both = compute_filters(records[:2], records[2:])
    assert both['true_filters_passed'] == 0.0 and both['true_filters_budget'] == 0.5 and both['filters_passed'] == 0.5
    assert compute_filters([])['filters_passed'] is None
    with pytest.raises(ValueError):
        compute_filters(records, records[:1])
