"""``dl_substructure_match`` (``csrc/substructure.hip``) on the GPU against ``tests/substructure_ref.py``, bit for bit - both
root tables, both counts and the status - on the hand-derived case table, on a seeded random batch and on the smallest shapes
at which each part of the kernel can go wrong; the wrappers' input handling; and ``analyze_patterns`` / ``generate --filters``
end to end."""
import filecmp
import functools
import json
import math
import os
import random

import pytest
import torch

import substructure_cases as sc
import substructure_ref as sr
from substructure_cases import FILLER, batch_of, molecule, on_device, rows_of

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FIELDS = ('first_root', 'first_root_marked', 'n_hits', 'n_hits_marked', 'status')


def compiled(smarts):
    from difflinker_amd.patterns import compile_patterns
    return compile_patterns(list(smarts))


def reference(molecules, N, patterns, scatter=True, capacity=None, max_steps=4096, with_marks=True):
    """What the kernel must write for ``batch_of(molecules, N, scatter, capacity)``: the five outputs as lists."""
    from difflinker_amd import const
    from difflinker_amd.patterns import ATOMIC_NUMBER
    capacity = max([len(m['entries']) for m in molecules] + [1]) if capacity is None else capacity
    matcher = sr.Matcher(patterns)
    out = {name: [] for name in FIELDS}
    for b, m in enumerate(molecules):
        given = len(m['entries']) if m['n_bonds'] is None else m['n_bonds']
        read = min(max(given, 0), capacity)
        entries = (m['entries'][:capacity] + [(FILLER,) * 3] * capacity)[:read]
        flags = [e in m['aromatic'] for e in range(read)]
        mol = sr.Molecule([ATOMIC_NUMBER[s] for s in m['symbols']], [const.DEFAULT_VALENCE[s] for s in m['symbols']], entries,
                          flags, m['keep'], m['marked'] if with_marks else None)
        got = matcher.match(mol, rows=rows_of(b, len(m['symbols']), N, scatter), max_steps=max_steps,
                            status_in=m['status'] | (sr.OVERFLOW if given > capacity else 0), with_marks=with_marks)
        for name in FIELDS:
            out[name].append(got[name])
    return out


def launch(batch, patterns, max_steps=4096, with_drop=True, with_marks=True, with_flags=True, place=lambda t: t.to(DEV)):
    from difflinker_amd.metrics import match_patterns
    one_hot, mask, drop, mark, found, flags = batch
    x = torch.zeros(one_hot.shape[0], one_hot.shape[1], 3)
    got = match_patterns(place(one_hot), x.to(DEV), place(mask), on_device(found, place), place(flags) if with_flags else None,
                         patterns, True, drop_mask=place(drop) if with_drop else None,
                         mark_mask=place(mark) if with_marks else None, max_steps=max_steps)
    return got._asdict()


def assert_equals_reference(got, want, names=None):
    for name in FIELDS:
        a = got[name].cpu().tolist()
        assert len(a) == len(want[name]), name
        for b in range(len(a)):
            assert a[b] == want[name][b], (name, b, names[b] if names else None)


def check(molecules, N, patterns, names=None, **how):
    """One launch against the reference; returns the kernel's outputs."""
    launch_how = {k: how.pop(k) for k in ('with_drop', 'with_flags') if k in how}
    got = launch(batch_of(molecules, N, how.get('scatter', True), how.get('capacity')), patterns,
                 max_steps=how.get('max_steps', 4096), with_marks=how.get('with_marks', True), **launch_how)
    assert_equals_reference(got, reference(molecules, N, patterns, **how), names)
    return got


def chain(n, symbol='C'):
    return molecule([symbol] * n, [(k, k + 1, 1) for k in range(n - 1)])


def named(name, **more):
    return molecule(*sc.MOLECULES[name], **more)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_table():
    """Every pattern of the hand-derived table and every alert in ONE catalogue, every molecule of both in one batch."""
    smarts = sorted({s for rows in sc.EXPECTED.values() for s, _ in rows})
    from difflinker_amd.patterns import basic_catalogue_path, read_pattern_file
    alerts = read_pattern_file(basic_catalogue_path())
    patterns = compiled([(s, s) for s in smarts] + alerts)
    names = list(sc.MOLECULES) + [f'{alert} {which}' for alert in sc.ALERTS for which in ('hit', 'miss')]
    molecules = [named(name) for name in sc.MOLECULES] + [molecule(*sc.parse(text)) for pair in sc.ALERTS.values() for text in pair]
    return smarts, patterns, names, molecules


def test_the_case_table_in_one_launch():
    smarts, patterns, names, molecules = case_table()
    got = check(molecules, 16, patterns, names, with_marks=False)
    first = got['first_root'].cpu().tolist()
    at = {s: p for p, s in enumerate(smarts)}
    for b, name in enumerate(sc.MOLECULES):                                  # the hand-derived roots, not the restatement's
        rows = rows_of(b, len(sc.MOLECULES[name][0]), 16, True)
        for s, want in sc.EXPECTED[name]:
            assert first[b][at[s]] == (rows[min(want)] if want else -1), (name, s)
    offset = len(sc.MOLECULES)
    for k, alert in enumerate(sc.ALERTS):
        assert first[offset + 2 * k][len(smarts) + k] >= 0 and first[offset + 2 * k + 1][len(smarts) + k] == -1, alert
    assert int(got['status'].abs().sum()) == 0 and int(got['first_root_marked'].max()) == -1


def test_the_random_batch():
    molecules, smarts = sc.random_batch()
    patterns = compiled(smarts)
    batch = [molecule(*m, marked=[random.Random(b * 31 + k).random() < 0.3 for k in range(len(m[0]))]) for b, m in enumerate(molecules)]
    got = check(batch, 24, patterns)
    hits = int(got['n_hits'].sum())
    assert len(batch) * len(smarts) / 4 <= hits <= 3 * len(batch) * len(smarts) / 4 and int(got['status'].abs().sum()) == 0
    assert 0 < int(got['n_hits_marked'].sum()) < hits
    check(batch, 24, patterns, with_marks=False, scatter=False)


# ---- the shapes at which it can go wrong ------------------------------------------------------------------------------------------------
def test_empty_batch_and_empty_catalogue():
    patterns = compiled(['CC', 'N'])
    got = launch(batch_of([], 5), patterns)
    assert [tuple(got[name].shape) for name in FIELDS] == [(0, 2), (0, 2), (0,), (0,), (0,)]
    none = compiled([])
    assert (none.n_top, none.n_sub) == (0, 0)
    got = launch(batch_of([named('benzene'), molecule(['C', 'O'], [(0, 1, 2)], status=2)], 8), none)
    assert [tuple(got[name].shape) for name in FIELDS] == [(2, 0), (2, 0), (2,), (2,), (2,)]
    assert got['n_hits'].tolist() == [0, 0] and got['n_hits_marked'].tolist() == [0, 0] and got['status'].tolist() == [0, 2]
    cut = batch_of([named('benzene'), chain(3)], 8, capacity=2)
    assert launch(cut, none)['status'].tolist() == launch(cut, patterns)['status'].tolist() == [sr.OVERFLOW, 0], \
        'a list cut short is flagged with an empty catalogue as with any other'


@functools.lru_cache(maxsize=None)
def edge_molecules():
    interleaved = [k % 2 == 0 for k in range(14)]                            # pocket rows between the ligand's
    ring14 = [(k, (k + 2) % 14, 1) for k in range(0, 14, 2)] + [(k, k + 1, 1) for k in range(0, 14, 2)]
    return {
        'no atoms': molecule([], []),
        'one atom': molecule(['O'], []),
        'everything dropped': molecule(['C'] * 3, [(0, 1, 1), (1, 2, 1)], keep=[False] * 3),
        'status carried': molecule(['C', 'O'], [(0, 1, 2)], status=2),
        'pocket rows interleaved': molecule(['C', 'N'] * 7, ring14, keep=interleaved, marked=[k == 12 for k in range(14)]),
        'repeated pair': molecule(['C'] * 4, [(0, 1, 2), (1, 2, 1), (2, 3, 1), (1, 0, 1)]),
        'order 0': molecule(['C'] * 4, [(0, 1, 1), (1, 2, 0), (2, 3, 1)]),
        'entry out of range and a loop': molecule(['C'] * 4, [(0, 1, 1), (1, 1, 1), (2, 4, 1), (2, 3, 1)]),
        'negative count': molecule(['C'] * 3, [(0, 1, 1), (1, 2, 1)], n_bonds=-5),
        'chain 256': chain(256),
        'chain 257': chain(257),
        'chain 257, one dropped': molecule(['C'] * 257, chain(257)['entries'], keep=[k != 128 for k in range(257)]),
        'chain 47': chain(47),
        'benzene': named('benzene'), 'phenol': named('phenol', marked=[k == 6 for k in range(7)]), 'cubane': named('cubane'),
        'biphenyl': named('biphenyl'), 'rhodanine': named('rhodanine'),
    }


def test_every_edge_shape_in_one_launch():
    """33 patterns, so that every loop over patterns has a tail: among them one of the largest size a pattern may have, which
    fits the chains of 256 and of 48 or more atoms only, and patterns larger than most molecules."""
    from difflinker_amd import _lib
    names = list(edge_molecules())
    molecules = [edge_molecules()[name] for name in names]
    smarts = ['C' * _lib.DL_SUB_MAX_PATTERN_ATOMS, 'C' * 47, 'CC', 'C=C', 'C', 'N', 'O', '*', 'c1ccccc1', 'cO', 'C1CCC1', 'CCCC',
              '[D1]', '[D2]', '[R]', '[r4]', 'C~C~C', '[$(CC)]', '[!$(CC)]', 'c-c', 'S=C', '[#6]1[#16][#6][#7][#6]1', 'CN', 'C@C',
              'C!@C', '[H3]', '[H2]', '[X4]', '[v4]', 'c:c:c:c:c:c', '[CH2]([CH2])[CH2]', 'C(C)(C)C', 'CCCCCCCCCCCCCCCC']
    assert len(smarts) == 33
    patterns = compiled(smarts)
    got = check(molecules, 300, patterns, names, capacity=256)
    at = {name: b for b, name in enumerate(names)}
    first, status = got['first_root'].cpu().tolist(), got['status'].cpu().tolist()
    assert status[at['chain 257']] == sr.TOO_LARGE and first[at['chain 257']] == [-1] * 33 and status[at['chain 257, one dropped']] == 0
    assert first[at['chain 256']][0] >= 0 and first[at['chain 47']][0] == -1 and first[at['chain 47']][1] >= 0
    assert status[at['repeated pair']] == status[at['order 0']] == status[at['entry out of range and a loop']] == sr.BAD_BOND
    assert first[at['repeated pair']][3] >= 0, 'the first entry of the pair is the double bond'
    assert status[at['status carried']] == 2 and status[at['negative count']] == 0
    assert first[at['no atoms']] == first[at['everything dropped']] == [-1] * 33
    assert [p for p, r in enumerate(first[at['one atom']]) if r >= 0] == [6, 7, 18, 26], 'O, *, [!$(CC)] and [H2]'
    assert int(got['n_hits_marked'][at['pocket rows interleaved']]) > 0


def test_without_masks_flags_and_scatter():
    names = [name for name, m in edge_molecules().items() if len(m['symbols']) <= 47 and m['n_bonds'] is None]
    molecules = [dict(edge_molecules()[name], keep=None, marked=None) for name in names]
    patterns = compiled(['c1ccccc1', 'C1=CC=CC=C1', 'cc', 'C=C', 'CC', '[$(cO)]', 'a', 'A'])
    got = check(molecules, 47, patterns, names, scatter=False, with_marks=False, with_drop=False)
    plain = [dict(m, aromatic=set()) for m in molecules]
    bare = launch(batch_of(plain, 47, scatter=False), patterns, with_drop=False, with_marks=False, with_flags=False)
    assert_equals_reference(bare, reference(plain, 47, patterns, scatter=False, with_marks=False), names)
    b = names.index('benzene')
    assert got['first_root'][b].tolist()[:2] == [0, -1] and bare['first_root'][b].tolist()[:2] == [-1, 0], 'without flags: Kekule'


def test_a_list_cut_short_at_its_capacity():
    molecules = [chain(4), molecule(['C'] * 3, [(0, 1, 1), (1, 2, 1)], n_bonds=1000), named('benzene')]
    patterns = compiled(['CCC', 'CC', 'c'])
    got = check(molecules, 7, patterns, capacity=2)
    assert got['status'].tolist() == [sr.OVERFLOW] * 3 and got['first_root'][0].tolist()[0] >= 0
    got = check(molecules[:2], 7, patterns, capacity=4)
    assert got['status'].tolist() == [0, sr.OVERFLOW | sr.BAD_BOND]


def test_more_list_entries_than_the_neighbour_table_holds():
    """2048 kept entries are searched (here one pair over and over: a repeated pair); 2049 are too large, and then an entry that
    is no bond still sets its bit while repeated pairs are not looked for; entries to dropped atoms do not count."""
    from difflinker_amd import _lib
    full = _lib.DL_SUB_MAX_BONDS
    two = ['C', 'O']
    molecules = [molecule(two, [(0, 1, 2)] + [(1, 0, 1)] * (full - 1)), molecule(two, [(0, 1, 1)] * (full + 1)),
                 molecule(two, [(0, 1, 1)] * (full + 1) + [(0, 2, 1)]), molecule(two, [(0, 1, 1)] * full + [(1, 1, 1), (0, 1, 0)]),
                 molecule(two + ['N'], [(0, 1, 2)] + [(1, 2, 1)] * (full + 9), keep=[True, True, False])]
    names = ['2048 entries', '2049 entries', '2049 and a bad one', '2048 and two bad ones', 'most of them to a dropped atom']
    got = check(molecules, 3, compiled(['C=O', 'CO', '*']), names, capacity=full + 16, scatter=False)
    assert got['status'].tolist() == [sr.BAD_BOND, sr.TOO_LARGE, sr.TOO_LARGE | sr.BAD_BOND, sr.BAD_BOND, 0]
    assert got['first_root'].tolist() == [[0, -1, 0], [-1] * 3, [-1] * 3, [-1, 0, 0], [0, -1, 0]]
    assert got['n_hits'].tolist() == [2, 0, 0, 2, 2]


def test_the_most_sub_patterns_and_levels():
    """256 distinct bodies and four nesting levels in one catalogue: every bit row of the kernel's table is in use."""
    from difflinker_amd import _lib
    nested = '[$([#6][$([#6][$([#6][$([#6][#8])])])])]'
    flat = [f'[$([#{(6, 7, 8, 16)[k % 4]};D{k // 4 % 4}]~[D{k // 16 % 4};!x{k // 64}])]' for k in range(_lib.DL_SUB_MAX_SUBPATTERNS - 6)]
    patterns = compiled([nested] + flat + ['[$(CO),$(CN)]'])
    assert patterns.n_sub == _lib.DL_SUB_MAX_SUBPATTERNS and len(patterns.level_end) == _lib.DL_SUB_MAX_LEVELS
    molecules = [molecule(*sc.parse(text)) for text in ('CCCCO', 'CCCO', 'OCCCCN', 'C1CC1C(=O)N', 'CSC(C)(C)N', 'CC(C)(C)CCCCO')]
    molecules += [named('rhodanine'), named('phenol'), chain(256)]
    got = check(molecules, 256, patterns, scatter=False)
    assert got['first_root'][0, 0].item() == 0 and int(got['n_hits'][0]) > 10 and int(got['status'].abs().sum()) == 0


def test_marks_where_the_last_map_alone_touches_the_linker():
    """Neopentane-like stars: ``C(C)(C)C`` from the centre has 24 maps of the three branches onto the four leaves, in
    lexicographic order; with the leaf of highest index alone marked the first map that touches it comes late, and with
    ``CC`` from the centre the LAST map of the root is the only one that does."""
    star = molecule(['C'] * 5, [(0, k, 1) for k in range(1, 5)], marked=[k == 4 for k in range(5)])
    patterns = compiled(['CC', 'C(C)(C)C', 'C(C)(C)(C)(C)C', 'CCC'])
    got = check([star, dict(star, marked=[False] * 5), dict(star, marked=[k == 0 for k in range(5)])], 5, patterns, scatter=False)
    assert got['first_root'].tolist() == [[0, 0, -1, 1]] * 3
    assert got['first_root_marked'].tolist() == [[0, 0, -1, 1], [-1] * 4, [0, 0, -1, 1]]
    mol = sr.Molecule([6] * 5, [4] * 5, star['entries'], marked=star['marked'])
    assert sr.Matcher(patterns).search(mol, [], 0, 0, True, 4096)[3] == 5, 'the root and all four leaves: the marked one is tested last'


@pytest.mark.parametrize('smarts,marks,needed', [('CC', False, 2), ('CC', True, 4), ('C1CCC1', True, None)])
def test_the_budget_on_cubane(smarts, marks, needed):
    """With ``max_steps`` equal to the steps the most expensive root needs no bit is set; with one step fewer it is, and what
    was found before stands (``tests/test_substructure_host.py`` derives the 2 and the 4 by hand)."""
    patterns = compiled([smarts])
    cubane = named('cubane', marked=[False] * 8 if marks else None)
    others = [named('benzene'), named('cyclopropane')]
    if needed is None:
        mol = sr.Molecule([6] * 8, [4] * 8, cubane['entries'], marked=cubane['marked'])
        needed = max(sr.Matcher(patterns).search(mol, [], 0, root, True, 1 << 20)[3] for root in range(8))
    exact = check([cubane] + others, 12, patterns, max_steps=needed, with_marks=marks)
    short = check([cubane] + others, 12, patterns, max_steps=needed - 1, with_marks=marks)
    assert int(exact['status'][0]) == 0 and int(short['status'][0]) == sr.BUDGET
    assert int(exact['first_root'][0, 0]) >= 0 and (int(short['first_root'][0, 0]) >= 0) == marks


def test_a_sub_pattern_out_of_budget():
    patterns = compiled(['[$(C1CCC1)]', 'C'])
    got = check([named('cubane'), named('cyclopropane')], 8, patterns, max_steps=3)
    assert got['first_root'][0].tolist()[0] == -1 and int(got['status'][0]) == sr.BUDGET and int(got['n_hits'][0]) == 1


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_batch():
    names = ('phenol', 'cubane', 'rhodanine', 'biphenyl', 'two_pieces')
    molecules = [named(name, marked=[k % 3 == 0 for k in range(len(sc.MOLECULES[name][0]))]) for name in names]
    molecules += [edge_molecules()['pocket rows interleaved'], edge_molecules()['status carried'], edge_molecules()['repeated pair']]
    patterns = compiled(['c[OH]', 'C1CCC1', 'S=C', 'c-c', '[$(c:[$(c[OH])])]', 'CN', 'C=C', '[!R]', 'CO'])
    return molecules, patterns, batch_of(molecules, 16)


@pytest.mark.parametrize('form', ['strided', 'sliced', 'wide'])
def test_input_forms(form):
    """Strided, sliced and float64 / int64 / bool inputs, the ``Bonds`` members and the aromatic flags included, give the
    canonical run's bits, and nothing is written to an input or around it."""
    import input_forms as F
    molecules, patterns, batch = small_batch()
    want = reference(molecules, 16, patterns)
    keep = []

    def place(t):
        out = F.BY_NAME[form](t, DEV)
        keep.append((F.buffer_of(out), F.as_bytes(F.buffer_of(out)).clone()))
        return out
    got = launch(batch, patterns, place=place)
    torch.cuda.synchronize()
    assert_equals_reference(got, want)
    assert len(keep) == 11
    for buf, copy in keep:
        assert torch.equal(F.as_bytes(buf), copy)
    one_hot, mask, drop, mark, found, flags = batch
    B = len(molecules)
    squeezed = launch((one_hot, mask.reshape(B, 16, 1), drop.reshape(B, 16, 1), mark.reshape(B, 16, 1), found, flags), patterns)
    assert_equals_reference(squeezed, want)


def test_stale_output_memory(monkeypatch):
    """Every output element is written whatever the buffers held before (the harness of ``test_gpu_scratch.py``)."""
    import test_gpu_scratch as SC
    molecules, patterns, _ = small_batch()
    more = molecules + [chain(17), chain(300)]                               # one that fills every row, one that is too large
    batch = batch_of(more, 300)

    def run():
        got = launch(batch, patterns)
        torch.cuda.synchronize()
        return SC.Ran(got, [(name, got[name], got[name].element_size() * got[name].numel()) for name in FIELDS])
    got = SC.check_contract(monkeypatch, run)
    assert_equals_reference(got, reference(more, 300, patterns))


def test_arguments_are_checked_before_the_launch():
    from difflinker_amd._lib import HipLibraryError
    from difflinker_amd.metrics import match_patterns
    molecules, patterns, batch = small_batch()
    one_hot, mask, drop, mark, found, flags = batch
    place = lambda t: t.to(DEV)                                              # noqa: E731
    x = torch.zeros(len(molecules), 16, 3, device=DEV)
    with pytest.raises(ValueError, match='max_steps'):
        launch(batch, patterns, max_steps=0)
    with pytest.raises(ValueError, match='shapes disagree'):
        match_patterns(place(one_hot), x, place(mask[:, :5]), on_device(found, place), place(flags), patterns, True)
    with pytest.raises(ValueError, match='shapes disagree'):
        match_patterns(place(one_hot), x, place(mask), on_device(found, place), place(flags[:, :1]), patterns, True)
    with pytest.raises(HipLibraryError):
        match_patterns(one_hot, x.cpu(), mask, found, flags, patterns, True)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def placed(symbols, xy):
    return list(symbols), [(x, y, 0.0) for x, y in xy]


def polar(origin, length, degrees):
    return origin[0] + length * math.cos(math.radians(degrees)), origin[1] + length * math.sin(math.radians(degrees))


# flat drawings at the table's own bond lengths: acetyl chloride, ethanethiol, ethanol, dimethyl disulfide
DRAWN = {
    'acetyl_chloride': placed(['C', 'C', 'O', 'Cl'], [(-1.54, 0), (0, 0), polar((0, 0), 1.20, 60), polar((0, 0), 1.77, -60)]),
    'ethanethiol': placed(['C', 'C', 'S'], [(0, 0), (1.54, 0), polar((1.54, 0), 1.82, 70)]),
    'ethanol': placed(['C', 'C', 'O'], [(0, 0), (1.54, 0), polar((1.54, 0), 1.43, 70)]),
    'dimethyl_disulfide': placed(['C', 'S', 'S', 'C'], [(0, 0), (1.82, 0), polar((1.82, 0), 2.04, 70),
                                                       polar(polar((1.82, 0), 2.04, 70), 1.82, 0)]),
}


def test_analyze_patterns_to_scores():
    from difflinker_amd import const
    from difflinker_amd.metrics import analyze_patterns, compute_filters, patterns_to_host
    from difflinker_amd.patterns import load_catalogue
    catalogue = load_catalogue('basic')
    B, N = len(DRAWN), 5
    one_hot, x, mask, linker = torch.zeros(B, N, const.GEOM_NUMBER_OF_ATOM_TYPES), torch.zeros(B, N, 3), torch.zeros(B, N, 1), torch.zeros(B, N, 1)
    for b, (symbols, xyz) in enumerate(DRAWN.values()):
        for k, s in enumerate(symbols):
            one_hot[b, k, const.GEOM_ATOM2IDX[s]] = 1
            x[b, k] = torch.tensor(xyz[k])
            mask[b, k] = 1
        linker[b, 0] = 1                                                     # the first carbon alone is the linker
    result = analyze_patterns(one_hot.to(DEV), x.to(DEV), mask.to(DEV), True, linker.to(DEV), catalogue)
    records = patterns_to_host(result, catalogue.names)
    assert [r.hits for r in records] == [['acyl_halide'], ['thiol'], [], ['disulfide']]
    assert [r.linker_hits for r in records] == [[], [], [], []], 'the methyl carbon is in none of the groups'
    assert [r.status for r in records] == [0] * 4
    assert compute_filters(records) == {'filters_passed': 0.25, 'filters_passed_linker': 1.0, 'filter_hits_per_molecule': 0.75,
                                        'filters_budget': 0.0}
    linker[:, 0], linker[:, 1] = 0, 1                                        # the second atom: the acyl carbon, the CH2, the sulfur
    result = analyze_patterns(one_hot.to(DEV), x.to(DEV), mask.to(DEV), True, linker.to(DEV), catalogue)
    records = patterns_to_host(result, catalogue.names)
    assert [r.linker_hits for r in records] == [['acyl_halide'], [], [], ['disulfide']]
    assert compute_filters(records[:2], records[2:])['true_filters_passed'] == 0.5


def test_generate_writes_the_filters_and_changes_no_file(tmp_path):
    """``generate --filters basic`` on a tiny synthetic run, as ``test_gpu_select.run_twice`` drives it: ``filters.json`` with
    one record per written file, the four keys in ``metrics.json``, every other file byte for byte what it was."""
    import test_gpu_select as SEL
    from difflinker_amd.generate import generate
    from difflinker_amd.metrics import FILTER_NAMES
    ddpm = SEL.synthetic_ddpm()
    from test_gpu_generate import IO_DIR
    frag = os.path.join(IO_DIR, 'frag.sdf')
    runs = {}
    for tag, flags in (('plain', {'metrics': True}), ('filters', {'metrics': True, 'filters': 'basic'}), ('bare', {'filters': 'basic'})):
        torch.manual_seed(11)
        runs[tag] = generate(frag, ddpm, str(tmp_path / tag), n_samples=3, n_steps=5, linker_size='4', output_format='both', **flags)
    names = [os.path.basename(path) for path in runs['plain']]
    assert len(names) == 6 and all([os.path.basename(path) for path in runs[tag]] == names for tag in runs)
    assert set(os.listdir(tmp_path / 'filters')) - set(os.listdir(tmp_path / 'plain')) == {'filters.json'}
    assert set(os.listdir(tmp_path / 'plain')) - set(os.listdir(tmp_path / 'bare')) == {'metrics.json'}
    for name in sorted(os.listdir(tmp_path / 'plain')):
        if name != 'metrics.json':
            for tag in ('filters', 'bare'):
                assert filecmp.cmp(tmp_path / 'plain' / name, tmp_path / tag / name, shallow=False), (tag, name)
    assert filecmp.cmp(tmp_path / 'filters' / 'filters.json', tmp_path / 'bare' / 'filters.json', shallow=False)
    records = json.load(open(tmp_path / 'filters' / 'filters.json'))
    assert [r['file'] for r in records] == names and all(set(r) == {'file', 'hits', 'linker_hits', 'status'} for r in records)
    scores, plain = json.load(open(tmp_path / 'filters' / 'metrics.json')), json.load(open(tmp_path / 'plain' / 'metrics.json'))
    assert {k: v for k, v in scores.items() if k not in FILTER_NAMES} == plain and set(FILTER_NAMES) <= set(scores)
    assert scores['filters_budget'] == 0.0 and 0.0 <= scores['filters_passed'] <= scores['filters_passed_linker'] <= 1.0


def test_sample_writes_the_filters_and_changes_no_file(tmp_path):
    """``sample --filters basic`` as ``test_gpu_canon.test_sample_writes_the_strings_and_changes_no_file`` drives ``--smiles``:
    ``filters.json`` with one record per written sample file, the four keys and their ``true_`` values in ``metrics.json``,
    every other file byte for byte what it was."""
    import test_gpu_rings as RG
    from difflinker_amd.metrics import FILTER_NAMES
    from difflinker_amd.sample import sample
    m = RG.gentle_model(tmp_path, False)
    outs = {}
    for tag, flags in (('plain', {'metrics': True}), ('filters', {'metrics': True, 'filters': 'basic'})):
        m.edm.noise_seed = 5
        outs[tag] = sample(m, str(tmp_path / tag), 'zinc_final_test', 2, str(DEV), data=str(tmp_path), n_steps=5,
                           output_format='sdf', **flags)
    plain, out = outs['plain'], outs['filters']
    names = sorted(os.path.join(u, name) for u in os.listdir(out) if os.path.isdir(os.path.join(out, u))
                   for name in os.listdir(os.path.join(out, u)))
    for name in names:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain))) == ['filters.json']
    records = json.load(open(os.path.join(out, 'filters.json')))
    sampled = [name for name in names if name.endswith('_.sdf')]
    assert sorted(r['file'] for r in records) == sampled and len(sampled) == 10, 'one record per written file'
    assert all(set(r) == {'file', 'hits', 'linker_hits', 'status'} and set(r['linker_hits']) <= set(r['hits']) for r in records)
    scores, plain_scores = json.load(open(os.path.join(out, 'metrics.json'))), json.load(open(os.path.join(plain, 'metrics.json')))
    added = set(FILTER_NAMES) | {f'true_{k}' for k in FILTER_NAMES}
    assert {k: v for k, v in scores.items() if k not in added} == plain_scores and added <= set(scores)
    passed = sum(1 for r in records if not r['hits'] and not r['status'] & 516) / len(records)
    assert scores['filters_passed'] == passed and scores['filters_budget'] == 0.0
    assert scores['filter_hits_per_molecule'] == sum(len(r['hits']) for r in records) / len(records)
    assert 0.0 <= scores['true_filters_passed'] <= scores['true_filters_passed_linker'] <= 1.0
