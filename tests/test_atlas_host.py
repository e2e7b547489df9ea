"""The Python restatements of the bond-graph rules (``canon_ref``, ``mol_keys_ref``, ``rings_ref``, ``fragment_ref``,
``substructure_ref``) and ``metrics.isomorphisms`` against ``networkx`` on every graph of up to 7 atoms, seeded colourings of the
small ones and vertex-transitive cage graphs (``atlas_cases.py``).  The restatements and the kernels were written from one
paragraph of ``include/difflinker_hip.h`` each; the oracles here share nothing with either, so a mistake both have in common -
two graphs under one canonical code, an orbit split by a class, a ring size off by one, a root the search never reaches -
shows here, on the CPU, and ``test_gpu_atlas.py`` then holds the kernels to the same answers.

The whole file takes about two minutes.  The substructure sweep is the longest part: all 1252 molecules (disconnected ones
included) against the 31 patterns, with every odd-numbered atom marked; the marked oracle asks VF2 once per candidate root and
stops at the first map that touches a mark, which keeps the 7-atom molecules affordable, so nothing is restricted to 6."""
import functools
import itertools
import random

import atlas_cases as ac
import canon_ref as cr
import fragment_ref
import mol_keys_ref as kr
import rings_ref
import substructure_ref as sr

MAX_LEAVES = 65536


# ---- the families -------------------------------------------------------------------------------------------------------------------
def test_the_families_hold_what_the_random_graphs_of_the_other_tests_lack():
    atlas = ac.atlas()
    assert len(ac.high_degree()) == 568 and ac.high_degree()[-1] == 1251, 'atoms of degree 5 and 6'
    assert len(atlas[1251][0]) == 7 and len(atlas[1251][1]) == 21, 'K7 is the last atlas graph'
    assert sum(1 for m in atlas if ac.n_components(*m) > 1) == 1252 - 996, 'the disconnected graphs'
    assert len(ac.ballast()) == 208
    for types, bonds, where in ac.ballast():
        assert len(types) == len(where) + ac.BALLAST_PATH <= 72 and len(bonds) >= ac.BALLAST_PATH - 1
        assert len(where) < 2 or min(where) < ac.WORD <= max(where), 'an atom on either side of kept index 63 | 64'
    assert len(ac.named()) == 13 and max(len(t) for t, _ in ac.named().values()) == 20


# ---- canonical ranks ----------------------------------------------------------------------------------------------------------------
def canon(types, bonds, max_leaves=MAX_LEAVES):
    got = cr.canonical_ranks(types, bonds, max_leaves=max_leaves)
    assert sorted(got['rank']) == list(range(len(types))), 'the ranks are a permutation'
    return got, cr.form(types, bonds, got['rank'])


@functools.lru_cache(maxsize=None)
def atlas_runs():
    """Per atlas graph the results of the graph as given and of two renumbered copies: ``[(result, form)] * 3``."""
    rng = random.Random(5)
    return [[canon(*m) for m in (molecule, ac.renumber(*molecule, rng), ac.renumber(*molecule, rng))] for molecule in ac.atlas()]


@functools.lru_cache(maxsize=None)
def atlas_automorphisms():
    return [ac.automorphisms(*m) for m in ac.atlas()]


def test_one_code_per_atlas_graph_whatever_the_numbering():
    codes = set()
    for k, runs in enumerate(atlas_runs()):
        assert all(got['status'] == 0 for got, _ in runs), k
        assert len({got['code'] for got, _ in runs}) == 1 and len({form for _, form in runs}) == 1, k
        assert len({got['n_leaves'] for got, _ in runs}) == 1, k
        codes.add(runs[0][0]['code'])
    assert len(codes) == 1252, 'equal codes only for the same graph'
    assert max(runs[0][0]['n_leaves'] for runs in atlas_runs()) == atlas_runs()[-1][0][0]['n_leaves'] == 5040, 'K7: 7! leaves'


def test_coloured_graphs_share_a_code_exactly_when_networkx_calls_them_isomorphic():
    items = ac.coloured()
    classes = ac.isomorphism_classes([(t, b) for t, b, _ in items])
    members = {}
    for c in classes:
        members[c] = members.get(c, 0) + 1
    assert 5 * sum(1 for c in classes if members[c] > 1) >= len(items), 'a fifth of the items share their class with another'
    rng = random.Random(6)
    code_of_class, class_of_code = {}, {}
    for (types, bonds, _), c in zip(items, classes):
        for molecule in ((types, bonds), ac.renumber(types, bonds, rng)):
            got, _ = canon(*molecule)
            assert got['status'] == 0
            assert code_of_class.setdefault(c, got['code']) == got['code'], 'one class, two codes'
            assert class_of_code.setdefault(got['code'], c) == c, 'one code, two classes'
    assert len(code_of_class) == len(class_of_code) == len(members)


def test_named_graphs_take_one_leaf_per_automorphism():
    codes = {}
    for name, (types, bonds) in ac.named().items():
        got, _ = canon(types, bonds)
        count, orbits = ac.automorphisms(types, bonds)
        assert got['status'] == 0 and got['n_leaves'] == count == ac.AUTOMORPHISMS[name], name
        assert len(orbits) == 1, 'vertex-transitive'
        codes[name] = got['code']
    assert len(set(codes.values())) == len(codes)
    rook, shrikhande = ac.named()['rook'], ac.named()['shrikhande']
    assert codes['rook'] != codes['shrikhande'], 'strongly regular with the same parameters, and not the same graph'
    assert kr.colours_and_key(*rook)[1] == kr.colours_and_key(*shrikhande)[1], '1-WL cannot tell them apart'


def test_leaves_are_a_multiple_of_the_automorphisms_without_twin_cells():
    twins = 0
    for k in ac.small(6):
        if ac.has_twin_cell(*ac.atlas()[k]):
            twins += 1
            continue
        assert atlas_runs()[k][0][0]['n_leaves'] % atlas_automorphisms()[k][0] == 0, k
    assert twins == 29 and len(ac.small(6)) - twins == 179


# ---- keys, classes and orbits ---------------------------------------------------------------------------------------------------------
def test_keys_and_colours_are_exactly_1_wl():
    colours, classes = ac.exact_wl(ac.atlas())
    results = [kr.colours_and_key(*m) for m in ac.atlas()]
    assert ac.partition([r[1] for r in results]) == ac.partition(classes) and len(set(classes)) == 1226
    for k, (r, exact) in enumerate(zip(results, colours)):
        assert ac.partition(r[0]) == ac.partition(exact), k


def test_a_class_never_separates_two_atoms_of_one_orbit():
    coarser = 0
    for k, molecule in enumerate(ac.atlas()):
        classes = cr._Graph(*molecule).root()
        orbits = atlas_automorphisms()[k][1]
        assert all(len({classes[i] for i in orbit}) == 1 for orbit in orbits), k
        assert ac.partition(classes) == ac.partition(kr.colours_and_key(*molecule)[0]), 'the classes are the colour classes'
        coarser += len(set(classes)) < len(orbits)
    assert coarser == 2, 'two graphs of 1252 whose classes are coarser than their orbits: permitted, and rare'
    for name, molecule in ac.named().items():
        assert len(set(cr._Graph(*molecule).root())) == 1, name


# ---- rings ------------------------------------------------------------------------------------------------------------------------------
def test_rings_of_every_atlas_graph():
    for k, (types, bonds) in enumerate(ac.atlas()):
        n = len(types)
        got = rings_ref.molecule([1.0] * n, bonds, len(bonds))
        assert (got['n_atoms'], got['n_bonds'], got['status']) == (n, len(bonds), 0), k
        assert got['n_components'] == ac.n_components(types, bonds) and got['n_rings'] == ac.cyclomatic(types, bonds), k
        assert got['bond_ring'] == ac.bond_rings(types, bonds) and got['atom_ring'] == ac.atom_rings(types, bonds), k


# ---- double cuts ----------------------------------------------------------------------------------------------------------------------
LOOSE = {'min_linker': 1, 'min_fragment': 1, 'min_path_atoms': 1, 'linker_leq_frags': 0}
R = 16                                           # a tree of 7 atoms has 6 bridges: 15 pairs


def check_cuts(types, bonds, got, labels_of, what):
    """``got``: the outputs of one molecule with ``cuts`` as rows of 10 and ``labels_of(r)`` the labels of record ``r`` by atom
    number; shared with ``test_gpu_atlas.py``."""
    n = len(types)
    bridges = ac.bridges(types, bonds)
    entries = [e for e, (i, j, _) in enumerate(bonds) if frozenset((i, j)) in bridges]
    assert got['n_atoms'] == n and got['n_bonds'] == len(bonds) and got['n_cuttable'] == len(bridges), what
    for e, (i, j, _) in enumerate(bonds):
        assert got['bond_side'][e] == (len(ac.side_of(types, bonds, i, j)) if e in entries else 0), (what, e)
    if ac.n_components(types, bonds) > 1:
        assert got['status'] == fragment_ref.DISCONNECTED and got['n_cuts'] == 0, what
        return
    pairs = list(itertools.combinations(entries, 2))
    assert got['status'] == 0 and got['n_cuts'] == len(pairs) <= R, what
    for r, (e1, e2) in enumerate(pairs):                                    # in lexicographic order of the list positions
        record = [int(v) for v in got['cuts'][r]]
        assert record[:2] == [e1, e2], (what, r)
        labels = labels_of(r)
        parts = {frozenset(k for k in range(n) if labels[k] == part) for part in (0, 1, 2)}
        assert parts == ac.three_parts(types, bonds, bonds[e1][:2], bonds[e2][:2]), (what, r)
        assert record[6:9] == [sum(1 for k in range(n) if labels[k] == part) for part in (0, 1, 2)], (what, r)


def test_double_cuts_of_every_atlas_graph():
    for k, (types, bonds) in enumerate(ac.atlas()):
        n = len(types)
        got = fragment_ref.molecule([1.0] * n, [[1.0, 0.0, 0.0]] * n, bonds, len(bonds), R, **LOOSE)
        check_cuts(types, bonds, got, lambda r: got['labels'][r], k)


# ---- substructure search --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compiled_patterns():
    from difflinker_amd.patterns import compile_patterns
    return compile_patterns([(text, f'atlas {k}') for k, text in ac.patterns()])


@functools.lru_cache(maxsize=None)
def atlas_roots():
    """Per atlas molecule and pattern the oracle's ``(roots, roots_marked)`` with the odd-numbered atoms marked."""
    return [[ac.roots(m, ac.atlas()[k], ac.odd_atoms(m[0])) for k, _ in ac.patterns()] for m in ac.atlas()]


def test_substructure_roots_of_every_pattern_in_every_atlas_graph():
    matcher = sr.Matcher(compiled_patterns())
    most = 0
    for b, (types, bonds) in enumerate(ac.atlas()):
        n = len(types)
        marked = [k % 2 == 1 for k in range(n)]
        mol = sr.Molecule([6] * n, [4] * n, bonds, marked=marked)
        got = matcher.match(mol, max_steps=ac.SUB_MAX_STEPS, with_marks=True)
        plain = matcher.match(mol, max_steps=ac.SUB_MAX_STEPS, with_marks=False) if n <= 6 else None
        assert got['status'] == 0, (b, 'no budget bit, nothing else')
        most = max([most] + list(got['steps'].values()))
        for p, (roots, roots_marked) in enumerate(atlas_roots()[b]):
            assert got['roots'][p] == roots and got['first_root'][p] == min(roots, default=-1), (b, p)
            assert got['roots_marked'][p] == roots_marked and got['first_root_marked'][p] == min(roots_marked, default=-1), (b, p)
            if plain is not None:                                           # the search that stops at its first map
                assert plain['roots'][p] == roots and plain['first_root'][p] == got['first_root'][p], (b, p)
                assert plain['status'] == 0 and not plain['roots_marked'][p] and plain['first_root_marked'][p] == -1, (b, p)
    assert ac.SUB_MAX_STEPS // 2 < most <= ac.SUB_MAX_STEPS, f'the longest search takes {most} steps'


# ---- the map enumerator of the RMSD score -----------------------------------------------------------------------------------------------
def test_isomorphisms_onto_itself_are_the_automorphisms():
    from difflinker_amd.metrics import Graph, isomorphisms
    for k in ac.small(6):
        types, bonds = ac.atlas()[k]
        maps, truncated = isomorphisms(Graph(types, bonds, None), Graph(types, bonds, None))
        assert len(maps) == atlas_automorphisms()[k][0] and not truncated, k
        assert len({tuple(m) for m in maps}) == len(maps), k
