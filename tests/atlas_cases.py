"""Inputs and oracles of the atlas sweep (``test_atlas_host.py``, ``test_gpu_atlas.py``): every graph of up to 7 atoms, seeded
colourings of the small ones, vertex-transitive and cage graphs, and the small graphs next to a long nitrogen path - each with
answers that come from ``networkx`` alone (the graph atlas it ships, VF2, bridges, cycle bases, shortest paths).  Nothing here
imports the package, torch or a ``*_ref.py`` restatement, so what the oracles say shares no code and no author with the rules
of ``include/difflinker_hip.h``.

A molecule is ``(types, bonds)`` in the project's form: element indices of ``const.ATOM2IDX`` and ``(i, j, order)``."""
import functools
import itertools
import random

import networkx as nx
from networkx.algorithms.isomorphism import GraphMatcher
from networkx.generators.atlas import graph_atlas_g

from canon_cases import C, N, renumber  # noqa: F401  (renumber is part of what this module offers)

BALLAST_PATH = 64                                # nitrogen atoms next to each small graph (see ``ballast``)
WORD = 64                                        # kept atoms per word of the 256 x 256 bit matrix


# ---- the four families --------------------------------------------------------------------------------------------------------------
def _plain(g):
    """A networkx graph whose nodes are 0..n-1 as an all-carbon, all-single molecule."""
    assert sorted(g.nodes) == list(range(g.number_of_nodes()))
    return [C] * g.number_of_nodes(), [(min(i, j), max(i, j), 1) for i, j in sorted(tuple(sorted(e)) for e in g.edges)]


@functools.lru_cache(maxsize=None)
def atlas():
    """The 1252 atlas graphs of 1..7 nodes in atlas order."""
    out = [_plain(g) for g in graph_atlas_g()[1:]]
    assert len(out) == 1252 and sum(1 for t, _ in out if len(t) <= 6) == 208
    return out


def small(most=6, least=1):
    """Positions in ``atlas()`` of the graphs of ``least..most`` nodes."""
    return [k for k, (t, _) in enumerate(atlas()) if least <= len(t) <= most]


COLOURINGS = 6                                   # per graph
ATOM_PALETTE = (C, C, C, C, C, N)                # a sixth of the atoms nitrogen, an eighth of the bonds double: about one of each
ORDER_PALETTE = (1, 1, 1, 1, 1, 1, 1, 2)         # in a 6-node graph, so that colourings of one graph often coincide


@functools.lru_cache(maxsize=None)
def coloured():
    """``COLOURINGS`` seeded colourings of every atlas graph of 2..6 nodes: ``[(types, bonds, atlas position)]``."""
    out = []
    for k in small(6, 2):
        types, bonds = atlas()[k]
        for c in range(COLOURINGS):
            rng = random.Random(1000 * k + c)
            out.append(([rng.choice(ATOM_PALETTE) for _ in types], [(i, j, rng.choice(ORDER_PALETTE)) for i, j, _ in bonds], k))
    return out


def _integers(g):
    return nx.convert_node_labels_to_integers(g, ordering='sorted')


def shrikhande():
    g = nx.Graph()
    for a, b in itertools.product(range(4), repeat=2):
        for da, db in ((1, 0), (0, 1), (1, 1)):
            g.add_edge((a, b), ((a + da) % 4, (b + db) % 4))
    return g


# name -> (graph, |Aut| as the issue lists it)
_NAMED = {
    'petersen': (nx.petersen_graph, 120), 'dodecahedral': (nx.dodecahedral_graph, 120), 'cubical': (nx.cubical_graph, 48),
    'prismane': (lambda: nx.circular_ladder_graph(3), 12), 'hypercube4': (lambda: nx.hypercube_graph(4), 384),
    'rook': (lambda: nx.cartesian_product(nx.complete_graph(4), nx.complete_graph(4)), 1152), 'shrikhande': (shrikhande, 192),
    'truncated_tetrahedron': (nx.truncated_tetrahedron_graph, 24), 'moebius_kantor': (nx.moebius_kantor_graph, 96),
    'desargues': (nx.desargues_graph, 240), 'k33': (lambda: nx.complete_bipartite_graph(3, 3), 72),
    'icosahedral': (nx.icosahedral_graph, 120), 'octahedral': (nx.octahedral_graph, 48),
}
AUTOMORPHISMS = {name: count for name, (_, count) in _NAMED.items()}


@functools.lru_cache(maxsize=None)
def named():
    """name -> (types, bonds): vertex-transitive and cage graphs, all carbon and single."""
    return {name: _plain(_integers(make())) for name, (make, _) in _NAMED.items()}


@functools.lru_cache(maxsize=None)
def ballast():
    """Every atlas graph of 1..6 nodes united with a path of ``BALLAST_PATH`` nitrogen atoms, the atom numbers shuffled (seeded)
    until the small graph has an atom on either side of kept index 63 | 64: ``[(types, bonds, where)]``, ``where[k]`` the number
    of atom ``k`` of the small graph.  The path has 64 atoms, not 60: with 60 a graph of fewer than 5 atoms ends before index 64
    and cannot lie across the word boundary."""
    out = []
    for k in small(6):
        types, bonds = atlas()[k]
        n = len(types)
        rng = random.Random(k)
        while True:
            new = list(range(n + BALLAST_PATH))
            rng.shuffle(new)
            if n < 2 or (min(new[:n]) < WORD <= max(new[:n])):
                break
        all_types = [None] * (n + BALLAST_PATH)
        for old, t in enumerate(types + [N] * BALLAST_PATH):
            all_types[new[old]] = t
        rows = bonds + [(n + p, n + p + 1, 1) for p in range(BALLAST_PATH - 1)]
        rows = [(new[i], new[j], o) if rng.random() < 0.5 else (new[j], new[i], o) for i, j, o in rows]
        rng.shuffle(rows)
        out.append((all_types, rows, new[:n]))
    return out


HIGH_DEGREE = 5                                  # the molecule-like random graphs of the other tests stop at degree 4


@functools.lru_cache(maxsize=None)
def high_degree():
    """Positions in ``atlas()`` of the graphs with an atom of degree 5 or 6 (K7 is the last atlas graph); none of the seeded
    random graphs of the other tests has one."""
    return [k for k, (types, bonds) in enumerate(atlas()) if max(degrees(types, bonds), default=0) >= HIGH_DEGREE]


def degrees(types, bonds):
    d = [0] * len(types)
    for i, j, _ in bonds:
        d[i] += 1
        d[j] += 1
    return d


def has_twin_cell(types, bonds):
    """Two atoms of degree 1 on one neighbour: the only symmetry the search of ``dl_canonical_ranks`` does not enumerate."""
    d = degrees(types, bonds)
    leaves_on = [0] * len(types)
    for i, j, _ in bonds:
        leaves_on[j] += d[i] == 1
        leaves_on[i] += d[j] == 1
    return max(leaves_on, default=0) >= 2


# ---- SMARTS ---------------------------------------------------------------------------------------------------------------------------
def smarts(types, bonds):
    """A connected all-carbon graph as a SMARTS string by a depth-first search from node 0: atom ``C``, explicit ``-`` bonds,
    ring-closure digits (the opening end carries the bond), branches in parentheses.  Pattern atom 0 is node 0."""
    n = len(types)
    nbrs = [[] for _ in range(n)]
    for i, j, _ in bonds:
        nbrs[i].append(j)
        nbrs[j].append(i)
    parent, order = {0: None}, []

    def visit(u):
        order.append(u)
        for w in sorted(nbrs[u]):
            if w not in parent:
                parent[w] = u
                visit(w)
    visit(0)
    assert len(order) == n, 'a pattern is connected'
    position = {u: k for k, u in enumerate(order)}
    digit = {}
    for i, j, _ in bonds:
        if parent[i] != j and parent[j] != i:
            digit[frozenset((i, j))] = len(digit) + 1
    assert len(digit) <= 9

    def write(u):
        text = 'C'
        for w in sorted(nbrs[u], key=position.get):
            d = digit.get(frozenset((u, w)))
            if d is not None:
                text += f'-{d}' if position[u] < position[w] else f'{d}'
        children = [w for w in sorted(nbrs[u]) if parent[w] == u]
        for k, w in enumerate(children):
            piece = '-' + write(w)
            text += piece if k == len(children) - 1 else f'({piece})'
        return text
    return write(0)


# The step budget of the substructure sweeps: the smallest power of two that the longest search of test_atlas_host.py (397
# steps, in a 7-atom molecule with its odd atoms marked) stays within.  A molecule of 6 atoms stays within it whatever its
# marks: from one root a 5-atom pattern takes at most 1 + 5 + 5*5 + 20*5 + 60*5 = 431 steps.
SUB_MAX_STEPS = 512


@functools.lru_cache(maxsize=None)
def patterns():
    """The 31 connected atlas graphs of 1..5 nodes: ``[(atlas position, SMARTS)]``."""
    out = [(k, smarts(*atlas()[k])) for k in small(5) if n_components(*atlas()[k]) == 1]
    assert len(out) == 31
    return out


# ---- oracles: networkx only ---------------------------------------------------------------------------------------------------------
def graph(types, bonds):
    g = nx.Graph()
    g.add_nodes_from((k, {'t': t}) for k, t in enumerate(types))
    g.add_edges_from((i, j, {'o': o}) for i, j, o in bonds)
    assert g.number_of_edges() == len(bonds)
    return g


_SAME_TYPE = lambda a, b: a['t'] == b['t']       # noqa: E731
_SAME_ORDER = lambda a, b: a['o'] == b['o']      # noqa: E731


def n_components(types, bonds):
    return nx.number_connected_components(graph(types, bonds))


def cyclomatic(types, bonds):
    return len(nx.cycle_basis(graph(types, bonds)))


def bond_rings(types, bonds):
    """Per bond, in list order: 1 + the shortest path between its ends with the bond removed; 0 for a bridge."""
    g = graph(types, bonds)
    out = []
    for i, j, _ in bonds:
        data = g.edges[i, j]
        g.remove_edge(i, j)
        out.append(1 + nx.shortest_path_length(g, i, j) if nx.has_path(g, i, j) else 0)
        g.add_edge(i, j, **data)
    return out


def atom_rings(types, bonds):
    """Per atom the smallest non-zero ``bond_rings`` value over its bonds, 0 when it has none."""
    out = [0] * len(types)
    for (i, j, _), ring in zip(bonds, bond_rings(types, bonds)):
        for k in (i, j):
            if ring and (out[k] == 0 or ring < out[k]):
                out[k] = ring
    return out


def bridges(types, bonds):
    """The bridges as a set of frozensets."""
    return {frozenset(e) for e in nx.bridges(graph(types, bonds))}


def side_of(types, bonds, i, j):
    """The atoms on the side of ``i`` once the bridge ``i - j`` is removed."""
    g = graph(types, bonds)
    g.remove_edge(i, j)
    return nx.node_connected_component(g, i)


def three_parts(types, bonds, first, second):
    """The components left after the two bridges ``first`` and ``second`` (pairs of atoms) are removed, as a set of frozensets."""
    g = graph(types, bonds)
    g.remove_edge(*first)
    g.remove_edge(*second)
    return {frozenset(part) for part in nx.connected_components(g)}


def automorphisms(types, bonds):
    """``(|Aut|, orbits)``: the number of type- and order-preserving automorphisms and the orbits they give as a list of sets."""
    g = graph(types, bonds)
    count, orbit = 0, {k: {k} for k in g.nodes}
    for m in GraphMatcher(g, g, node_match=_SAME_TYPE, edge_match=_SAME_ORDER).isomorphisms_iter():
        count += 1
        for a, b in m.items():
            if orbit[a] is not orbit[b]:
                orbit[a] |= orbit[b]
                for c in orbit[b]:
                    orbit[c] = orbit[a]
    return count, list({id(s): s for s in orbit.values()}.values())


def isomorphism_classes(molecules):
    """Class number per molecule (numbered by first appearance) under ``networkx.is_isomorphic`` with types and orders matched,
    bucketed first by the sorted (type, degree, sorted incident orders) sequence."""
    buckets, out, n_classes = {}, [], 0
    for types, bonds in molecules:
        around = [[] for _ in types]
        for i, j, o in bonds:
            around[i].append(o)
            around[j].append(o)
        invariant = tuple(sorted((t, len(a), tuple(sorted(a))) for t, a in zip(types, around)))
        g = graph(types, bonds)
        for other, number in buckets.setdefault(invariant, []):
            if nx.is_isomorphic(g, other, node_match=_SAME_TYPE, edge_match=_SAME_ORDER):
                out.append(number)
                break
        else:
            buckets[invariant].append((g, n_classes))
            out.append(n_classes)
            n_classes += 1
    return out


def roots(molecule, pattern, marked=None):
    """``(roots, roots_marked)``: the atoms of ``molecule`` that are the image of atom 0 of the all-carbon ``pattern`` under some
    subgraph monomorphism, and under one whose image holds an atom of ``marked`` (a set; None: no marks asked for).  Only the
    carbon atoms of the molecule can be images, so VF2 runs on the subgraph they induce; and it runs once per candidate root,
    with that atom and pattern atom 0 pinned to each other by a node attribute, so that the enumeration can stop at the first
    map (or the first that touches a mark) instead of listing the thousands a dense graph has."""
    types, bonds = molecule
    carbon = [k for k, t in enumerate(types) if t == C]
    assert all(t == C for t in pattern[0]) and all(o == 1 for _, _, o in pattern[1])
    assert all(o == 1 for i, j, o in bonds if types[i] == types[j] == C)
    m = graph(types, bonds).subgraph(carbon).copy()
    p = graph(*pattern)
    found, found_marked = set(), set()
    if p.number_of_nodes() > m.number_of_nodes() or p.number_of_edges() > m.number_of_edges():
        return found, found_marked
    nx.set_node_attributes(m, False, 'pin')
    nx.set_node_attributes(p, False, 'pin')
    p.nodes[0]['pin'] = True
    for root in carbon:
        m.nodes[root]['pin'] = True
        for image in GraphMatcher(m, p, node_match=lambda a, b: a['pin'] == b['pin']).subgraph_monomorphisms_iter():
            assert image[root] == 0                                            # molecule atom -> pattern atom
            found.add(root)
            if marked is None:
                break
            if not marked.isdisjoint(image):
                found_marked.add(root)
                break
        m.nodes[root]['pin'] = False
    return found, found_marked


def odd_atoms(types):
    return {k for k in range(len(types)) if k % 2 == 1}


def exact_wl(molecules, rounds=None):
    """1-WL without a hash, over a set of molecules at once: a colour is the position of an atom's signature among the sorted
    distinct signatures of ALL the molecules, which makes colours comparable across them.  The start is the type; a round's
    signature is (own colour, sorted (neighbour's colour, order) pairs); ``max(n, 1)`` rounds for the largest ``n`` unless
    ``rounds`` says otherwise.  Returns ``(colours per molecule, graph class per molecule)``, the class being the sorted
    multiset of final colours, numbered by first appearance."""
    rows = []
    for types, bonds in molecules:
        row = [[] for _ in types]
        for i, j, o in bonds:
            row[i].append((j, o))
            row[j].append((i, o))
        rows.append(row)
    colours = [list(types) for types, _ in molecules]
    rounds = max([len(t) for t, _ in molecules] + [1]) if rounds is None else rounds
    for _ in range(rounds):
        signatures = [[(c[k], tuple(sorted((c[j], o) for j, o in row[k]))) for k in range(len(c))] for c, row in zip(colours, rows)]
        number = {s: at for at, s in enumerate(sorted({s for per in signatures for s in per}))}
        colours = [[number[s] for s in per] for per in signatures]
    classes, out = {}, []
    for c in colours:
        out.append(classes.setdefault(tuple(sorted(c)), len(classes)))
    return colours, out


def partition(labels):
    """The partition of positions by label, as a set of frozensets: what two labellings are compared by."""
    groups = {}
    for at, label in enumerate(labels):
        groups.setdefault(label, set()).add(at)
    return {frozenset(g) for g in groups.values()}
