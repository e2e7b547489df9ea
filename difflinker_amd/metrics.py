"""Scores of sampled molecules without RDKit — the questions of the reference's ``src/metrics.py`` (validity, connectivity,
uniqueness, novelty) and the DeLinker recovery rate of ``src/delinker.py``, asked of the bond graph ``csrc/bonds.hip`` leaves
on the device.

``analyze`` runs bond perception and then ``dl_molecule_keys`` (``csrc/mol_keys.hip``): per molecule the number of atoms over
their valence limit (``const.ALLOWED_BONDS``), the number of pieces, and a 64-bit key from colour refinement that does not
depend on the numbering of the atoms.  Equal keys are necessary for two molecules to be the same graph, not sufficient (1-WL
cannot tell decalin from bicyclopentyl), so ``same_molecule`` settles every key collision exactly on the host.

What these numbers are NOT: RDKit's sanitisation (aromaticity, kekulisation, charges), canonical SMILES, stereo, energies.
"Valid" here is the valence rule alone; "the same molecule" is an isomorphism of the graph labelled with elements and bond
orders 1, 2, 3.

``compute_geometry`` adds the reference's 3D score (compute_metrics.py:366-402): the RMSD of every recovered sample against
its true molecule, the smallest over all isomorphisms of the two graphs (``isomorphisms`` on the host, the alignments of a
whole list in one launch of ``dl_best_rmsd``, ``csrc/rmsd.hip``), times ``sqrt(n_atoms / n_linker)``.

``analyze_clashes`` / ``compute_clashes`` answer what none of the above can, because they all drop the pocket first: does the
generated linker fit, or does it sit inside the protein?  Generated atoms against protein atoms under a van der Waals rule
(``dl_clash_scores``, ``csrc/clash.hip``); the reference has no code for it, the rule is stated in ``analyze_clashes``.

``analyze_shapes`` / ``compute_shapes`` score EVERY sample in 3D, recovered or not: the gridded van der Waals volume it shares
with its true molecule, in place (``dl_shape_scores``, ``csrc/shape.hip``).  This stands where the reference has the shape
half of SC-RDKit; the grid rule is this project's own after RDKit's defaults, not RDKit's, and the numbers are not RDKit's.

``analyze_rings`` / ``compute_rings`` score ring topology, which none of the above sees: the number of rings of the linker
(the reference's ``rings_n``, compute_metrics.py:128-145), three- and four-membered rings, and macrocycles closed through a
fragment (``dl_ring_scores``, ``csrc/rings.hip``).  The ring count is the cyclomatic number, not RDKit's symmetrised count.

``analyze_aromatic`` / ``compute_aromatic`` score what needs aromaticity: the aromatic rings of the linker, the reference's
ring filter ("no double bond inside a non-aromatic ring", compute_metrics.py:269-277) and the valence rule on bond orders
that treat aromatic rings properly (``dl_aromatic_rings``, ``csrc/aromatic.hip``).  Aromaticity is perceived from the 3D
geometry by a rule of this project's own - not RDKit's model, not OpenBabel's bond typing; see
``molecule_builder.refine_bond_orders``.

``analyze_fingerprints`` / ``tanimoto_nearest`` / ``compute_diversity`` answer the set-level questions exact identity cannot:
are the samples of one input different from each other, how close does a sample come to its true molecule, how close is the
nearest molecule of a reference set (``dl_fingerprints`` and ``dl_tanimoto_nearest``, ``csrc/fingerprint.hip``).  The circular
fingerprint is this project's own, built on the colours of ``molecule_keys`` - not RDKit's Morgan fingerprint.

``analyze_pharmacophores`` / ``compute_pharmacophores`` give the other half of SC-RDKit: pharmacophore features perceived from
the refined bond graph and their Best-mode feature-map match against the true molecule's (``dl_pharmacophore_features`` and
``dl_feature_match``, ``csrc/pharmacophore.hip``), and with the shape records ``sc_similarity``.  The feature rule is this
project's own, after RDKit's ``BaseFeatures.fdef`` and ``FeatMapParams`` defaults - not RDKit's numbers.

``analyze_interactions`` / ``compute_interactions`` answer what the clash score cannot: does the linker make contacts with
the protein, and more or fewer than the data set's own linker in the same pocket?  Heavy atoms typed as hydrophobic, donor or
acceptor from elements and geometry, and the intermolecular terms of Trott & Olson (AutoDock Vina, 2010) over them
(``dl_interaction_types`` and ``dl_interaction_scores``, ``csrc/interaction.hip``).  This project's own rule after that
published form - NOT AutoDock Vina's numbers: no hydrogens, no PDBQT typing, no search, no intramolecular term.

``analyze_pose_checks`` / ``compute_pose_checks`` ask what none of the above does: is the molecule's own 3D geometry
physically plausible?  Bond lengths against the typical lengths of the bond table, bond angles against the ideal of the
centre's class, and clashes between atoms four or more bonds apart (``dl_pose_checks``, ``csrc/pose_checks.hip``), on the
geometric bond orders.  This project's own rule after the idea of PoseBusters' intramolecular checks - NOT PoseBusters.

``select_records`` / ``compute_selection`` answer which few samples of an input to look at and how many really different
answers there are: Taylor-Butina clusters and MaxMin diverse subsets of the valid samples' fingerprints
(``dl_tanimoto_cluster`` and ``dl_tanimoto_pick``, ``csrc/select.hip``).  This project's own statement of both rules, on this
project's fingerprint - NOT RDKit's ``Butina.ClusterData`` or ``MaxMinPicker`` on ties.

``relax_to_host`` / ``compute_relaxation`` report what ``molecule_builder.relax`` (``dl_relax_molecules``, ``csrc/relax.hip``)
did to every sample: the restraint energy before and after, how far atoms moved, how many runs converged and how often the
distance table's bond list changed.  This project's own restrained clean-up - NOT UFF, MMFF or any toolkit's optimiser.

``canonical_ranks`` / ``smiles_to_host`` / ``compute_smiles`` say WHICH molecule a sample is: canonical atom ranks and a
canonical 64-bit code by an individualisation-refinement search over the colours of ``molecule_keys`` (``dl_canonical_ranks``,
``csrc/canon.hip``), and from the ranks one SMILES string per molecule (``molecule_builder.smiles``).  This project's own
rule - NOT RDKit's canonical ranks or canonical SMILES: Kekule orders as perceived, no aromatic lower case, no hydrogens
beyond brackets on over-valent atoms, no charges, no stereo, at most 256 atoms.

``match_patterns`` / ``analyze_patterns`` / ``compute_filters`` ask whether a sample contains a substructure: the reference's
PAINS filter (compute_metrics.py, RDKit's ``FilterCatalog`` over the SMARTS file given as ``pains_smarts_loc``) and any
other list of structural alerts, as a depth-first search per pattern and root atom on the refined bond graph
(``dl_substructure_match``, ``csrc/substructure.hip``; the patterns compiled by ``patterns.py``).  A subset of SMARTS and a
matching rule of this project's own - NOT RDKit's matcher: no charges, no stereo, no explicit hydrogens, no SSSR counts.
``stereo`` / ``stereo_codes`` / ``analyze_stereo`` / ``compute_stereo`` say WHICH STEREOISOMER a sample is, from its coordinates:
tetrahedral centres and stereo double bonds with labels relative to the colour classes of ``canonical_ranks``
(``dl_stereo_perceive``, ``csrc/stereo.hip``), stereo-aware codes by two more launches of ``dl_canonical_ranks`` on types widened
by the labels, and isomeric strings (``molecule_builder.smiles``).  This project's own rule - NOT RDKit's stereo perception
and NOT CIP: no R/S or E/Z names, no trivalent N, P or sulfoxide centres, no allenes or atropisomers.
"""
import ctypes
import math
from collections import namedtuple
from fractions import Fraction
from functools import partial

import numpy as np
import torch

from . import _lib, const
from . import patterns as pattern_compiler
from .molecule_builder import normalize_bonds, perceive_all_bonds, perceive_bonds, refine_bond_orders, smiles

Analysis = namedtuple('Analysis', 'n_atoms n_over n_components n_bonds key colour status bonds')
Graph = namedtuple('Graph', 'types bonds colours')
Molecule = namedtuple('Molecule', 'key n_over n_components status graph')

METRIC_NAMES = ('valence_validity', 'connectivity', 'validity_and_connectivity', 'uniqueness', 'novelty', 'recovery')
_MAX_VALENCE = {}


def _max_valence(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _MAX_VALENCE:
        _MAX_VALENCE[key] = const.max_valence_table(is_geom).to(device).contiguous()
    return _MAX_VALENCE[key]


def molecule_keys(one_hot, node_mask, found, is_geom, drop_mask=None):
    """``dl_molecule_keys`` on the result ``found`` of ``perceive_bonds`` for the same ``one_hot`` and ``node_mask``; device
    tensors in, an ``Analysis`` of device tensors out, no host synchronisation."""
    _lib.require_device('molecule_keys', one_hot=one_hot, node_mask=node_mask, drop_mask=drop_mask)
    B, N, nf = one_hot.shape
    if node_mask.numel() != B * N or (drop_mask is not None and drop_mask.numel() != B * N):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}')
    dev = one_hot.device
    one_hot, node_mask, drop_mask = (_lib.dense(t, dev, torch.float32) for t in (one_hot, node_mask, drop_mask))
    limits = _max_valence(dev, is_geom)
    i32 = partial(_lib.empty_i32, dev)
    out = Analysis(i32(B), i32(B), i32(B), i32(B), torch.empty(B, dtype=torch.int64, device=dev),
                   torch.empty((B, N), dtype=torch.int64, device=dev), i32(B), found)
    found = normalize_bonds(found, B, dev, 'molecule_keys')          # (what the kernel reads; the result keeps the caller's object)
    capacity = found.bonds.shape[1]
    args = _lib.DLMolKeysArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(),
        drop_mask=_lib.ptr(drop_mask), capacity=capacity,
        n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if capacity else None,
        valence_in=found.valence.data_ptr(), n_components_in=found.n_components.data_ptr(),
        status_in=found.status.data_ptr(), max_valence=limits.data_ptr(), max_valence_len=limits.numel(),
        n_atoms=out.n_atoms.data_ptr(), n_over=out.n_over.data_ptr(), n_components=out.n_components.data_ptr(),
        n_bonds=out.n_bonds.data_ptr(), key=out.key.data_ptr(), colour=out.colour.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_molecule_keys', args, dev)
    return out


def canonical_ranks(one_hot, node_mask, found, is_geom, drop_mask=None, max_leaves=256):
    """``dl_canonical_ranks`` (``csrc/canon.hip``) on the result ``found`` of ``perceive_bonds`` for the same ``one_hot`` and
    ``node_mask``, with the input handling of ``molecule_keys``; device tensors in, a dict of device tensors out, no host
    synchronisation.  ``is_geom`` plays no part in the rule (the graph carries type indices); it is taken so that the call
    reads like ``molecule_keys``.

    ``rank``      int32 ``[B,N]`` by atom number: the canonical ranks, a permutation of ``0..n-1`` over the kept atoms, -1 for
                  dropped atoms and from the atom count on
    ``code``      int64 ``[B]``: the 64 bits of the canonical code.  Equal codes: the same graph (elements, bond orders) up to
                  a 64-bit hash, where equal keys of ``molecule_keys`` are only necessary
    ``n_leaves``  int32 ``[B]``: leaves of the search that were evaluated
    ``status``    int32 ``[B]``: the bits of ``found.status`` plus ``_lib.DL_CANON_TOO_LARGE`` (more than 256 kept atoms or 2048
                  kept bonds: ranks -1, code 0), ``_lib.DL_CANON_BAD_BOND`` and ``_lib.DL_CANON_BUDGET`` (more than
                  ``max_leaves`` leaves or 32 branching levels: the ranks are a permutation, but not promised canonical)

    The rule is this project's own (``include/difflinker_hip.h``, restated in ``tests/canon_ref.py``), NOT RDKit's ranks."""
    _lib.require_device('canonical_ranks', one_hot=one_hot, node_mask=node_mask, drop_mask=drop_mask)
    B, N, nf = one_hot.shape
    if node_mask.numel() != B * N or (drop_mask is not None and drop_mask.numel() != B * N):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}')
    if not 1 <= int(max_leaves) <= _lib.DL_CANON_MAX_LEAVES:
        raise ValueError(f'max_leaves must be in 1..{_lib.DL_CANON_MAX_LEAVES}, got {max_leaves!r}')
    dev = one_hot.device
    one_hot, node_mask, drop_mask = (_lib.dense(t, dev, torch.float32) for t in (one_hot, node_mask, drop_mask))
    out = {'rank': _lib.empty_i32(dev, B, N), 'code': torch.empty(B, dtype=torch.int64, device=dev),
           'n_leaves': _lib.empty_i32(dev, B), 'status': _lib.empty_i32(dev, B)}
    found = normalize_bonds(found, B, dev, 'canonical_ranks')
    capacity = found.bonds.shape[1]
    args = _lib.DLCanonArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        capacity=capacity, n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if capacity else None,
        status_in=found.status.data_ptr(), max_leaves=int(max_leaves), rank=out['rank'].data_ptr(),
        code=out['code'].data_ptr(), n_leaves=out['n_leaves'].data_ptr(), status=out['status'].data_ptr())
    _lib.launch('dl_canonical_ranks', args, dev)
    return out


def smiles_to_host(result, one_hot, node_mask, found, drop_mask=None):
    """One string per molecule of a ``canonical_ranks`` result, on the host (``molecule_builder.smiles`` on the kept atoms,
    renumbered from 0, with the bonds of ``found`` between them and the canonical ranks): ``None`` for a molecule without
    ranks (``DL_CANON_TOO_LARGE``) or with more than 99 ring closures open at once.  Synchronises."""
    B, N = one_hot.shape[:2]
    rank = result['rank'].cpu().tolist()
    too_large = (result['status'].cpu() & _lib.DL_CANON_TOO_LARGE).tolist()
    n_bonds, bonds = found.n_bonds.cpu().tolist(), found.bonds.cpu()
    real = node_mask.reshape(B, N).cpu() != 0
    types = one_hot.detach().cpu().argmax(dim=2)
    out = []
    for b in range(B):
        t = types[b][real[b]].tolist()
        new = {k: r for k, r in enumerate(rank[b][:len(t)]) if r >= 0}      # atom number -> rank, kept atoms only
        if too_large[b]:
            out.append(None)
            continue
        index = {k: at for at, k in enumerate(new)}
        rows = bonds[b, :max(0, min(n_bonds[b], bonds.shape[1]))].tolist()
        out.append(smiles([t[k] for k in new], [(index[i], index[j], o) for i, j, o in rows if i in index and j in index],
                          [new[k] for k in new]))
    return out


SmilesRecord = namedtuple('SmilesRecord', 'smiles linker_smiles code canonical')
SMILES_NAMES = ('smiles_uniqueness', 'smiles_canonical')
SMILES_COLUMNS = ('file',) + SmilesRecord._fields


def smiles_records(one_hot, node_mask, found, linker_mask, drop_mask=None, max_leaves=256):
    """One ``SmilesRecord`` per molecule of a batch, from TWO launches of ``dl_canonical_ranks`` on the bond list ``found``
    (the list the ``.sdf`` files carry): ``smiles`` of the molecule without the ``drop_mask`` rows (the pocket), ``linker_smiles``
    of the ``linker_mask`` rows as a molecule of their own (as ``analyze_rings`` takes them), ``code`` the whole molecule's
    canonical code as 16 hex digits, and ``canonical``: 1 unless a launch set ``DL_CANON_BUDGET``, a bad-bond or the
    too-large bit (a string is ``''`` then where there is none).  Synchronises."""
    B, N = one_hot.shape[:2]
    linker = linker_mask.reshape(B, N).to(torch.float32)
    not_linker = (linker == 0).to(torch.float32)
    whole = canonical_ranks(one_hot, node_mask, found, True, drop_mask, max_leaves)
    part = canonical_ranks(one_hot, node_mask, found, True, not_linker, max_leaves)
    strings = smiles_to_host(whole, one_hot, node_mask, found, drop_mask)
    linker_strings = smiles_to_host(part, one_hot, node_mask, found, not_linker)
    flagged = ((whole['status'] | part['status']) &
               (_lib.DL_CANON_BUDGET | _lib.DL_CANON_BAD_BOND | _lib.DL_CANON_TOO_LARGE)).cpu().tolist()
    codes = whole['code'].cpu().tolist()
    return [SmilesRecord(strings[b] or '', linker_strings[b] or '', format(codes[b] & 0xFFFFFFFFFFFFFFFF, '016x'),
                         0 if flagged[b] or strings[b] is None or linker_strings[b] is None else 1) for b in range(B)]


def write_smiles_csv(path, files, records, isomeric=None):
    """``smiles.csv``: one row per written file (``files``: its name as the other reports give it, with the record of its
    molecule), columns ``SMILES_COLUMNS``; with ``isomeric`` (one string per file, ``StereoRecord.isomeric_smiles``) a last
    column ``isomeric_smiles``."""
    import csv
    with open(path, 'w', newline='') as f:
        out = csv.writer(f)
        out.writerow(SMILES_COLUMNS + (() if isomeric is None else ('isomeric_smiles',)))
        for at, (name, record) in enumerate(zip(files, records)):
            out.writerow((name,) + tuple(record) + (() if isomeric is None else (isomeric[at],)))


def compute_smiles(rows, pred, true=None):
    """The two scores of the strings: ``rows`` are the ``SmilesRecord`` values of the samples (``smiles_records``), ``pred`` and
    ``true`` the ``Molecule`` records ``compute_metrics`` takes for the same samples.

    ``smiles_uniqueness``  distinct strings among the samples ``uniqueness`` counts classes of (valid, in one piece, clean
                           status, and with ``true`` a true molecule that is so as well) / their number: all inputs at once,
                           as ``uniqueness`` is.  The two agree unless a 64-bit code collided or a budget was hit.  0 without
                           such a sample
    ``smiles_canonical``   share of rows with ``canonical`` set; 0 without rows"""
    chosen = [k for k in range(len(rows)) if _good(pred[k]) and (true is None or _good(true[k]))]
    distinct = {rows[k].smiles for k in chosen}
    return {'smiles_uniqueness': len(distinct) / len(chosen) if chosen else 0.0,
            'smiles_canonical': sum(1 for r in rows if r.canonical) / len(rows) if rows else 0.0}


def analyze(one_hot, x, node_mask, is_geom, drop_mask=None, margins=const.MARGINS_EDM):
    """Bonds, then scores and keys, of every molecule of a batch on the HIP device: ``one_hot [B,N,nf]``, ``x [B,N,3]``,
    ``node_mask`` and the optional ``drop_mask`` (the pocket atoms of a pocket model) ``[B,N,1]`` or ``[B,N]``.

    Returns an ``Analysis`` of device tensors: ``n_atoms``, ``n_over``, ``n_components``, ``n_bonds`` (int32 ``[B]``, all over the
    atoms that are not dropped), ``key`` (int64 ``[B]``: the 64 bits of the key), ``colour`` (int64 ``[B,N]`` by atom number, 0
    for dropped atoms and beyond the atom count), ``status`` (int32 ``[B]``: ``_lib.DL_BONDS_*`` / ``_lib.DL_KEYS_*`` bits) and
    ``bonds``, the ``perceive_all_bonds`` result it was computed from.  The bond list is never cut short
    (``perceive_all_bonds`` widens it), and nothing synchronises beyond what that call does."""
    _lib.require_device('analyze', one_hot=one_hot, x=x, node_mask=node_mask)
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    return molecule_keys(one_hot, node_mask, found, is_geom, drop_mask)


def to_host(result, one_hot, node_mask, drop_mask=None):
    """The ``Molecule`` records ``compute_metrics`` reads, one per row of an ``Analysis``, on the host.  The graph of a record
    holds the kept atoms only, renumbered from 0: element indices, bonds ``(i, j, order)`` and the atoms' final colours."""
    B, N = one_hot.shape[:2]
    keys = result.key.cpu().tolist()
    n_over, n_comp, status = result.n_over.cpu().tolist(), result.n_components.cpu().tolist(), result.status.cpu().tolist()
    colour = result.colour.cpu()
    n_bonds, bonds = result.bonds.n_bonds.cpu().tolist(), result.bonds.bonds.cpu()
    real = node_mask.reshape(B, N).cpu() != 0
    dropped = None if drop_mask is None else drop_mask.reshape(B, N).cpu() != 0
    types = one_hot.detach().cpu().argmax(dim=2)
    out = []
    for b in range(B):
        t = types[b][real[b]].tolist()
        keep = [True] * len(t) if dropped is None else (~dropped[b][real[b]]).tolist()
        new = {}
        for k, kept in enumerate(keep):
            if kept:
                new[k] = len(new)
        rows = bonds[b, :min(n_bonds[b], bonds.shape[1])].tolist()
        graph = Graph([t[k] for k in new], [(new[i], new[j], o) for i, j, o in rows if i in new and j in new],
                      [colour[b, k].item() for k in new])
        out.append(Molecule(keys[b], n_over[b], n_comp[b], status[b], graph))
    return out


def _adjacency(graph):
    adj = [dict() for _ in graph.types]
    for i, j, order in graph.bonds:
        adj[i][j] = order
        adj[j][i] = order
    return adj


def same_molecule(a, b):
    """Exact isomorphism of two ``Graph`` values (element per atom, order per bond): a backtracking match that pairs only
    atoms of equal final colour (of equal element when a graph carries no colours) and equal degree.  It is meant for
    molecules whose keys are equal; refinement then leaves one candidate per atom in all but symmetric positions, and the
    match is confirmed in linear time.  Its answer does not depend on the colours being right, only its speed does."""
    n = len(a.types)
    if n != len(b.types) or len(a.bonds) != len(b.bonds):
        return False
    coloured = a.colours is not None and b.colours is not None
    adj_a, adj_b = _adjacency(a), _adjacency(b)
    if sum(len(r) for r in adj_a) != 2 * len(a.bonds) or sum(len(r) for r in adj_b) != 2 * len(b.bonds):
        raise ValueError('a bond is listed twice or joins an atom to itself')
    tag_a = [(a.colours[k] if coloured else 0, a.types[k], len(adj_a[k])) for k in range(n)]
    tag_b = [(b.colours[k] if coloured else 0, b.types[k], len(adj_b[k])) for k in range(n)]
    if sorted(tag_a) != sorted(tag_b):
        return False
    # visit a's atoms so that each one follows a neighbour where there is one: the bonds to matched atoms prune early
    order, seen = [], [False] * n
    for root in range(n):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        while queue:
            u = queue.pop(0)
            order.append(u)
            for v in adj_a[u]:
                if not seen[v]:
                    seen[v] = True
                    queue.append(v)
    by_tag = {}
    for v in range(n):
        by_tag.setdefault(tag_b[v], []).append(v)
    image, used = [-1] * n, [False] * n
    choice = [0] * n                                       # next candidate to try at each depth
    depth = 0
    while 0 <= depth < n:
        u = order[depth]
        candidates = by_tag[tag_a[u]]
        placed = False
        while choice[depth] < len(candidates):
            v = candidates[choice[depth]]
            choice[depth] += 1
            if used[v]:
                continue
            # equal degrees and every bond of u to a matched atom found in b with its order: with equal bond counts the
            # finished map is onto the bonds of b as well
            if all(image[w] < 0 or adj_b[v].get(image[w]) == o for w, o in adj_a[u].items()):
                image[u], used[v] = v, True
                placed = True
                break
        if placed:
            depth += 1
            if depth < n:
                choice[depth] = 0
        else:
            depth -= 1
            if depth >= 0:
                used[image[order[depth]]] = False
                image[order[depth]] = -1
    return depth == n


def isomorphisms(a, b, limit=None):
    """Every isomorphism of two ``Graph`` values, found with the pruning of ``same_molecule`` (final colour, element and
    degree tags, the same visiting order, bond orders against matched neighbours), continuing after each complete assignment
    instead of returning.  Returns ``(maps, truncated)``: ``maps[i][k]`` is the atom of ``b`` matched to atom ``k`` of ``a``;
    at most ``limit`` maps are returned, and ``truncated`` says that there are more.  The first map is the one
    ``same_molecule`` stops at, and ``bool(maps) == same_molecule(a, b)`` for every ``limit`` of at least 1 (or ``None``: no
    limit); a ``limit`` below 1 asks for no map and gets ``([], False)`` without a search."""
    n = len(a.types)
    if n != len(b.types) or len(a.bonds) != len(b.bonds) or (limit is not None and limit < 1):
        return [], False
    coloured = a.colours is not None and b.colours is not None
    adj_a, adj_b = _adjacency(a), _adjacency(b)
    if sum(len(r) for r in adj_a) != 2 * len(a.bonds) or sum(len(r) for r in adj_b) != 2 * len(b.bonds):
        raise ValueError('a bond is listed twice or joins an atom to itself')
    tag_a = [(a.colours[k] if coloured else 0, a.types[k], len(adj_a[k])) for k in range(n)]
    tag_b = [(b.colours[k] if coloured else 0, b.types[k], len(adj_b[k])) for k in range(n)]
    if sorted(tag_a) != sorted(tag_b):
        return [], False
    if n == 0:
        return [[]], False
    order, seen = [], [False] * n
    for root in range(n):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        while queue:
            u = queue.pop(0)
            order.append(u)
            for v in adj_a[u]:
                if not seen[v]:
                    seen[v] = True
                    queue.append(v)
    by_tag = {}
    for v in range(n):
        by_tag.setdefault(tag_b[v], []).append(v)
    maps, image, used = [], [-1] * n, [False] * n
    choice = [0] * n
    depth = 0
    while depth >= 0:
        if depth == n:                                     # complete: record it and go on from the last atom's next candidate
            if limit is not None and len(maps) == limit:
                return maps, True
            maps.append(list(image))
            depth -= 1
            used[image[order[depth]]] = False
            image[order[depth]] = -1
            continue
        u = order[depth]
        candidates = by_tag[tag_a[u]]
        placed = False
        while choice[depth] < len(candidates):
            v = candidates[choice[depth]]
            choice[depth] += 1
            if used[v]:
                continue
            if all(image[w] < 0 or adj_b[v].get(image[w]) == o for w, o in adj_a[u].items()):
                image[u], used[v] = v, True
                placed = True
                break
        if placed:
            depth += 1
            if depth < n:
                choice[depth] = 0
        else:
            depth -= 1
            if depth >= 0:
                used[image[order[depth]]] = False
                image[order[depth]] = -1
    return maps, False


def group(keys, graphs):
    """The classes of identical molecules as lists of positions, in order of first appearance: buckets of equal ``keys``,
    each split by ``same_molecule``."""
    buckets = {}
    for pos, key in enumerate(keys):
        classes = buckets.setdefault(key, [])
        for members in classes:
            if same_molecule(graphs[members[0]], graphs[pos]):
                members.append(pos)
                break
        else:
            classes.append([pos])
    return sorted((members for classes in buckets.values() for members in classes), key=lambda m: m[0])


def _good(mol):
    return mol.n_over == 0 and mol.n_components == 1 and mol.status == 0


def compute_metrics(pred, true=None, input_index=None):
    """Scores of the predicted ``Molecule`` records ``pred`` (``to_host``), each a plain float in [0, 1].

    ``true[k]`` is the data set's molecule for the input ``pred[k]`` was sampled from, and ``input_index[k]`` names that input
    (samples of one input share it).  As in the reference's ``sample_and_analyze`` (lightning.py:380-384), a prediction
    counts only when its true molecule is itself valid and connected; the others are dropped first.

    ``valence_validity``           share of predictions in which no atom carries more bonds than ``const.ALLOWED_BONDS`` allows
                                   (and whose status is clean).  This is the valence rule, NOT RDKit's sanitisation.
    ``connectivity``               share in one piece.
    ``validity_and_connectivity``  both at once - named after the reference's key because it is the quantity
                                   ``compute_best_validation_metrics`` selects by; again the valence rule, not sanitisation.
    ``uniqueness``                 classes of identical molecules among the valid and connected predictions / their number.
    ``novelty``                    share of those classes that match no true molecule.
    ``recovery``                   share of inputs with at least one sample identical to the input's true molecule.

    Without ``true`` (generation from a fragment file has none) novelty and recovery are left out and nothing is dropped.
    No predictions: every score is 0, as the reference's ``compute_metrics`` answers (metrics.py:87-95)."""
    names = METRIC_NAMES if true is not None else METRIC_NAMES[:4]
    if true is not None:
        if not (len(true) == len(pred) == len(input_index)):
            raise ValueError(f'{len(pred)} predictions, {len(true)} true molecules, {len(input_index)} input indices')
        rows = [k for k in range(len(pred)) if _good(true[k])]
        pred, true, input_index = [pred[k] for k in rows], [true[k] for k in rows], [input_index[k] for k in rows]
    if len(pred) == 0:
        return {name: 0.0 for name in names}
    valid = [m.n_over == 0 and m.status == 0 for m in pred]
    connected = [m.n_components == 1 for m in pred]
    good = [k for k in range(len(pred)) if _good(pred[k])]
    classes = group([pred[k].key for k in good], [pred[k].graph for k in good])
    out = {'valence_validity': sum(valid) / len(pred), 'connectivity': sum(connected) / len(pred),
           'validity_and_connectivity': len(good) / len(pred), 'uniqueness': len(classes) / len(good) if good else 0.0}
    if true is None:
        return out
    by_key = {}
    for m in true:
        by_key.setdefault(m.key, []).append(m.graph)
    known = lambda m: any(same_molecule(g, m.graph) for g in by_key.get(m.key, ()))   # noqa: E731
    novel = [members for members in classes if not known(pred[good[members[0]]])]
    out['novelty'] = len(novel) / len(classes) if classes else 0.0
    inputs, recovered = set(input_index), set()
    for k in good:
        if input_index[k] not in recovered and pred[k].key == true[k].key and same_molecule(pred[k].graph, true[k].graph):
            recovered.add(input_index[k])
    out['recovery'] = len(recovered) / len(inputs)
    return {name: float(out[name]) for name in names}


def kept_positions(x, node_mask, drop_mask=None):
    """The coordinates of the kept atoms of every molecule, compacted to the front in the numbering ``to_host`` gives a
    ``Graph`` (real rows in row order, the dropped ones left out): ``x [B,N,3]`` and masks ``[B,N,1]`` or ``[B,N]`` in, the
    compact fp32 ``[B,N,3]`` (zero from the count on) and the int32 counts ``[B]`` out.  Tensor ops on the tensors' own device,
    no host synchronisation."""
    B, N = x.shape[:2]
    keep = node_mask.reshape(B, N) != 0
    if drop_mask is not None:
        keep = keep & (drop_mask.reshape(B, N) == 0)
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)              # kept rows first, each group in row order
    counts = keep.sum(1)
    compact = torch.gather(x.to(torch.float32), 1, order[:, :, None].expand(B, N, 3))
    compact = compact * (torch.arange(N, device=x.device)[None, :] < counts[:, None])[:, :, None]
    return compact.contiguous(), counts.to(torch.int32)


def pack_maps(maps, n_max):
    """The map table of ``dl_best_rmsd`` on the host: ``maps[p]`` is the list of pair ``p``'s maps (each a list of its atom
    count's length).  Returns ``(table, offsets)``: an int16 tensor of ``offsets[-1] * n_max`` 16-bit indices and the int32
    offsets ``[P + 1]``; the block of pair ``p`` starts at ``offsets[p] * n_max`` and is atom-major (``include/difflinker_hip.h``)."""
    if n_max > 32768:
        raise ValueError(f'n_max {n_max}: the indices are packed through int16')
    offsets = np.zeros(len(maps) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(m) for m in maps])
    if offsets[-1] >= 2 ** 31:
        raise ValueError(f'{offsets[-1]} maps do not fit the 32-bit offsets of one launch')
    table = np.zeros(int(offsets[-1]) * n_max, dtype=np.int16)
    for p, rows in enumerate(maps):
        if len(rows):
            block = np.asarray(rows, dtype=np.int16).reshape(len(rows), -1).T      # [n, m]: atom-major
            at = int(offsets[p]) * n_max
            table[at:at + block.size] = block.reshape(-1)
    return torch.from_numpy(table), torch.from_numpy(offsets.astype(np.int32))


def best_rmsd(xa, xb, n_atoms, maps, offsets):
    """``dl_best_rmsd`` on a list of pairs: ``xa``, ``xb`` fp32 ``[P,n_max,3]`` (``kept_positions`` rows), ``n_atoms`` int32
    ``[P]``, and the table and offsets of ``pack_maps``, all on the HIP device.  Returns device tensors ``(rmsd, best,
    status)``: fp32 ``[P]`` (NaN where ``status`` is not 0), the winning map's index within its pair (of equal ones the
    lowest) and the ``_lib.DL_RMSD_*`` bits.  One launch, no host synchronisation."""
    _lib.require_device('best_rmsd', xa=xa, xb=xb, n_atoms=n_atoms, maps=maps, offsets=offsets)
    P, n_max = xa.shape[:2]
    if xa.shape != (P, n_max, 3) or xb.shape != xa.shape or n_atoms.numel() != P or offsets.numel() != P + 1 or n_max < 1 \
            or maps.numel() % n_max:
        raise ValueError(f'shapes disagree: xa {tuple(xa.shape)}, xb {tuple(xb.shape)}, n_atoms {tuple(n_atoms.shape)}, '
                         f'offsets {tuple(offsets.shape)}, maps {tuple(maps.shape)}')
    if maps.dtype not in (torch.int16, torch.uint16):
        raise ValueError(f'maps must hold 16-bit indices, got {maps.dtype}')
    dev = xa.device
    xa, xb = (_lib.dense(t, dev, torch.float32) for t in (xa, xb))
    n_atoms, offsets = (_lib.dense(t, dev, torch.int32) for t in (n_atoms, offsets))
    maps = maps.to(dev).contiguous()
    rmsd = torch.empty(P, dtype=torch.float32, device=dev)
    best, status = _lib.empty_i32(dev, P), _lib.empty_i32(dev, P)
    args = _lib.DLRmsdArgs(P=P, n_max=n_max, xa=xa.data_ptr(), xb=xb.data_ptr(), n_atoms=n_atoms.data_ptr(),
                           map_offsets=offsets.data_ptr(), maps=maps.data_ptr() if maps.numel() else None,
                           maps_capacity=maps.numel() // n_max, rmsd=rmsd.data_ptr(), best=best.data_ptr(),
                           status=status.data_ptr())
    _lib.launch('dl_best_rmsd', args, dev)
    return rmsd, best, status


def _stack_rows(rows, n_max):
    """``[len(rows), n_max, 3]`` fp32 from per-molecule ``[>= n, 3]`` rows of any widths, in one padding op, not one copy per
    row: views cut to ``n_max``, padded to the longest, then to ``n_max``.  Rows from an atom's count on are never read."""
    out = torch.nn.utils.rnn.pad_sequence([r[:n_max].to(torch.float32) for r in rows], batch_first=True)
    if out.shape[1] < n_max:
        out = torch.nn.functional.pad(out, (0, 0, 0, n_max - out.shape[1]))
    return out.contiguous()


GEOMETRY_NAMES = ('rmsd', 'rmsd_molecules', 'rmsd_truncated')


def compute_geometry(pred, true, pred_x, true_x, n_linker, max_matches=65536):
    """The reference's RMSD score (compute_metrics.py:366-402) over the ``Molecule`` records ``pred`` and ``true`` of
    ``compute_metrics``: every prediction that is valid, connected and the same molecule as its (valid, connected) true one
    is aligned onto it under every isomorphism of the two graphs - at most ``max_matches`` of them - and the smallest RMSD,
    times ``sqrt(n_atoms / n_linker[k])``, enters the mean.  ``pred_x[k]`` and ``true_x[k]`` are device tensors whose first
    rows are the atoms' coordinates in the graphs' numbering (rows of ``kept_positions``).  Predictions with
    ``n_linker[k] == 0`` are skipped.  All alignments run in ONE ``best_rmsd`` launch.

    Returns ``rmsd`` (the mean as a float; ``None`` when no sample recovered its molecule, where the reference's mean of an
    empty list is NaN, which JSON cannot hold), ``rmsd_molecules`` (how many samples it is over: recovered samples, as in the
    reference, not inputs) and ``rmsd_truncated`` (how many of them have more than ``max_matches`` isomorphisms; they are
    scored over the ones found).  A pair the kernel flags (``_lib.DL_RMSD_*``: more atoms than it takes) is left out of both.

    What this is NOT: RDKit's GetBestRMS to the letter - no hydrogens (as in the reference, which strips them), no stereo
    perception, and the correspondences come from the graph of elements and bond orders instead of RDKit's substructure match."""
    if not (len(pred) == len(true) == len(pred_x) == len(true_x) == len(n_linker)):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true molecules, {len(pred_x)} and {len(true_x)} coordinate sets, '
                         f'{len(n_linker)} linker sizes')
    rows, maps, truncated = [], [], []
    for k in range(len(pred)):
        if not (_good(true[k]) and _good(pred[k]) and pred[k].key == true[k].key and int(n_linker[k]) > 0):
            continue
        found, cut = isomorphisms(pred[k].graph, true[k].graph, max_matches)
        if found and len(found[0]):
            rows.append(k)
            maps.append(found)
            truncated.append(cut)
    if not rows:
        return {'rmsd': None, 'rmsd_molecules': 0, 'rmsd_truncated': 0}
    counts = [len(pred[k].graph.types) for k in rows]
    n_max = max(counts)
    dev = pred_x[rows[0]].device
    xa, xb = (_stack_rows([xs[k] for k in rows], n_max) for xs in (pred_x, true_x))
    table, offsets = pack_maps(maps, n_max)
    rmsd, _, status = best_rmsd(xa, xb, torch.tensor(counts, dtype=torch.int32, device=dev), table.to(dev), offsets.to(dev))
    rmsd, status = rmsd.cpu().tolist(), status.cpu().tolist()
    scaled = [rmsd[p] * math.sqrt(counts[p] / int(n_linker[k])) for p, k in enumerate(rows) if status[p] == 0]
    cut = sum(1 for p in range(len(rows)) if status[p] == 0 and truncated[p])
    return {'rmsd': sum(scaled) / len(scaled) if scaled else None, 'rmsd_molecules': len(scaled), 'rmsd_truncated': cut}


Clashes = namedtuple('Clashes', 'n_query n_target n_clashes n_clash_atoms n_contacts min_dist2 status atom_clashes '
                                'atom_min_dist2 query_mask')
ClashRecord = namedtuple('ClashRecord', 'n_query n_target n_clashes n_clash_atoms n_contacts min_distance status atom_clashes '
                                        'atom_min_distance')
CLASH_NAMES = ('clash_molecules', 'clash_flagged', 'clash_free', 'clashes_per_molecule', 'clash_atoms_share',
               'contacts_per_molecule', 'min_distance')
CLASH_TRUE_NAMES = ('true_clashes_per_molecule', 'true_clash_free', 'clash_excess')


def analyze_clashes(one_hot, x, query_mask, target_mask=None, protein=None, is_geom=True, scale=0.75, tolerance=0.0,
                    contact_cutoff=4.0, thresholds=None):
    """Steric clashes of generated atoms with the protein, for every molecule of a batch in one launch of
    ``dl_clash_scores`` on the HIP device.

    THE RULE (this project's own: the reference reports clash counts in its paper and has no code for them).  Atoms are heavy
    atoms, hydrogens are implicit.  A pair is one QUERY atom - a row of ``query_mask [B,N]`` or ``[B,N,1]``, the generated
    atoms - and one TARGET atom - a row of ``target_mask`` (the batch's ``pocket_mask``) that is not a query row, or an atom
    of ``protein = (positions [M,3], types [M])``, a list shared by all molecules and given in the frame of ``x``.  An atom's
    type is the first largest entry of its ``one_hot [B,N,nf]`` row.  With ``t = threshold[query type][target type]``
    (``const.clash_threshold_table(is_geom, scale, tolerance)``: ``scale * (r_vdw[a] + r_vdw[b]) - tolerance`` over Bondi's
    radii, fp32, or the caller's ``thresholds [nf,nf]``) a pair CLASHES when ``d2 < t * t`` and ``t > 0``, and is a CONTACT
    when ``d2 < contact_cutoff * contact_cutoff``; ``d2 = ((dx*dx) + (dy*dy)) + (dz*dz)`` in fp32 without fused
    multiply-adds, the comparisons strict.  ``scale = 1`` is the plain sum of the radii; with implicit hydrogens that flags
    ordinary contacts, hence the default 0.75.

    Returns a ``Clashes`` of device tensors: ``n_query``, ``n_target``, ``n_clashes`` (pairs), ``n_clash_atoms`` (query atoms
    with a clash), ``n_contacts`` (int32 ``[B]``), ``min_dist2`` (fp32 ``[B]``: the smallest SQUARED distance, ``+inf``
    without a pair), ``status`` (int32 ``[B]``: ``_lib.DL_CLASH_*`` bits; with ``NONFINITE`` or ``TOO_LARGE`` the counts are
    0 and the minima NaN), ``atom_clashes`` (int32 ``[B,N]``, 0 on non-query rows), ``atom_min_dist2`` (fp32 ``[B,N]``,
    ``+inf`` on non-query rows and without targets) and the ``query_mask`` it was given.  No host synchronisation.

    What this is NOT: no hydrogens, no clashes inside the ligand, no energy or docking score."""
    shared = () if protein is None else tuple(protein)
    _lib.require_device('analyze_clashes', one_hot=one_hot, x=x, query_mask=query_mask, target_mask=target_mask,
                        thresholds=thresholds, **{f'protein[{k}]': t for k, t in enumerate(shared)})
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or query_mask.numel() != B * N or (target_mask is not None and target_mask.numel() != B * N):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, query_mask '
                         f'{tuple(query_mask.shape)}')
    dev = one_hot.device
    f32 = partial(_lib.dense, device=dev, dtype=torch.float32)
    one_hot, x, qm = f32(one_hot), f32(x), f32(query_mask).reshape(B, N)
    tm = None if target_mask is None else f32(target_mask).reshape(B, N)
    M, px, pt = 0, None, None
    if protein is not None:
        px, pt = f32(shared[0]), _lib.dense(shared[1], dev, torch.int32)
        M = pt.numel()
        if px.shape != (M, 3):
            raise ValueError(f'shapes disagree: protein positions {tuple(px.shape)}, types {tuple(pt.shape)}')
    if thresholds is None:
        thresholds = const.clash_threshold_table(is_geom, scale, tolerance).to(dev)
    thresholds = f32(thresholds)
    if thresholds.shape != (nf, nf):
        raise ValueError(f'thresholds {tuple(thresholds.shape)} for {nf} atom types')
    i32 = partial(_lib.empty_i32, dev)
    out = Clashes(i32(B), i32(B), i32(B), i32(B), i32(B), torch.empty(B, dtype=torch.float32, device=dev), i32(B), i32(B, N),
                  torch.empty(B, N, dtype=torch.float32, device=dev), qm)
    args = _lib.DLClashArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), query_mask=qm.data_ptr(),
        target_mask=_lib.ptr(tm), M=M, target_x=px.data_ptr() if M else None,
        target_type=pt.data_ptr() if M else None, threshold=thresholds.data_ptr(), contact_cutoff=float(contact_cutoff),
        n_query=out.n_query.data_ptr(), n_target=out.n_target.data_ptr(), n_clashes=out.n_clashes.data_ptr(),
        n_clash_atoms=out.n_clash_atoms.data_ptr(), n_contacts=out.n_contacts.data_ptr(), min_dist2=out.min_dist2.data_ptr(),
        status=out.status.data_ptr(), atom_clashes=out.atom_clashes.data_ptr(), atom_min_dist2=out.atom_min_dist2.data_ptr())
    _lib.launch('dl_clash_scores', args, dev)
    return out


def clashes_to_host(result):
    """The ``ClashRecord`` values ``compute_clashes`` reads, one per molecule of a ``Clashes``, on the host: the counts as
    ints, ``min_distance`` in Angstrom (the fp64 square root of ``min_dist2``: ``inf`` without a pair, NaN for a flagged molecule),
    ``status``, and ``atom_clashes`` / ``atom_min_distance`` as lists over the QUERY atoms only, in row order."""
    cols = [getattr(result, name).cpu().tolist() for name in ('n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts')]
    root = lambda t: np.sqrt(t.cpu().numpy().astype(np.float64))      # noqa: E731  (numpy's square root is correctly rounded)
    closest = root(result.min_dist2).tolist()
    status = result.status.cpu().tolist()
    rows = result.query_mask.cpu() != 0
    atom_c, atom_d = result.atom_clashes.cpu(), root(result.atom_min_dist2)
    return [ClashRecord(cols[0][b], cols[1][b], cols[2][b], cols[3][b], cols[4][b], closest[b], status[b],
                        atom_c[b][rows[b]].tolist(), atom_d[b][rows[b].numpy()].tolist()) for b in range(len(status))]


def _clash_scored(record):
    return not record.status & (_lib.DL_CLASH_NONFINITE | _lib.DL_CLASH_TOO_LARGE)


def compute_clashes(pred, true=None):
    """Scores of the ``ClashRecord`` values ``pred`` (``clashes_to_host``), plain numbers:

    ``clash_molecules``        records scored: the flagged ones (``DL_CLASH_NONFINITE`` / ``DL_CLASH_TOO_LARGE``: their counts
                               mean nothing) are left out of everything below
    ``clash_flagged``          how many were left out
    ``clash_free``             share of the scored records with ``n_clashes == 0``
    ``clashes_per_molecule``   mean number of clashing pairs
    ``clash_atoms_share``      clashing query atoms over query atoms, both summed over the scored records
    ``contacts_per_molecule``  mean number of contact pairs
    ``min_distance``           mean of the per-molecule smallest distance in Angstrom; records without a pair are left out,
                               ``None`` when that leaves none

    With ``true`` - one record per prediction: the data set's own linker scored in the same pocket - three more keys, over the
    positions where both records are scored: ``true_clashes_per_molecule``, ``true_clash_free`` and ``clash_excess`` (the
    mean of ``pred - true`` clashing pairs).  Without ``true`` they are absent.  Nothing scored: every share and mean is 0."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    good = [m for m in pred if _clash_scored(m)]
    n = len(good)
    mean = lambda values: float(sum(values) / len(values)) if values else 0.0      # noqa: E731
    queries = sum(m.n_query for m in good)
    closest = [m.min_distance for m in good if math.isfinite(m.min_distance)]
    out = {'clash_molecules': n, 'clash_flagged': len(pred) - n,
           'clash_free': mean([m.n_clashes == 0 for m in good]),
           'clashes_per_molecule': mean([m.n_clashes for m in good]),
           'clash_atoms_share': float(sum(m.n_clash_atoms for m in good) / queries) if queries else 0.0,
           'contacts_per_molecule': mean([m.n_contacts for m in good]),
           'min_distance': mean(closest) if closest else None}
    if true is not None:
        both = [(p, t) for p, t in zip(pred, true) if _clash_scored(p) and _clash_scored(t)]
        out['true_clashes_per_molecule'] = mean([t.n_clashes for _, t in both])
        out['true_clash_free'] = mean([t.n_clashes == 0 for _, t in both])
        out['clash_excess'] = mean([p.n_clashes - t.n_clashes for p, t in both])
    return out


XsTypes = namedtuple('XsTypes', 'xs_type status')
Interactions = namedtuple('Interactions', 'n_query n_target n_pairs n_hbonds n_hydrophobic terms status atom_terms xs_type '
                                          'type_status query_mask')
InteractionRecord = namedtuple('InteractionRecord', 'n_query n_target n_pairs n_hbonds n_hydrophobic terms score status '
                                                    'atom_scores')
INTERACTION_TERMS = ('gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond')
INTERACTION_NAMES = ('interaction_molecules', 'interaction_flagged', 'interaction_score') + \
    tuple(f'interaction_{name}' for name in INTERACTION_TERMS) + \
    ('hbonds_per_molecule', 'hydrophobic_contacts_per_molecule', 'interaction_score_per_atom')
INTERACTION_TRUE_NAMES = ('true_interaction_score', 'true_hbonds_per_molecule', 'interaction_excess')
FIXED_ONE = 4294967296.0            # 2^32: one unit of the fixed-point terms


def interaction_types(one_hot, x, group, is_geom=True, margins=const.MARGINS_EDM):
    """Heavy atoms typed as hydrophobic, hydrogen-bond donor or acceptor from elements and geometry alone, for every molecule
    of a batch in one launch of ``dl_interaction_types`` (``csrc/interaction.hip``) on the HIP device.

    ``one_hot [B,N,nf]`` (an atom's element is the first largest entry, in the project's order C O N F S Cl Br I P),
    ``x [B,N,3]``, ``group [B,N]`` or ``[B,N,1]`` of integers: 0 = the row is not typed and never read; rows of one molecule
    with the same non-zero id are typed among themselves.  Two rows of a group are NEIGHBOURS when ``perceive_bonds`` would
    bond them (the single-bond bound of ``const.bond_threshold_table(is_geom, margins)``, the same fp32 arithmetic, strict);
    ``deg`` counts them, ``hetero`` says one is not carbon.  C is HYDROPHOBIC when not hetero; F, Cl, Br, I are HYDROPHOBIC;
    N is a DONOR when ``deg < 3`` and never an acceptor; O is always an ACCEPTOR and a DONOR too when ``deg == 0`` (a water)
    or when ``deg == 1`` and that neighbour lies at ``d2 >= 1.6875`` A^2 (a hydroxyl, not a carbonyl); S and P carry no flag.

    KNOWN MISREADINGS: a pyridine or nitrile N is typed a donor; a histidine's two N are both donors; pocket residues cut at
    the pocket boundary lose a neighbour.

    Returns ``XsTypes(xs_type, status)``: int32 ``[B,N]`` - the element in bits 0-3, ``_lib.DL_XS_HYDROPHOBIC`` / ``DL_XS_DONOR``
    / ``DL_XS_ACCEPTOR`` above, -1 on rows of group 0 - and int32 ``[B]``: ``_lib.DL_INTERACT_NONFINITE`` when a typed row is
    not finite, the molecule's rows are then all -1.  No host synchronisation."""
    _lib.require_device('interaction_types', one_hot=one_hot, x=x, group=group)
    if one_hot.dim() != 3:
        raise ValueError(f'one_hot {tuple(one_hot.shape)} is not [B,N,nf]')
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or group.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, group {tuple(group.shape)}')
    dev = one_hot.device
    one_hot, x = _lib.dense(one_hot, dev, torch.float32), _lib.dense(x, dev, torch.float32)
    group = _lib.dense(group, dev, torch.int32).reshape(B, N)
    table = const.bond_threshold_table(is_geom, margins)[..., 0].contiguous().to(dev)
    if table.shape != (nf, nf):
        raise ValueError(f'{nf} atom types in one_hot, {table.shape[0]} in the vocabulary')
    out = XsTypes(_lib.empty_i32(dev, B, N), _lib.empty_i32(dev, B))
    if N == 0:
        return out
    args = _lib.DLInteractTypesArgs(B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), group=group.data_ptr(),
                                    table=table.data_ptr(), xs_type=out.xs_type.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_interaction_types', args, dev)
    return out


def protein_types(positions, types, is_geom=True):
    """The ``xs_types`` int32 ``[M]`` of a shared target list ``positions [M,3]``, ``types [M]`` (element indices), typed as
    one group in one launch, for the caller to keep per protein and hand to ``analyze_interactions`` as
    ``protein = (positions, types, xs_types)``.  An atom whose type is outside the vocabulary is not typed (-1) and is then
    skipped by the score."""
    _lib.require_device('protein_types', positions=positions, types=types)
    M = types.numel()
    if positions.shape != (M, 3):
        raise ValueError(f'shapes disagree: protein positions {tuple(positions.shape)}, types {tuple(types.shape)}')
    dev = positions.device
    nf = const.GEOM_NUMBER_OF_ATOM_TYPES if is_geom else const.NUMBER_OF_ATOM_TYPES
    if M == 0:
        return torch.empty(0, dtype=torch.int32, device=dev)
    types = types.to(device=dev, dtype=torch.int64).reshape(M)
    known = (types >= 0) & (types < nf)
    one_hot = torch.nn.functional.one_hot(types.clamp(0, nf - 1), nf).to(torch.float32)
    return interaction_types(one_hot[None], positions.reshape(1, M, 3), known.to(torch.int32)[None], is_geom).xs_type[0]


def analyze_interactions(one_hot, x, query_mask, ligand_mask, target_mask=None, protein=None, is_geom=True,
                         margins=const.MARGINS_EDM):
    """Contacts of generated atoms with the protein: the empirical intermolecular terms of Trott & Olson (AutoDock Vina, J.
    Comput. Chem. 2010) for every molecule of a batch, in two launches on the HIP device (``dl_interaction_types``, then
    ``dl_interaction_scores``, ``csrc/interaction.hip``).

    THE RULE (this project's own after that published functional form).  QUERY atoms are the rows of ``query_mask`` (the
    generated atoms); they are typed in the context of the whole ligand, the rows of ``ligand_mask`` (group 1; query rows
    belong to it whatever ``ligand_mask`` says).  TARGET atoms are the rows of ``target_mask`` that are no query rows (the
    batch's ``pocket_mask``; typed among themselves as group 2 - a row in both masks is a ligand row) and the atoms of
    ``protein = (positions [M,3], types [M], xs_types [M])``, a list shared by all molecules, in the frame of ``x``, typed
    once by ``protein_types``.  Masks are ``[B,N]`` or ``[B,N,1]``.  The typing is ``interaction_types``'s.  For a query atom
    ``a`` and a target atom ``b``, in fp64 without fused multiply-adds from the fp32 coordinates: the pair counts when
    ``d2 < 64`` (8 A, strict); ``s = sqrt(d2) - (R[a] + R[b])`` with ``const.XS_RADII``;
    ``gauss1 = exp(-(s / 0.5)^2)``, ``gauss2 = exp(-((s - 3) / 2)^2)``, ``repulsion = s^2`` when ``s < 0``,
    ``hydrophobic`` (both atoms HYDROPHOBIC) 1 below ``s = 0.5`` falling to 0 at 1.5, ``hbond`` (a donor facing an acceptor)
    1 below ``s = -0.7`` falling to 0 at 0.  Every pair term is rounded to a 64-bit fixed point with 32 fractional bits and
    all sums are integer sums: the same bits on every run.

    Returns an ``Interactions`` of device tensors: ``n_query``, ``n_target``, ``n_pairs`` (inside the cut), ``n_hbonds``,
    ``n_hydrophobic`` (int32 ``[B]``), ``terms`` (int64 ``[B,5]`` fixed point: gauss1, gauss2, repulsion, hydrophobic, hbond),
    ``status`` (int32 ``[B]``: ``_lib.DL_INTERACT_*`` bits; with ``NONFINITE``, ``TOO_LARGE`` - more than 1024 query atoms -
    or ``UNTYPED`` everything else is 0), ``atom_terms`` (int64 ``[B,N,5]``, 0 on non-query rows), ``xs_type`` and
    ``type_status`` of the typing launch and the ``query_mask`` it was given.  ``interactions_to_host`` forms the weighted
    score.  No host synchronisation.

    What this is NOT: AutoDock Vina's numbers.  No hydrogens, no PDBQT typing, no search or pose optimisation, no
    intramolecular term and no rotor normalisation (the published rotor weight is not used)."""
    shared = () if protein is None else tuple(protein)
    _lib.require_device('analyze_interactions', one_hot=one_hot, x=x, query_mask=query_mask, ligand_mask=ligand_mask,
                        target_mask=target_mask, **{f'protein[{k}]': t for k, t in enumerate(shared)})
    if one_hot.dim() != 3:
        raise ValueError(f'one_hot {tuple(one_hot.shape)} is not [B,N,nf]')
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in (query_mask, ligand_mask)) or \
            (target_mask is not None and target_mask.numel() != B * N):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, query_mask '
                         f'{tuple(query_mask.shape)}, ligand_mask {tuple(ligand_mask.shape)}')
    if protein is not None and len(shared) != 3:
        raise ValueError(f'protein is (positions, types, xs_types): got {len(shared)} members')
    dev = one_hot.device
    radius = const.xs_radius_table(is_geom).to(dev)
    if radius.numel() != nf:
        raise ValueError(f'{nf} atom types in one_hot, {radius.numel()} in the vocabulary')
    f32 = partial(_lib.dense, device=dev, dtype=torch.float32)
    one_hot, x, qm = f32(one_hot), f32(x), f32(query_mask).reshape(B, N)
    lig = (f32(ligand_mask).reshape(B, N) != 0) | (qm != 0)
    tm = None if target_mask is None else f32(target_mask).reshape(B, N)
    M, px, pxs = 0, None, None
    if protein is not None:
        px, pxs = f32(shared[0]), _lib.dense(shared[2], dev, torch.int32)
        M = pxs.numel()
        if px.shape != (M, 3) or shared[1].numel() != M:
            raise ValueError(f'shapes disagree: protein positions {tuple(px.shape)}, types {tuple(shared[1].shape)}, xs_types '
                             f'{tuple(pxs.shape)}')
    group = lig.to(torch.int32)
    if tm is not None:
        group = group + 2 * ((tm != 0) & ~lig).to(torch.int32)
    i32 = partial(_lib.empty_i32, dev)
    if N == 0:
        zero = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        return Interactions(zero(B), zero(B), zero(B), zero(B), zero(B), torch.zeros((B, 5), dtype=torch.int64, device=dev),
                            zero(B), torch.zeros((B, 0, 5), dtype=torch.int64, device=dev), i32(B, 0), zero(B), qm)
    typed = interaction_types(one_hot, x, group, is_geom, margins)
    out = Interactions(i32(B), i32(B), i32(B), i32(B), i32(B), torch.empty((B, 5), dtype=torch.int64, device=dev), i32(B),
                       torch.empty((B, N, 5), dtype=torch.int64, device=dev), typed.xs_type, typed.status, qm)
    args = _lib.DLInteractArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), xs_type=typed.xs_type.data_ptr(), query_mask=qm.data_ptr(),
        target_mask=_lib.ptr(tm), M=M, target_x=px.data_ptr() if M else None,
        target_xs=pxs.data_ptr() if M else None, radius=radius.data_ptr(),
        n_query=out.n_query.data_ptr(), n_target=out.n_target.data_ptr(), n_pairs=out.n_pairs.data_ptr(),
        n_hbonds=out.n_hbonds.data_ptr(), n_hydrophobic=out.n_hydrophobic.data_ptr(), terms=out.terms.data_ptr(),
        status=out.status.data_ptr(), atom_terms=out.atom_terms.data_ptr())
    _lib.launch('dl_interaction_scores', args, dev)
    return out


def interaction_score(terms):
    """The weighted score of five fixed-point term sums, in fp64: ``sum(w_k * terms_k) / 2^32`` with
    ``const.INTERACTION_WEIGHTS``, the terms taken in order.  Negative is favourable."""
    total = 0.0
    for w, t in zip(const.INTERACTION_WEIGHTS, terms):
        total += w * float(t)
    return total / FIXED_ONE


def interactions_to_host(result):
    """The ``InteractionRecord`` values ``compute_interactions`` reads, one per molecule of an ``Interactions``, on the host:
    the counts as ints, ``terms`` as the five fixed-point integers, ``score`` (``interaction_score`` of them), ``status``, and
    ``atom_scores``: the weighted score of every QUERY atom, in row order."""
    cols = [getattr(result, name).cpu().tolist() for name in ('n_query', 'n_target', 'n_pairs', 'n_hbonds', 'n_hydrophobic')]
    terms, status = result.terms.cpu().tolist(), result.status.cpu().tolist()
    rows = result.query_mask.cpu() != 0
    atom = result.atom_terms.cpu()
    return [InteractionRecord(cols[0][b], cols[1][b], cols[2][b], cols[3][b], cols[4][b], terms[b], interaction_score(terms[b]),
                              status[b], [interaction_score(t) for t in atom[b][rows[b]].tolist()])
            for b in range(len(status))]


def _interaction_scored(record):
    return not record.status & (_lib.DL_INTERACT_NONFINITE | _lib.DL_INTERACT_TOO_LARGE | _lib.DL_INTERACT_UNTYPED)


def compute_interactions(pred, true=None):
    """Scores of the ``InteractionRecord`` values ``pred`` (``interactions_to_host``), plain numbers:

    ``interaction_molecules``               records scored: the flagged ones (``DL_INTERACT_NONFINITE`` / ``TOO_LARGE`` /
                                            ``UNTYPED``: their sums mean nothing) are left out of everything below
    ``interaction_flagged``                 how many were left out
    ``interaction_score``                   mean weighted sum (negative is favourable)
    ``interaction_gauss1`` ... ``_hbond``   mean raw terms, unweighted
    ``hbonds_per_molecule``                 mean number of pairs with a hydrogen-bond term above 0
    ``hydrophobic_contacts_per_molecule``   mean number of pairs with a hydrophobic term above 0
    ``interaction_score_per_atom``          the weighted sums over the query atoms, both summed over the scored records

    With ``true`` - one record per prediction: the data set's own linker scored in the same pocket - three more keys, over the
    positions where both records are scored: ``true_interaction_score``, ``true_hbonds_per_molecule`` and
    ``interaction_excess`` (the mean of ``pred - true`` weighted sums: positive means the sample binds worse under this rule).
    Without ``true`` they are absent.  Nothing scored: every mean is 0."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    good = [m for m in pred if _interaction_scored(m)]
    n = len(good)
    mean = lambda values: float(sum(values) / len(values)) if values else 0.0      # noqa: E731
    queries = sum(m.n_query for m in good)
    out = {'interaction_molecules': n, 'interaction_flagged': len(pred) - n, 'interaction_score': mean([m.score for m in good])}
    for k, name in enumerate(INTERACTION_TERMS):
        out[f'interaction_{name}'] = mean([m.terms[k] / FIXED_ONE for m in good])
    out['hbonds_per_molecule'] = mean([m.n_hbonds for m in good])
    out['hydrophobic_contacts_per_molecule'] = mean([m.n_hydrophobic for m in good])
    out['interaction_score_per_atom'] = float(sum(m.score for m in good) / queries) if queries else 0.0
    if true is not None:
        both = [(p, t) for p, t in zip(pred, true) if _interaction_scored(p) and _interaction_scored(t)]
        out['true_interaction_score'] = mean([t.score for _, t in both])
        out['true_hbonds_per_molecule'] = mean([t.n_hbonds for _, t in both])
        out['interaction_excess'] = mean([p.score - t.score for p, t in both])
    return out


Shapes = namedtuple('Shapes', 'vol_a vol_b vol_min core_a core_b core_both n_a n_b status')
ShapeRecord = namedtuple('ShapeRecord', Shapes._fields)
SHAPE_NAMES = ('shape_molecules', 'shape_flagged', 'shape_similarity', 'shape_tanimoto', 'shape_similarity_7',
               'shape_similarity_8', 'shape_similarity_9')
SHAPE_R2_MAX = 400.0                             # the largest squared radius dl_shape_scores admits: 20 A


def analyze_shapes(one_hot_a, x_a, mask_a, one_hot_b, x_b, mask_b, is_geom=True, scale=0.8, step=0.25):
    """Gridded van der Waals overlap of molecule A and molecule B of every pair of a batch, in the frame the two share, in
    one launch of ``dl_shape_scores`` on the HIP device.

    THE RULE (this project's own.  Spacing, scale and layering follow RDKit's shape encoding - ``gridSpacing`` 0.5,
    ``vdwScale`` 0.8, ``stepSize`` 0.25, two bits per point, heavy atoms only - but the grid is not RDKit's and neither are
    the numbers).  A row takes part when its mask (``[B,N]`` or ``[B,N,1]``) is non-zero; its type is the first largest entry
    of its one-hot row.  Lattice points sit at ``(0.5 i, 0.5 j, 0.5 k)`` for all integers, in the frame of the coordinates.
    With ``r2 = const.shape_radius_table(is_geom, scale, step)`` an atom of type ``t`` gives a point
    ``(d2 < r2[t][0]) + (d2 < r2[t][1]) + (d2 < r2[t][2])``, ``d2 = ((dx*dx) + (dy*dy)) + (dz*dz)`` in fp32 without fused
    multiply-adds, the comparisons strict; a point's LEVEL for a molecule is the maximum over the molecule's atoms: 3 inside
    the scaled van der Waals sphere, 2 and 1 in two layers of ``step`` around it.  ``Na`` and ``Nb`` may differ.

    Returns a ``Shapes`` of int32 device tensors ``[B]``: ``vol_a`` / ``vol_b`` (sum of the levels), ``vol_min`` (sum of
    ``min(level_A, level_B)``), ``core_a`` / ``core_b`` / ``core_both`` (points at level 3), ``n_a`` / ``n_b`` (rows that took
    part) and ``status``: 0, or one of ``_lib.DL_SHAPE_NONFINITE`` (a participating coordinate is NaN or infinite),
    ``DL_SHAPE_OUT_OF_RANGE`` (beyond 4096 A), ``DL_SHAPE_TOO_LARGE`` (the pair spans more than 120 A), decided in this
    order; a flagged pair has every other output 0.  No host synchronisation.

    What this is NOT: no alignment (the molecules are compared where they are), no pharmacophore features (the other half
    of SC-RDKit is ``analyze_pharmacophores``), no hydrogens, not RDKit's numbers.  The lattice is fixed in space: a common shift of both molecules by
    less than the spacing moves the counts a little."""
    _lib.require_device('analyze_shapes', one_hot_a=one_hot_a, x_a=x_a, mask_a=mask_a, one_hot_b=one_hot_b, x_b=x_b,
                        mask_b=mask_b)
    B, Na, nf = one_hot_a.shape
    Nb = one_hot_b.shape[1]
    if (one_hot_b.shape != (B, Nb, nf) or x_a.shape != (B, Na, 3) or x_b.shape != (B, Nb, 3) or mask_a.numel() != B * Na
            or mask_b.numel() != B * Nb):
        raise ValueError(f'shapes disagree: one_hot_a {tuple(one_hot_a.shape)}, x_a {tuple(x_a.shape)}, mask_a '
                         f'{tuple(mask_a.shape)}, one_hot_b {tuple(one_hot_b.shape)}, x_b {tuple(x_b.shape)}, mask_b '
                         f'{tuple(mask_b.shape)}')
    r2 = const.shape_radius_table(is_geom, scale, step)
    if r2.shape != (nf, 3):
        raise ValueError(f'radius table {tuple(r2.shape)} for {nf} atom types')
    if not bool((torch.isfinite(r2) & (r2 <= SHAPE_R2_MAX)).all()):
        raise ValueError(f'scale {scale} and step {step} give a radius that is not finite or is above 20 A')
    dev = one_hot_a.device
    f32 = partial(_lib.dense, device=dev, dtype=torch.float32)
    one_hot_a, x_a, ma = f32(one_hot_a), f32(x_a), f32(mask_a).reshape(B, Na)
    one_hot_b, x_b, mb = f32(one_hot_b), f32(x_b), f32(mask_b).reshape(B, Nb)
    r2 = r2.to(dev).contiguous()
    out = Shapes(*(_lib.empty_i32(dev, B) for _ in Shapes._fields))
    args = _lib.DLShapeArgs(B=B, Na=Na, Nb=Nb, nf=nf, x_a=x_a.data_ptr(), one_hot_a=one_hot_a.data_ptr(), mask_a=ma.data_ptr(),
                            x_b=x_b.data_ptr(), one_hot_b=one_hot_b.data_ptr(), mask_b=mb.data_ptr(), r2=r2.data_ptr(),
                            **{name: getattr(out, name).data_ptr() for name in Shapes._fields})
    _lib.launch('dl_shape_scores', args, dev)
    return out


def shapes_to_host(result):
    """One ``ShapeRecord`` of plain ints per pair of a ``Shapes``, on the host."""
    cols = [getattr(result, name).cpu().tolist() for name in Shapes._fields]
    return [ShapeRecord(*row) for row in zip(*cols)]


def _shape_scored(record):
    return record.status == 0 and record.vol_a > 0


def _tanimoto(record):
    return record.vol_min / (record.vol_a + record.vol_b - record.vol_min)


def compute_shapes(records, linker_records=None, pred=None):
    """Scores of the ``ShapeRecord`` values ``records`` (``shapes_to_host``; A the sample, B its true molecule), in fp64:

    ``shape_molecules``         pairs scored: unflagged, with ``vol_a > 0``; the others are left out of everything below
    ``shape_flagged``           pairs with a status flag
    ``shape_similarity``        mean of ``vol_min / vol_a``: the share of the sample's gridded volume that lies inside the true
                                molecule's, 1 - the protrude distance - the term SC-RDKit weighs by 0.5, on this project's grid
    ``shape_tanimoto``          mean of ``vol_min / (vol_a + vol_b - vol_min)``
    ``shape_similarity_7/8/9``  percent of the scored pairs with ``shape_similarity`` above 0.7 / 0.8 / 0.9, as the reference
                                reports SC-RDKit

    With ``linker_records`` (the same pairs scored over their linker rows only) ``shape_tanimoto_linker``, the mean over those
    records.  With ``pred`` (the ``to_host`` records of ``analyze`` for the same samples) ``shape_tanimoto_valid``, the mean
    over the samples that are valid and in one piece.  A mean or a percentage over nothing is ``None``, as ``rmsd`` is."""
    if pred is not None and len(pred) != len(records):
        raise ValueError(f'{len(records)} shape records, {len(pred)} molecules')
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in records if _shape_scored(m)]
    similarity = [m.vol_min / m.vol_a for m in good]
    above = lambda bar: 100.0 * sum(v > bar for v in similarity) / len(similarity) if similarity else None   # noqa: E731
    out = {'shape_molecules': len(good), 'shape_flagged': sum(1 for m in records if m.status != 0),
           'shape_similarity': mean(similarity), 'shape_tanimoto': mean([_tanimoto(m) for m in good]),
           'shape_similarity_7': above(0.7), 'shape_similarity_8': above(0.8), 'shape_similarity_9': above(0.9)}
    if linker_records is not None:
        out['shape_tanimoto_linker'] = mean([_tanimoto(m) for m in linker_records if _shape_scored(m)])
    if pred is not None:
        out['shape_tanimoto_valid'] = mean([_tanimoto(m) for m, mol in zip(records, pred) if _shape_scored(m) and _good(mol)])
    return out


Rings = namedtuple('Rings', 'n_atoms n_bonds n_components n_rings bond_ring atom_ring ring_hist status bonds')
RingRecord = namedtuple('RingRecord', 'n_rings n_rings_ligand marked_hist status')
RING_NAMES = ('ring_molecules', 'ring_flagged', 'rings_n', 'rings_n_ligand', 'ring_free', 'small_ring', 'macrocycle',
              'ring_bonds_3', 'ring_bonds_4', 'ring_bonds_5', 'ring_bonds_6', 'ring_bonds_7', 'ring_bonds_8plus')


def ring_scores(node_mask, found, drop_mask=None, mark_mask=None):
    """``dl_ring_scores`` on the result ``found`` of ``perceive_bonds`` for the same ``node_mask`` (``[B,N]`` or ``[B,N,1]``;
    ``drop_mask`` and ``mark_mask`` alike, by row): device tensors in, a ``Rings`` of int32 device tensors out, no host
    synchronisation.

    THE RULE, over the simple graph of the kept atoms (real rows that ``drop_mask`` leaves) and the distinct bonds between
    them: ``n_atoms``, ``n_bonds``, ``n_components`` ``[B]``; ``n_rings = n_bonds - n_atoms + n_components`` ``[B]``, the
    cyclomatic number - RDKit's ring count except for cages such as cubane, where RDKit's symmetrised set has more;
    ``bond_ring [B,capacity]``: for every list entry that is a kept bond the number of atoms of the smallest ring through
    it, 0 for a bridge and for every other entry; ``atom_ring [B,N]`` by atom number (the k-th real row is atom k): the
    smallest ring the atom lies in, 0 for none, for dropped atoms and from the atom count on; ``ring_hist [B,2,7]``: the kept
    bonds by smallest ring (bin 0 none, bins 1-5 rings of 3-7 atoms, bin 6 of 8 or more), row 0 all of them, row 1 those
    with a ``mark_mask`` end (zero without ``mark_mask``); ``status [B]``: the ``_lib.DL_BONDS_*`` bits of ``found``,
    ``DL_RINGS_BAD_BOND`` and ``DL_RINGS_TOO_LARGE`` (more than 256 kept atoms: everything but ``n_atoms`` is 0); ``bonds``
    is ``found``."""
    masks = (node_mask,) + tuple(m for m in (drop_mask, mark_mask) if m is not None)
    _lib.require_device('ring_scores', node_mask=node_mask, drop_mask=drop_mask, mark_mask=mark_mask, bonds=found.bonds)
    B = found.n_bonds.shape[0]
    if node_mask.numel() % max(B, 1) or (B == 0 and node_mask.dim() < 2):
        raise ValueError(f'shapes disagree: node_mask {tuple(node_mask.shape)}, {B} bond lists')
    N = node_mask.numel() // B if B else node_mask.shape[1]
    if any(m.numel() != B * N for m in masks) or found.bonds.dim() != 3 or found.bonds.shape[0] != B:
        raise ValueError(f'shapes disagree: masks {[tuple(m.shape) for m in masks]}, bonds {tuple(found.bonds.shape)}')
    dev = node_mask.device
    node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32) for t in (node_mask, drop_mask, mark_mask))
    capacity = found.bonds.shape[1]
    i32 = partial(_lib.empty_i32, dev)
    out = Rings(i32(B), i32(B), i32(B), i32(B), i32(B, capacity), i32(B, N), i32(B, 2, _lib.DL_RING_BINS), i32(B), found)
    found = normalize_bonds(found, B, dev, 'ring_scores')
    args = _lib.DLRingsArgs(
        B=B, N=N, node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask), mark_mask=_lib.ptr(mark_mask), capacity=capacity,
        n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if capacity else None,
        status_in=found.status.data_ptr(), n_atoms=out.n_atoms.data_ptr(), n_bonds=out.n_bonds.data_ptr(),
        n_components=out.n_components.data_ptr(), n_rings=out.n_rings.data_ptr(),
        bond_ring=out.bond_ring.data_ptr() if capacity else None, atom_ring=out.atom_ring.data_ptr(),
        ring_hist=out.ring_hist.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_ring_scores', args, dev)
    return out


def analyze_rings(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM):
    """Rings of every molecule of a batch on the HIP device, in two views of ONE bond perception (``perceive_all_bonds``,
    which synchronises; the two ``dl_ring_scores`` launches do not): ``(ligand, linker)``, both ``Rings``.

    ``ligand``  the molecule without the ``drop_mask`` rows (the pocket of a pocket model), the ``linker_mask`` rows marked:
                row 1 of its ``ring_hist`` holds the rings that linker bonds take part in, those closed through a fragment
                included
    ``linker``  everything that is not a linker row dropped: the linker as a molecule of its own, as the reference takes it
                for ``rings_n`` (compute_metrics.py:128-145).  A ring closed through a fragment atom is absent here."""
    _lib.require_device('analyze_rings', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    linker = linker_mask.reshape(B, N).to(torch.float32)
    ligand = ring_scores(node_mask, found, drop_mask, linker)
    return ligand, ring_scores(node_mask, found, (linker == 0).to(torch.float32))


def rings_to_host(ligand, linker):
    """One ``RingRecord`` of plain values per molecule of the two views ``analyze_rings`` returns: ``n_rings`` of the linker
    view, ``n_rings_ligand``, ``marked_hist`` (row 1 of the ligand view's ``ring_hist``: the linker's bonds by smallest ring)
    and ``status``, the bits of both views."""
    rings, rings_ligand = linker.n_rings.cpu().tolist(), ligand.n_rings.cpu().tolist()
    marked = ligand.ring_hist[:, 1].cpu().tolist()
    status = (ligand.status | linker.status).cpu().tolist()
    return [RingRecord(*row) for row in zip(rings, rings_ligand, marked, status)]


def _ring_scored(record):
    return not record.status & ~_lib.DL_BONDS_NONFINITE


def compute_rings(pred, true=None):
    """Scores of the ``RingRecord`` values ``pred`` (``rings_to_host``), in fp64:

    ``ring_molecules``    records scored; those with any status bit other than ``DL_BONDS_NONFINITE`` (a cut list, an entry
                          that is no bond, more than 256 atoms) are left out of everything below
    ``ring_flagged``      how many were left out
    ``rings_n``           mean number of rings of the linker taken as a molecule of its own - the reference's column; the
                          cyclomatic number, which is RDKit's count except for cages
    ``rings_n_ligand``    the same over the whole ligand
    ``ring_free``         share of the scored records whose linker has no ring
    ``small_ring``        share with a linker bond in a three- or four-membered ring of the ligand
    ``macrocycle``        share with a linker bond whose smallest ring in the ligand has 8 or more atoms
    ``ring_bonds_3`` ... ``ring_bonds_7``, ``ring_bonds_8plus``
                          the linker bonds that lie in a ring, summed over the scored records, split by the size of their
                          smallest ring: shares that add up to 1

    With ``true`` - one record per prediction, the data set's own molecule - over the positions where both are scored:
    ``true_rings_n`` and ``rings_n_match``, the share of samples whose linker has as many rings as the data set's linker.
    Shares are in [0, 1]; a mean or a share over nothing is ``None``, as in ``compute_shapes``."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in pred if _ring_scored(m)]
    bins = [sum(m.marked_hist[k] for m in good) for k in range(_lib.DL_RING_BINS)]
    in_rings = sum(bins[1:])
    out = {'ring_molecules': len(good), 'ring_flagged': len(pred) - len(good),
           'rings_n': mean([m.n_rings for m in good]), 'rings_n_ligand': mean([m.n_rings_ligand for m in good]),
           'ring_free': mean([m.n_rings == 0 for m in good]),
           'small_ring': mean([m.marked_hist[1] + m.marked_hist[2] > 0 for m in good]),
           'macrocycle': mean([m.marked_hist[_lib.DL_RING_BINS - 1] > 0 for m in good])}
    for k, name in enumerate(RING_NAMES[7:], start=1):
        out[name] = float(bins[k] / in_rings) if in_rings else None
    if true is not None:
        both = [(p, t) for p, t in zip(pred, true) if _ring_scored(p) and _ring_scored(t)]
        out['true_rings_n'] = mean([t.n_rings for _, t in both])
        out['rings_n_match'] = mean([p.n_rings == t.n_rings for p, t in both])
    return out


AromaticScores = namedtuple('AromaticScores', 'n_aromatic_linker n_aromatic n_planar n_filtered_bonds n_over status refined '
                                              'aromatic')
AromaticRecord = namedtuple('AromaticRecord', 'n_aromatic_linker n_aromatic n_planar n_filtered_bonds n_over status')
AROMATIC_NAMES = ('aromatic_molecules', 'aromatic_flagged', 'aromatic_rings_n', 'ring_filter', 'valence_validity_geometric')


def analyze_aromatic(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM, planarity=0.1,
                     substituent=0.5):
    """Aromatic rings and geometric bond orders of every molecule of a batch on the HIP device: ONE bond perception
    (``perceive_all_bonds``, which synchronises), then three launches that do not - ``refine_bond_orders`` with the
    ``linker_mask`` rows marked, ``ring_scores`` on the same list and ``molecule_keys`` on the refined one - and device tensor
    operations that combine them.  ``drop_mask`` rows (the pocket of a pocket model) are left out of all three.

    Returns an ``AromaticScores`` of device tensors ``[B]``: ``n_aromatic_linker`` (aromatic rings all of whose atoms are
    linker rows), ``n_aromatic``, ``n_planar``; ``n_filtered_bonds``, the bonds of new order 2 that lie in a ring
    (``bond_ring > 0``) and are not aromatic - what the reference's ring filter rejects; ``n_over``, the atoms over their
    valence limit with the new orders; ``status``, the bits of all three launches; and ``refined`` / ``aromatic`` as
    ``refine_bond_orders`` returns them.  Aromaticity is this project's own geometric rule, not RDKit's or OpenBabel's."""
    _lib.require_device('analyze_aromatic', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    linker = linker_mask.reshape(B, N).to(torch.float32)
    refined, aromatic = refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask, linker, planarity, substituent)
    rings = ring_scores(node_mask, found, drop_mask)
    keys = molecule_keys(one_hot, node_mask, refined, is_geom, drop_mask)
    filtered = (refined.bonds[:, :, 2] == 2) & (rings.bond_ring > 0) & (aromatic.bond_aromatic == 0)
    return AromaticScores(aromatic.n_aromatic_marked, aromatic.n_aromatic_rings, aromatic.n_planar_rings,
                          filtered.sum(dim=1).to(torch.int32), keys.n_over, aromatic.status | rings.status | keys.status,
                          refined, aromatic)


def aromatic_to_host(result):
    """One ``AromaticRecord`` of plain values per molecule of an ``AromaticScores``."""
    columns = [getattr(result, name).cpu().tolist() for name in AromaticRecord._fields]
    return [AromaticRecord(*row) for row in zip(*columns)]


def _aromatic_scored(record):
    return not record.status & ~_lib.DL_BONDS_NONFINITE


def compute_aromatic(pred, true=None):
    """Scores of the ``AromaticRecord`` values ``pred`` (``aromatic_to_host``), in fp64:

    ``aromatic_molecules``          records scored; those with any status bit other than ``DL_BONDS_NONFINITE`` (a cut list, an
                                    entry that is no bond, more than 256 atoms, more than 64 planar rings, a ring system of
                                    more than 32 atoms) are left out of everything below
    ``aromatic_flagged``            how many were left out
    ``aromatic_rings_n``            mean number of aromatic rings that lie wholly in the linker
    ``ring_filter``                 share of the scored records with no double bond inside a ring that is not aromatic - the
                                    reference's 2D ring filter (compute_metrics.py:269-277) on this project's aromaticity
    ``valence_validity_geometric``  share with no atom over its valence limit under the geometric bond orders

    With ``true`` - one record per prediction, the data set's own molecule - over the positions where both are scored:
    ``true_aromatic_rings_n``, ``true_ring_filter`` and ``true_valence_validity_geometric``.  A mean or a share over nothing
    is ``None``, as in ``compute_rings``.  Aromaticity here is a geometric rule of this project's own, not RDKit's."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in pred if _aromatic_scored(m)]
    out = {'aromatic_molecules': len(good), 'aromatic_flagged': len(pred) - len(good),
           'aromatic_rings_n': mean([m.n_aromatic_linker for m in good]),
           'ring_filter': mean([m.n_filtered_bonds == 0 for m in good]),
           'valence_validity_geometric': mean([m.n_over == 0 for m in good])}
    if true is not None:
        both = [t for p, t in zip(pred, true) if _aromatic_scored(p) and _aromatic_scored(t)]
        out['true_aromatic_rings_n'] = mean([t.n_aromatic_linker for t in both])
        out['true_ring_filter'] = mean([t.n_filtered_bonds == 0 for t in both])
        out['true_valence_validity_geometric'] = mean([t.n_over == 0 for t in both])
    return out


Fingerprints = namedtuple('Fingerprints', 'bits n_on n_atoms n_centres status')
Nearest = namedtuple('Nearest', 'index common union sum_q20 n_pairs')
DiversityRecord = namedtuple('DiversityRecord', 'input status sum_q20 n_pairs sum_q20_linker n_pairs_linker true_common '
                                                'true_union true_common_linker true_union_linker ref_common ref_union')
DIVERSITY_NAMES = ('diversity_molecules', 'internal_diversity', 'internal_diversity_linker')
DIVERSITY_TRUE_NAMES = ('similarity_to_true', 'similarity_to_true_linker')
DIVERSITY_REFERENCE_NAMES = ('nearest_reference_similarity', 'nearest_reference_identical')
Q20 = 1 << 20                                    # the fixed point of dl_tanimoto_args.sum_q20


def fingerprints(one_hot, node_mask, found, drop_mask=None, centre_mask=None, radius=2, n_bits=2048):
    """``dl_fingerprints`` on the result ``found`` of ``perceive_bonds`` (or ``refine_bond_orders``) for the same ``one_hot``
    and ``node_mask``: device tensors in, a ``Fingerprints`` of device tensors out, on torch's current stream, no host
    synchronisation.  It mirrors ``molecule_keys``.

    THE RULE (this project's own; NOT RDKit's Morgan fingerprint: the invariants are the element and the bond orders alone,
    the hash is the one of ``molecule_keys``, duplicate environments are not removed and nothing is counted).  With the
    colours ``c_r`` of ``molecule_keys``' refinement after ``r`` rounds, the on-bits of a molecule are ``c_r[i] mod n_bits``
    for ``0 <= r <= radius`` and every kept atom ``i`` that is a centre; ``centre_mask`` (``[B,N]`` or ``[B,N,1]`` by row,
    like ``drop_mask``) chooses the centres, every kept atom without it.  The environments always see the whole kept molecule.

    ``bits`` int32 ``[B, n_bits / 32]`` (the 32 bits of each word; bit ``k`` of a fingerprint is bit ``k % 32`` of word
    ``k // 32``), ``n_on``, ``n_atoms`` (kept), ``n_centres`` and ``status`` int32 ``[B]``: the ``_lib.DL_BONDS_*`` bits of
    ``found`` plus ``DL_FP_BAD_BOND`` and ``DL_FP_TOO_LARGE`` (more than 256 kept atoms: no bits)."""
    masks = (node_mask,) + tuple(m for m in (drop_mask, centre_mask) if m is not None)
    _lib.require_device('fingerprints', one_hot=one_hot, node_mask=node_mask, drop_mask=drop_mask, centre_mask=centre_mask,
                        n_bonds=found.n_bonds)
    if radius not in range(_lib.DL_FP_MAX_RADIUS + 1) or n_bits not in _lib.DL_FP_BITS:
        raise ValueError(f'radius must be 0..{_lib.DL_FP_MAX_RADIUS} and n_bits one of {_lib.DL_FP_BITS}: got {radius}, {n_bits}')
    B, N, nf = one_hot.shape
    if any(m.numel() != B * N for m in masks) or found.bonds.dim() != 3 or found.bonds.shape[0] != B:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, masks {[tuple(m.shape) for m in masks]}, bonds '
                         f'{tuple(found.bonds.shape)}')
    dev = one_hot.device
    one_hot, node_mask, drop_mask, centre_mask = (_lib.dense(t, dev, torch.float32)
                                                  for t in (one_hot, node_mask, drop_mask, centre_mask))
    i32 = partial(_lib.empty_i32, dev)
    out = Fingerprints(i32(B, n_bits // 32), i32(B), i32(B), i32(B), i32(B))
    found = normalize_bonds(found, B, dev, 'fingerprints')
    capacity = found.bonds.shape[1]
    args = _lib.DLFingerprintArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        centre_mask=_lib.ptr(centre_mask), capacity=capacity, n_bonds_in=found.n_bonds.data_ptr(),
        bonds=found.bonds.data_ptr() if capacity else None, status_in=found.status.data_ptr(), radius=int(radius),
        n_bits=int(n_bits), bits=out.bits.data_ptr(), n_on=out.n_on.data_ptr(), n_atoms=out.n_atoms.data_ptr(),
        n_centres=out.n_centres.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_fingerprints', args, dev)
    return out


def analyze_fingerprints(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM, radius=2,
                         n_bits=2048):
    """Fingerprints of every molecule of a batch on the HIP device, in two views of ONE bond perception
    (``perceive_all_bonds``, which synchronises; the two ``dl_fingerprints`` launches do not): ``(whole, linker)``, both
    ``Fingerprints``.  ``whole`` has every kept atom as a centre; ``linker`` only the ``linker_mask`` rows, whose
    environments still reach into the fragments.  ``drop_mask`` rows (the pocket of a pocket model) are left out of both.
    All samples of one input share their fragments, so ``whole`` mostly measures the fragments; ``linker`` is the one that
    tells the samples of an input apart."""
    _lib.require_device('analyze_fingerprints', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    whole = fingerprints(one_hot, node_mask, found, drop_mask, None, radius, n_bits)
    return whole, fingerprints(one_hot, node_mask, found, drop_mask, linker_mask.reshape(B, N), radius, n_bits)


def _aligned_rows(rows):
    return rows.clone() if rows.data_ptr() % 16 else rows


def tanimoto_nearest(a_bits, b_bits, a_offsets=None, b_offsets=None, exclude_diagonal=False, want_sum=True):
    """``dl_tanimoto_nearest``: for every row of ``a_bits [Ma,W]`` its nearest neighbour and its summed similarity among the
    candidate rows of ``b_bits [Mb,W]`` (``Fingerprints.bits``: int32 words, any other dtype is refused with a ``ValueError``; any
    strides and offset; the two may be the same tensor), on torch's current stream
    with no host synchronisation.  ``a_offsets`` and ``b_offsets`` (int32 ``[G+1]``, both or neither; ``a_offsets`` must not
    decrease) split the rows into ``G`` groups: row ``i`` with ``a_offsets[g] <= i < a_offsets[g+1]`` has the candidates
    ``b_offsets[g] <= j < b_offsets[g+1]``, without ``j == i`` when ``exclude_diagonal``.  Without offsets: one group over
    everything.

    The similarity of a pair is Tanimoto on THIS PROJECT'S fingerprint (not RDKit's): ``c / u`` with ``c = popcount(a & b)``
    and ``u = popcount(a | b)``, and 1 when both are empty.  Returns a ``Nearest`` of device tensors ``[Ma]``: ``index`` (the
    candidate of the greatest similarity, compared exactly; of equal ones the lowest; -1 without candidates), ``common`` and
    ``union`` (that pair's ``c`` and ``u``), ``sum_q20`` (int64: the sum over the candidates of ``floor(c * 2**20 / u)``, or
    ``None`` without ``want_sum``) and ``n_pairs`` (candidates).  All integers: the same bits on every run."""
    _lib.require_device('tanimoto_nearest', a_bits=a_bits, b_bits=b_bits, a_offsets=a_offsets, b_offsets=b_offsets)
    if a_bits.dim() != 2 or b_bits.dim() != 2 or a_bits.shape[1] != b_bits.shape[1] or a_bits.shape[1] * 32 not in _lib.DL_FP_BITS:
        raise ValueError(f'shapes disagree: a_bits {tuple(a_bits.shape)}, b_bits {tuple(b_bits.shape)}')
    if a_bits.dtype != torch.int32 or b_bits.dtype != torch.int32:
        raise ValueError(f'fingerprint rows are int32 words, got {a_bits.dtype} and {b_bits.dtype}')
    if (a_offsets is None) != (b_offsets is None) or (a_offsets is not None and a_offsets.numel() != b_offsets.numel()):
        raise ValueError('a_offsets and b_offsets come together and have the same length')
    dev = a_bits.device
    Ma, W = a_bits.shape
    Mb = b_bits.shape[0]
    # the kernel reads the rows 16 bytes at a time and the C entry point refuses a pointer that is not aligned to that (a row
    # slice of a larger set is aligned to 4): such rows are handed over as an aligned copy
    same = b_bits is a_bits
    a_bits = _aligned_rows(a_bits.contiguous())
    b_bits = a_bits if same else _aligned_rows(b_bits.contiguous())
    if a_offsets is None:
        a_offsets, b_offsets = (torch.full((2,), m, dtype=torch.int32, device=dev) for m in (Ma, Mb))     # [0, M], filled on
        a_offsets[0], b_offsets[0] = 0, 0                                                                  # the device
    a_offsets, b_offsets = (_lib.dense(t, dev, torch.int32) for t in (a_offsets, b_offsets))
    G = max(a_offsets.numel() - 1, 0)
    i32 = partial(_lib.empty_i32, dev, Ma)
    out = Nearest(i32(), i32(), i32(), torch.empty(Ma, dtype=torch.int64, device=dev) if want_sum else None, i32())
    args = _lib.DLTanimotoArgs(
        Ma=Ma, Mb=Mb, W=W, G=G, a_bits=a_bits.data_ptr() if Ma else None, b_bits=b_bits.data_ptr() if Mb else None,
        a_offsets=a_offsets.data_ptr() if G else None, b_offsets=b_offsets.data_ptr() if G else None,
        exclude_diagonal=int(bool(exclude_diagonal)), nn_index=out.index.data_ptr(), nn_common=out.common.data_ptr(),
        nn_union=out.union.data_ptr(), n_pairs=out.n_pairs.data_ptr(), sum_q20=_lib.ptr(out.sum_q20))
    _lib.launch('dl_tanimoto_nearest', args, dev)
    return out


def _grouped(rows, groups, n_groups):
    """``rows`` (int64 positions) sorted by their group, and the int32 offsets ``[n_groups + 1]`` of the groups."""
    order = torch.argsort(groups[rows], stable=True)
    counts = torch.bincount(groups[rows], minlength=n_groups)
    offsets = torch.zeros(n_groups + 1, dtype=torch.int64, device=rows.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return rows[order], offsets.to(torch.int32)


def diversity_records(whole, linker, input_index, true_whole=None, true_linker=None, reference=None):
    """The ``DiversityRecord`` values ``compute_diversity`` reads, one per sample, from fingerprints kept on the device.

    ``whole`` and ``linker`` are the two ``Fingerprints`` of ``analyze_fingerprints`` for ALL samples (batches concatenated
    with ``cat_fingerprints``); ``input_index[k]`` names the input sample ``k`` came from.  With ``true_whole`` /
    ``true_linker`` (the same for the true molecules, one row per DISTINCT input, in order of first appearance in
    ``input_index``) every sample is also compared with its own true molecule; with ``reference`` (int32 bits ``[R,W]`` of
    a reference set, clean rows only) with its nearest row there.  A sample or true molecule with a status bit in either
    view takes part in no comparison.  Launches: two for the pairs among the samples of each input (groups = inputs,
    diagonal excluded), two against the true molecules (B groups of one row), one against the reference (one group)."""
    n = whole.bits.shape[0]
    if not (linker.bits.shape[0] == n == len(input_index)):
        raise ValueError(f'{n} and {linker.bits.shape[0]} fingerprints, {len(input_index)} input indices')
    dev = whole.bits.device
    dense = {}
    groups_host = [dense.setdefault(v, len(dense)) for v in input_index]
    G = len(dense)
    status = (whole.status | linker.status)
    zeros = lambda: torch.zeros(n, dtype=torch.int64, device=dev)           # noqa: E731
    cols = {name: zeros() for name in DiversityRecord._fields[2:]}
    if n:
        groups = torch.tensor(groups_host, dtype=torch.int64, device=dev)
        rows, offsets = _grouped(torch.nonzero(status == 0).reshape(-1), groups, G)
        for view, tail in ((whole, ''), (linker, '_linker')):
            bits = view.bits[rows].contiguous()
            near = tanimoto_nearest(bits, bits, offsets, offsets, exclude_diagonal=True)
            cols['sum_q20' + tail][rows], cols['n_pairs' + tail][rows] = near.sum_q20, near.n_pairs.long()
        if true_whole is not None:
            if true_whole.bits.shape[0] != G or true_linker.bits.shape[0] != G:
                raise ValueError(f'{G} inputs, {true_whole.bits.shape[0]} and {true_linker.bits.shape[0]} true fingerprints')
            clean = (true_whole.status | true_linker.status) == 0
            b_offsets = torch.zeros(G + 1, dtype=torch.int64, device=dev)
            b_offsets[1:] = torch.cumsum(clean.long(), 0)                   # a flagged true molecule: an empty range
            b_offsets = b_offsets.to(torch.int32)
            for view, true_view, tail in ((whole, true_whole, ''), (linker, true_linker, '_linker')):
                near = tanimoto_nearest(view.bits[rows].contiguous(), true_view.bits[clean].contiguous(), offsets, b_offsets,
                                        want_sum=False)
                has = near.index >= 0
                cols['true_common' + tail][rows] = torch.where(has, near.common, -1).long()
                cols['true_union' + tail][rows] = near.union.long()
        if reference is not None:
            near = tanimoto_nearest(whole.bits[rows].contiguous(), reference, want_sum=False)
            cols['ref_common'][rows] = torch.where(near.index >= 0, near.common, -1).long()
            cols['ref_union'][rows] = near.union.long()
    status = status.cpu().tolist()
    host = {name: t.cpu().tolist() for name, t in cols.items()}
    absent = [name for name in cols if (name.startswith('true_') and true_whole is None)
              or (name.startswith('ref_') and reference is None)]
    out = []
    for k in range(n):
        values = {name: (None if name in absent else host[name][k]) for name in cols}
        for c, u in (('true_common', 'true_union'), ('true_common_linker', 'true_union_linker'), ('ref_common', 'ref_union')):
            if values[c] is not None and (values[c] < 0 or status[k] != 0):  # nothing to compare with
                values[c] = values[u] = None
        out.append(DiversityRecord(input=input_index[k], status=status[k], **values))
    return out


def cat_fingerprints(parts):
    """One ``Fingerprints`` from the ``Fingerprints`` of several batches, rows concatenated on the device."""
    return Fingerprints(*(torch.cat([getattr(p, name) for p in parts]) for name in Fingerprints._fields))


def _similarity(common, union):
    return 1.0 if union == 0 else common / union


def compute_diversity(records, with_true=None, with_reference=None):
    """Set-level scores of the ``DiversityRecord`` values ``records`` (``diversity_records``), on the host, in fp64.  Every
    similarity here is Tanimoto on THIS PROJECT'S circular fingerprint (``fingerprints``), NOT on RDKit's Morgan
    fingerprint: the numbers compare runs of this project with each other and nothing else.

    ``diversity_molecules``           records scored: those with status 0; the others are left out of everything below
    ``internal_diversity``            the mean, over the inputs with at least two scored samples, of ``1 - `` the mean
                                      pairwise similarity among that input's samples (from ``sum_q20 / n_pairs / 2**20``:
                                      every ordered pair once, each similarity rounded down to a multiple of ``2**-20``)
    ``internal_diversity_linker``     the same on the fingerprints whose centres are the linker atoms: the one that tells the
                                      samples of an input apart, since they share their fragments
    ``similarity_to_true``, ``similarity_to_true_linker``
                                      when the records carry them: the mean similarity of every scored sample to its own
                                      true molecule
    ``nearest_reference_similarity``  when the records carry them: the mean of every scored sample's greatest similarity to
                                      the reference set, and
    ``nearest_reference_identical``   the share of those samples with a reference fingerprint equal to their own

    ``with_true`` / ``with_reference`` say whether those keys are wanted; ``None`` (the default): when some record carries
    such a value.  A mean over nothing is ``None``, as in ``compute_rings``."""
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in records if m.status == 0]
    out = {'diversity_molecules': len(good)}
    for tail in ('', '_linker'):
        sums = {}
        for m in good:
            total, pairs = sums.get(m.input, (0, 0))
            sums[m.input] = (total + getattr(m, 'sum_q20' + tail), pairs + getattr(m, 'n_pairs' + tail))
        out['internal_diversity' + tail] = mean([1.0 - total / pairs / Q20 for total, pairs in sums.values() if pairs > 0])
    carried = lambda u: any(getattr(m, u) is not None for m in records)      # noqa: E731
    for name, c, u, wanted in (('similarity_to_true', 'true_common', 'true_union', with_true),
                               ('similarity_to_true_linker', 'true_common_linker', 'true_union_linker', with_true),
                               ('nearest_reference_similarity', 'ref_common', 'ref_union', with_reference)):
        if not (carried(u) if wanted is None else wanted):
            continue
        scored = [(getattr(m, c), getattr(m, u)) for m in good if getattr(m, u) is not None]
        out[name] = mean([_similarity(cc, uu) for cc, uu in scored])
        if name == 'nearest_reference_similarity':
            out['nearest_reference_identical'] = mean([cc == uu for cc, uu in scored])
    return out


Clusters = namedtuple('Clusters', 'cluster centroid n_neighbours n_clusters status num den')
Picks = namedtuple('Picks', 'picks pick_common pick_union n_picked status pick_rank')
SelectRecord = namedtuple('SelectRecord', 'input eligible cluster is_centroid cluster_size n_neighbours pick_rank pick_similarity')
SELECTION_NAMES = ('selection_molecules', 'clusters_per_input', 'cluster_ratio', 'largest_cluster_share')
SELECT_VIEWS = ('linker', 'whole')


def threshold_fraction(threshold):
    """The similarity threshold ``dl_tanimoto_cluster`` compares with, as ``(num, den)``: ``threshold`` (a decimal string, a
    ``Fraction`` or a float) through ``fractions.Fraction(...).limit_denominator(1000)``.  It must lie in (0, 1]."""
    value = Fraction(threshold).limit_denominator(1000)
    if not 0 < value <= 1:
        raise ValueError(f'the similarity threshold must lie in (0, 1], got {threshold!r}')
    return value.numerator, value.denominator


def _fingerprint_set(who, bits, offsets, **more):
    """What the two selection wrappers do with their rows and offsets, as ``tanimoto_nearest`` does: ``(bits, offsets, G)``."""
    _lib.require_device(who, bits=bits, offsets=offsets, **more)
    if bits.dim() != 2 or bits.shape[1] * 32 not in _lib.DL_FP_BITS:
        raise ValueError(f'bits must be [M,W] with W * 32 one of {_lib.DL_FP_BITS}: got {tuple(bits.shape)}')
    if bits.dtype != torch.int32:
        raise ValueError(f'fingerprint rows are int32 words, got {bits.dtype}')
    dev = bits.device
    bits = _aligned_rows(bits.contiguous())      # a row slice of a larger set is aligned to 4 bytes: handed over as a copy
    if offsets is None:
        offsets = torch.full((2,), bits.shape[0], dtype=torch.int32, device=dev)     # [0, M], filled on the device
        offsets[0] = 0
    offsets = _lib.dense(offsets, dev, torch.int32)
    return bits, offsets, max(offsets.numel() - 1, 0)


def tanimoto_clusters(bits, offsets=None, threshold='0.65'):
    """``dl_tanimoto_cluster``: Taylor-Butina sphere-exclusion clusters of every group of the fingerprint rows ``bits [M,W]``
    (``Fingerprints.bits``: int32 words, any other dtype is refused with a ``ValueError``; any strides and offset), on
    torch's current stream with no host synchronisation.  ``offsets`` (int32 ``[G+1]``, not decreasing) splits the rows
    into ``G`` groups of at most 4096 rows; without it: one group over everything.

    THE RULE (this project's own statement after RDKit's ``Butina.ClusterData(reordering=False)``, on THIS PROJECT'S
    fingerprint; NOT promised to reproduce RDKit's output on ties).  With ``num / den = threshold`` (``threshold_fraction``)
    row ``j != i`` of the same group is a neighbour of ``i`` when ``c * den >= num * u`` (``c = popcount(a & b)``,
    ``u = popcount(a | b)``; two empty rows are neighbours).  The rows are walked by their number of neighbours, descending,
    among equals by index; a row not yet assigned becomes the centroid of the next cluster and takes its unassigned
    neighbours.

    Returns a ``Clusters``: ``cluster`` (group-local id), ``centroid`` (row index of the cluster's centroid) and
    ``n_neighbours`` int32 ``[M]``; ``n_clusters`` and ``status`` (``_lib.DL_SELECT_TOO_LARGE``: more than 4096 rows, nothing
    was clustered) int32 ``[G]``; and the ``num`` and ``den`` that were used.  A row of no group, or of a group that is too
    large, has -1, -1 and 0."""
    num, den = threshold_fraction(threshold)
    bits, offsets, G = _fingerprint_set('tanimoto_clusters', bits, offsets)
    dev = bits.device
    M, W = bits.shape
    i32 = partial(_lib.empty_i32, dev)
    out = Clusters(i32(M), i32(M), i32(M), i32(G), i32(G), num, den)
    args = _lib.DLClusterArgs(
        M=M, W=W, G=G, bits=bits.data_ptr() if M else None, offsets=offsets.data_ptr() if G else None, num=num, den=den,
        cluster=out.cluster.data_ptr(), centroid=out.centroid.data_ptr(), n_neighbours=out.n_neighbours.data_ptr(),
        n_clusters=out.n_clusters.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_tanimoto_cluster', args, dev)
    return out


def tanimoto_picks(bits, k, offsets=None, first=None):
    """``dl_tanimoto_pick``: a MaxMin diverse subset of up to ``k`` rows (1 .. 4096) of every group of the fingerprint rows
    ``bits [M,W]``, rows and ``offsets`` as ``tanimoto_clusters`` takes them, on torch's current stream with no host
    synchronisation.  ``first`` (int32 ``[G]``, optional) is the row index of each group's first pick; without it every
    group starts from its lowest row.

    THE RULE (MaxMin with this project's own tie rules on THIS PROJECT'S fingerprint, NOT RDKit's ``MaxMinPicker``).  Every
    unpicked row keeps the greatest similarity to any pick so far (of equal ones the earliest pick's ``c`` and ``u``); the
    next pick is the unpicked row for which that is SMALLEST, fractions compared exactly, of equal ones the lowest row.

    Returns a ``Picks``: ``picks`` (row indices in pick order), ``pick_common`` and ``pick_union`` (the ``c`` and ``u`` of
    the pick's greatest similarity to the picks before it; -1 for the first) int32 ``[G,k]``, all -1 from ``n_picked`` on;
    ``n_picked`` and ``status`` (``_lib.DL_SELECT_TOO_LARGE``; ``_lib.DL_SELECT_BAD_FIRST``: ``first`` outside its group;
    either way nothing was picked) int32 ``[G]``; ``pick_rank`` int32 ``[M]``, the row's position in its group's pick order
    or -1."""
    k = int(k)
    if not 1 <= k <= _lib.DL_SELECT_MAX_ROWS:
        raise ValueError(f'k must be 1..{_lib.DL_SELECT_MAX_ROWS}, got {k}')
    bits, offsets, G = _fingerprint_set('tanimoto_picks', bits, offsets, first=first)
    dev = bits.device
    M, W = bits.shape
    if first is not None:
        if first.numel() != G:
            raise ValueError(f'{G} groups, {first.numel()} first picks')
        first = _lib.dense(first, dev, torch.int32)
    i32 = partial(_lib.empty_i32, dev)
    out = Picks(i32(G, k), i32(G, k), i32(G, k), i32(G), i32(G), i32(M))
    args = _lib.DLPickArgs(
        M=M, W=W, G=G, K=k, bits=bits.data_ptr() if M else None, offsets=offsets.data_ptr() if G else None,
        first=first.data_ptr() if first is not None and G else None, picks=out.picks.data_ptr(),
        pick_common=out.pick_common.data_ptr(), pick_union=out.pick_union.data_ptr(), n_picked=out.n_picked.data_ptr(),
        status=out.status.data_ptr(), pick_rank=out.pick_rank.data_ptr())
    _lib.launch('dl_tanimoto_pick', args, dev)
    return out


def good_molecules(molecules):
    """For every ``Molecule`` of ``to_host``: is it valid under the valence rule, in one piece and clean?  The rule by which
    ``compute_metrics`` counts a prediction, and the gate of ``select_records``."""
    return [_good(m) for m in molecules]


def _typical_rows(bits, offsets, group_of):
    """The most typical row of every group, int32 ``[G]``: the one of the greatest summed similarity to the others of its
    group (``tanimoto_nearest``'s ``sum_q20``), of equal ones the lowest; -1 for an empty group.  No host synchronisation."""
    G = offsets.numel() - 1
    dev = bits.device
    total = tanimoto_nearest(bits, bits, offsets, offsets, exclude_diagonal=True).sum_q20
    most = torch.full((G,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, group_of, total, 'amax')
    position = torch.arange(bits.shape[0], dtype=torch.int64, device=dev)
    nowhere = torch.iinfo(torch.int64).max
    candidate = torch.where(total == most[group_of], position, nowhere)
    first = torch.full((G,), nowhere, dtype=torch.int64, device=dev).scatter_reduce(0, group_of, candidate, 'amin')
    return torch.where(first == nowhere, -1, first).to(torch.int32)


def select_records(whole, linker, input_index, good, view='linker', threshold=None, k=None):
    """The ``SelectRecord`` values ``compute_selection`` and the tools read, one per sample: the clusters
    (``tanimoto_clusters``, with ``threshold``) and the diverse subset (``tanimoto_picks``, with ``k``) of every input's
    samples, from fingerprints kept on the device.

    ``whole`` and ``linker`` are the two ``Fingerprints`` of ``analyze_fingerprints`` for ALL samples (``cat_fingerprints``),
    ``input_index[k]`` names the input sample ``k`` came from and groups are the inputs, as in ``diversity_records``;
    ``view`` says which of the two fingerprints is compared (all samples of an input share their fragments, so ``'whole'``
    mostly measures the fragments).  Only ELIGIBLE samples are grouped: those with fingerprint status 0 in both views and
    ``good[k]`` true (``good_molecules`` of ``to_host``: valid under the valence rule and in one piece).  The gate is part of
    the rule: MaxMin prefers outliers, and a broken molecule is the furthest outlier there is.  An input's first pick is its
    most typical eligible sample: the greatest summed similarity to the others (``tanimoto_nearest`` on the same view), of
    equal ones the lowest.

    A record holds ``input``, ``eligible``, and - ``None`` when not asked for, not eligible, or in an input of more than 4096
    eligible samples - ``cluster`` (the id within its input), ``is_centroid``, ``cluster_size``, ``n_neighbours``,
    ``pick_rank`` (``None`` when not picked) and ``pick_similarity`` (``c / u`` in fp64 of the pick's greatest similarity
    to the picks before it; ``None`` for the first)."""
    n = whole.bits.shape[0]
    if not (linker.bits.shape[0] == n == len(input_index) == len(good)):
        raise ValueError(f'{n} and {linker.bits.shape[0]} fingerprints, {len(input_index)} input indices, {len(good)} flags')
    if view not in SELECT_VIEWS:
        raise ValueError(f'view must be one of {SELECT_VIEWS}, got {view!r}')
    dev = whole.bits.device
    dense = {}
    groups_host = [dense.setdefault(v, len(dense)) for v in input_index]
    G = len(dense)
    fields = {name: [None] * n for name in SelectRecord._fields[2:]}
    eligible = [False] * n
    if n:
        groups = torch.tensor(groups_host, dtype=torch.int64, device=dev)
        clean = ((whole.status | linker.status) == 0) & torch.tensor([bool(v) for v in good], dtype=torch.bool, device=dev)
        rows, offsets = _grouped(torch.nonzero(clean).reshape(-1), groups, G)
        bits = (linker if view == 'linker' else whole).bits[rows].contiguous()
        found = tanimoto_clusters(bits, offsets, threshold) if threshold is not None else None
        picked = tanimoto_picks(bits, min(int(k), _lib.DL_SELECT_MAX_ROWS), offsets,
                                _typical_rows(bits, offsets, groups[rows])) if k is not None else None
        rows = rows.cpu().tolist()               # the first host synchronisation
        for pos in rows:
            eligible[pos] = True
        if found is not None:
            cluster, centroid, n_neighbours = (t.cpu().tolist() for t in (found.cluster, found.centroid, found.n_neighbours))
            sizes = {}
            for at, pos in enumerate(rows):
                if cluster[at] >= 0:
                    sizes[centroid[at]] = sizes.get(centroid[at], 0) + 1
            for at, pos in enumerate(rows):
                if cluster[at] >= 0:
                    fields['cluster'][pos], fields['is_centroid'][pos] = cluster[at], centroid[at] == at
                    fields['cluster_size'][pos], fields['n_neighbours'][pos] = sizes[centroid[at]], n_neighbours[at]
        if picked is not None:
            order, common, union = (t.cpu().tolist() for t in (picked.picks, picked.pick_common, picked.pick_union))
            for g in range(G):
                for rank, at in enumerate(order[g]):
                    if at < 0:
                        break
                    fields['pick_rank'][rows[at]] = rank
                    if rank:
                        fields['pick_similarity'][rows[at]] = _similarity(common[g][rank], union[g][rank])
    return [SelectRecord(input=input_index[pos], eligible=eligible[pos], **{name: v[pos] for name, v in fields.items()})
            for pos in range(n)]


def compute_selection(records):
    """Set-level scores of the ``SelectRecord`` values ``records`` (``select_records`` with a threshold), on the host.  The
    clusters are Taylor-Butina clusters under THIS PROJECT'S rule on THIS PROJECT'S fingerprint, not RDKit's.

    ``selection_molecules``     eligible records: the only ones that were grouped
    ``clusters_per_input``      the mean number of clusters over the inputs with a clustered sample
    ``cluster_ratio``           the mean over those inputs of clusters / clustered samples: 1 when every sample is its own
                                cluster
    ``largest_cluster_share``   the mean over those inputs of the largest cluster's size / clustered samples

    A mean over nothing is ``None``, as in ``compute_diversity``."""
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    sizes = {}
    for m in records:
        if m.eligible and m.cluster is not None:
            of_input = sizes.setdefault(m.input, {})
            of_input[m.cluster] = of_input.get(m.cluster, 0) + 1
    totals = {key: sum(of_input.values()) for key, of_input in sizes.items()}
    return {'selection_molecules': sum(bool(m.eligible) for m in records),
            'clusters_per_input': mean([len(of_input) for of_input in sizes.values()]),
            'cluster_ratio': mean([len(of_input) / totals[key] for key, of_input in sizes.items()]),
            'largest_cluster_share': mean([max(of_input.values()) / totals[key] for key, of_input in sizes.items()])}


def selection_report(records, names):
    """What the tools write as ``selection.json``, from the ``SelectRecord`` values of ``select_records`` and ``names[k]``,
    the names of the files sample ``k`` wrote (none, one or several): every file's record by its name, ``picked`` (the file
    names in pick order; several inputs: one input after the other, in order of first appearance) and ``clusters`` (a list:
    the centroid's file name and the members' of every cluster, an input's clusters by id, inputs as for ``picked``)."""
    if len(names) != len(records):
        raise ValueError(f'{len(records)} records, {len(names)} lists of file names')
    report = {name: m._asdict() for m, files in zip(records, names) for name in files}
    inputs = {}
    for m in records:
        inputs.setdefault(m.input, len(inputs))
    ranked = sorted((inputs[m.input], m.pick_rank, k) for k, m in enumerate(records) if m.pick_rank is not None)
    report['picked'] = [name for _, _, k in ranked for name in names[k]]
    clusters = {}
    for k, m in enumerate(records):
        if m.cluster is not None:
            entry = clusters.setdefault((inputs[m.input], m.cluster), {'centroid': None, 'members': []})
            entry['members'] += names[k]
            if m.is_centroid and names[k]:
                entry['centroid'] = names[k][0]
    report['clusters'] = [clusters[key] for key in sorted(clusters)]
    return report


Features = namedtuple('Features', 'family anchor position marked n_features family_count status')
FeatureMatch = namedtuple('FeatureMatch', 'best_index best_d2 n_a n_b n_matched')
Pharmacophores = namedtuple('Pharmacophores', 'features_a features_b whole linker status')
PharmRecord = namedtuple('PharmRecord', 'n_a n_b n_matched score status')
PHARM_NAMES = ('feature_molecules', 'feature_flagged', 'feature_similarity', 'feature_similarity_linker')
PHARM_SC_NAMES = ('sc_similarity', 'sc_similarity_7', 'sc_similarity_8', 'sc_similarity_9')
_PHARM_TABLES = {}


def _pharm_tables(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _PHARM_TABLES:
        _PHARM_TABLES[key] = (const.feature_class_table(is_geom).to(device).contiguous(),
                              const.default_valence_table(is_geom).to(device).contiguous())
    return _PHARM_TABLES[key]


def pharmacophore_features(one_hot, x, node_mask, found, bond_aromatic, is_geom, drop_mask=None, mark_mask=None, capacity=None):
    """``dl_pharmacophore_features`` (``csrc/pharmacophore.hip``) on the results ``(found, aromatic)`` of
    ``refine_bond_orders`` for the same ``one_hot``, ``x`` and ``node_mask``: ``found`` is the refined ``Bonds`` (any ``Bonds``
    does) and ``bond_aromatic`` is ``aromatic.bond_aromatic`` ``[B,capacity of the list]``.  Device tensors in, a ``Features``
    of device tensors out, on torch's current stream, no host synchronisation.

    THE RULE is this project's own, after RDKit's ``BaseFeatures.fdef``; it is NOT RDKit's feature factory and these are NOT
    RDKit's numbers (``include/difflinker_hip.h`` states it in full; ``tests/pharmacophore_ref.py`` restates it).  Families:
    0 Donor (N, O with an open valence), 1 Acceptor (O outside aromatic rings; N without an open valence that has a multiple
    bond or is a tertiary amine away from conjugation), 2 PosIonizable (aliphatic amines; amidine and guanidine carbons),
    3 NegIonizable (carboxylic, phosphoric and sulfonic acid centres), 4 Hydrophobe (C among C; Cl, Br, I; thioether S),
    5 Aromatic (the centroid of every five- and six-ring of aromatic bonds), 6 LumpedHydrophobe (such a ring of carbons).  No
    hydrogens and no charges; no ZnBinder and no alkyl lumps.

    ``drop_mask`` (the pocket) removes atoms together with their bonds, ``mark_mask`` (the linker) marks atoms, both ``[B,N]``
    or ``[B,N,1]`` by row.  ``capacity`` is the length of the feature list per molecule, ``max(3 * N, 16)`` by default.
    ``family`` / ``anchor`` / ``marked`` ``[B,capacity]`` int32 (family -1 from the count on), ``position [B,capacity,3]``
    fp32, ``n_features [B]`` (the true count), ``family_count [B,7]``, ``status [B]``: the bits of ``found.status`` plus
    ``_lib.DL_PHARM_*`` (more than 256 kept atoms: nothing is listed; more than 64 rings: no ring features; the list too short;
    a NaN coordinate)."""
    masks = (node_mask,) + tuple(m for m in (drop_mask, mark_mask) if m is not None)
    _lib.require_device('pharmacophore_features', one_hot=one_hot, x=x, bond_aromatic=bond_aromatic, bonds=found.bonds,
                        node_mask=node_mask, drop_mask=drop_mask, mark_mask=mark_mask)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in masks) or found.bonds.dim() != 3 or found.bonds.shape[0] != B \
            or bond_aromatic.shape != found.bonds.shape[:2]:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in masks]}, bonds {tuple(found.bonds.shape)}, bond_aromatic '
                         f'{tuple(bond_aromatic.shape)}')
    dev = one_hot.device
    found = normalize_bonds(found, B, dev, 'pharmacophore_features')
    one_hot, x, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                   for t in (one_hot, x, node_mask, drop_mask, mark_mask))
    bond_aromatic = _lib.dense(bond_aromatic, dev, torch.int32)
    classes, valences = _pharm_tables(dev, is_geom)
    if classes.numel() < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {classes.numel()}')
    bond_capacity = found.bonds.shape[1]
    Fcap = max(3 * N, 16) if capacity is None else int(capacity)
    if Fcap < 0:
        raise ValueError(f'capacity must not be negative, got {capacity}')
    i32 = partial(_lib.empty_i32, dev)
    out = Features(i32(B, Fcap), i32(B, Fcap), torch.empty((B, Fcap, 3), dtype=torch.float32, device=dev), i32(B, Fcap), i32(B),
                   i32(B, _lib.DL_PHARM_FAMILIES), i32(B))
    args = _lib.DLPharmArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        mark_mask=_lib.ptr(mark_mask), feature_class=classes.data_ptr(), default_valence=valences.data_ptr(),
        capacity=bond_capacity, n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if bond_capacity else None,
        bond_aromatic=bond_aromatic.data_ptr() if bond_capacity else None, status_in=found.status.data_ptr(), Fcap=Fcap,
        family=out.family.data_ptr() if Fcap else None, anchor=out.anchor.data_ptr() if Fcap else None,
        position=out.position.data_ptr() if Fcap else None, marked=out.marked.data_ptr() if Fcap else None,
        n_features=out.n_features.data_ptr(), family_count=out.family_count.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_pharmacophore_features', args, dev)
    return out


def feature_match(a, b, radius=2.5, marked_only=False):
    """``dl_feature_match``: the Best-mode feature-map match of every pair of two ``Features`` (``a`` the samples, ``b`` their
    true molecules; any namedtuple with ``family``, ``position``, ``marked`` and ``n_features`` does, and the two lists may have
    different capacities), on torch's current stream with no host synchronisation.

    A feature takes part when its family is 0..6 and, with ``marked_only``, it is marked.  For every feature of ``b`` that takes
    part the nearest feature of ``a`` of the same family that takes part and lies strictly within ``radius``:
    ``d2 = ((dx*dx) + (dy*dy)) + (dz*dz)`` in fp32 without fused multiply-adds against ``radius * radius`` rounded to fp32 once;
    of equal distances the lowest index.  Returns a ``FeatureMatch``: ``best_index`` int32 and ``best_d2`` fp32 ``[B,Fb]``
    (-1 and +inf for none), ``n_a``, ``n_b`` (features taking part) and ``n_matched`` ``[B]``.  ``feature_score`` turns a row
    into the score.  This is RDKit's ``FeatMapScoreMode.Best`` with its default radius - on this project's features, NOT RDKit's."""
    _lib.require_device('feature_match', **{f'{side}.{name}': getattr(features, name) for side, features in (('a', a), ('b', b))
                                            for name in ('family', 'position', 'marked', 'n_features')})
    radius2 = float(radius) * float(radius)
    if not radius2 >= 0.0:
        raise ValueError(f'radius must be a number, got {radius}')
    B = a.n_features.shape[0]
    if a.family.dim() != 2 or b.family.dim() != 2:
        raise ValueError(f'shapes disagree: family {tuple(a.family.shape)} and {tuple(b.family.shape)}')
    Fa, Fb = a.family.shape[1], b.family.shape[1]
    for name, t, shape in (('a.n_features', a.n_features, (B,)), ('a.family', a.family, (B, Fa)), ('a.position', a.position, (B, Fa, 3)), ('a.marked', a.marked, (B, Fa)),
                           ('b.family', b.family, (B, Fb)), ('b.position', b.position, (B, Fb, 3)), ('b.marked', b.marked, (B, Fb)),
                           ('b.n_features', b.n_features, (B,))):
        if tuple(t.shape) != shape:
            raise ValueError(f'shapes disagree: {name} {tuple(t.shape)}, expected {shape}')
    dev = a.family.device
    fam_a, mk_a, n_a, fam_b, mk_b, n_b = (_lib.dense(t, dev, torch.int32)
                                          for t in (a.family, a.marked, a.n_features, b.family, b.marked, b.n_features))
    pos_a, pos_b = _lib.dense(a.position, dev, torch.float32), _lib.dense(b.position, dev, torch.float32)
    new = partial(_lib.empty_i32, dev)
    out = FeatureMatch(new(B, Fb), torch.empty((B, Fb), dtype=torch.float32, device=dev), new(B), new(B), new(B))
    args = _lib.DLFeatureMatchArgs(
        B=B, Fa=Fa, Fb=Fb, family_a=fam_a.data_ptr() if Fa else None, position_a=pos_a.data_ptr() if Fa else None,
        marked_a=mk_a.data_ptr() if Fa else None, n_features_a=n_a.data_ptr(),
        family_b=fam_b.data_ptr() if Fb else None, position_b=pos_b.data_ptr() if Fb else None,
        marked_b=mk_b.data_ptr() if Fb else None, n_features_b=n_b.data_ptr(), radius2=radius2,
        marked_only=int(bool(marked_only)), best_index=out.best_index.data_ptr() if Fb else None,
        best_d2=out.best_d2.data_ptr() if Fb else None, n_a=out.n_a.data_ptr(), n_b=out.n_b.data_ptr(),
        n_matched=out.n_matched.data_ptr())
    _lib.launch('dl_feature_match', args, dev)
    return out


def feature_score(best_d2, n_a, n_b):
    """The feature-map score of one pair on the host, in fp64 with ``math.exp``: ``sum_j exp(-best_d2[j]) / min(n_a, n_b)``
    over the matched features (finite ``best_d2``) in index order - RDKit's Gaussian profile of width 1 in Best mode, divided
    as the reference's ``get_FeatureMapScore`` divides.  ``None`` when ``min(n_a, n_b)`` is 0.  ``best_d2`` is a row of
    ``FeatureMatch.best_d2`` as plain floats."""
    if min(n_a, n_b) == 0:
        return None
    return sum(math.exp(-d) for d in best_d2 if d != math.inf) / min(n_a, n_b)


def analyze_pharmacophores(one_hot_a, x_a, mask_a, linker_a, one_hot_b, x_b, mask_b, linker_b, is_geom=True, drop_a=None,
                           drop_b=None, margins=const.MARGINS_EDM, radius=2.5):
    """Pharmacophore features of molecule A (the sample) and molecule B (its true molecule) of every pair of a batch, and
    their feature-map match, on the HIP device without a host synchronisation: on both sides ``perceive_bonds``, then
    ``refine_bond_orders``, then ``pharmacophore_features`` with the linker rows (``linker_a`` / ``linker_b``, ``[B,N]`` or
    ``[B,N,1]``) marked and the ``drop_a`` / ``drop_b`` rows (the pocket) left out; then ``feature_match`` twice: over all
    features (``whole``) and over the marked ones alone (``linker``).  ``Na`` and ``Nb`` may differ; the two molecules are
    compared where they are, no alignment.

    Returns a ``Pharmacophores``: ``features_a``, ``features_b`` (``Features``), ``whole``, ``linker`` (``FeatureMatch``) and
    ``status [B]``, the bits of both sides.  ``perceive_bonds`` is used with its default capacity, so a molecule whose atoms
    are piled on one another carries ``DL_BONDS_OVERFLOW`` and is left out of the scores.  The features are this project's
    own, after RDKit's ``BaseFeatures.fdef``, NOT RDKit's."""
    _lib.require_device('analyze_pharmacophores', one_hot_a=one_hot_a, x_a=x_a, mask_a=mask_a, linker_a=linker_a,
                        one_hot_b=one_hot_b, x_b=x_b, mask_b=mask_b, linker_b=linker_b)
    sides = []
    for one_hot, x, mask, linker, drop in ((one_hot_a, x_a, mask_a, linker_a, drop_a), (one_hot_b, x_b, mask_b, linker_b, drop_b)):
        B, N = one_hot.shape[:2]
        if linker.numel() != B * N or mask.numel() != B * N:
            raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, mask {tuple(mask.shape)}, linker '
                             f'{tuple(linker.shape)}')
        found = perceive_bonds(one_hot, x, mask, is_geom, margins)
        refined, aromatic = refine_bond_orders(found, one_hot, x, mask, is_geom, drop, linker)
        sides.append(pharmacophore_features(one_hot, x, mask, refined, aromatic.bond_aromatic, is_geom, drop, linker))
    fa, fb = sides
    return Pharmacophores(fa, fb, feature_match(fa, fb, radius), feature_match(fa, fb, radius, marked_only=True),
                          fa.status | fb.status)


def pharmacophores_to_host(result):
    """``(records, linker_records)`` of a ``Pharmacophores``: one ``PharmRecord`` of plain values per pair for the match over
    all features and one for the match over the linker's, the score by ``feature_score``."""
    status = result.status.cpu().tolist()
    out = []
    for match in (result.whole, result.linker):
        d2 = match.best_d2.cpu().tolist()
        columns = zip(match.n_a.cpu().tolist(), match.n_b.cpu().tolist(), match.n_matched.cpu().tolist(), d2, status)
        out.append([PharmRecord(n_a, n_b, n_matched, feature_score(row, n_a, n_b), s) for n_a, n_b, n_matched, row, s in columns])
    return tuple(out)


def _pharm_scored(record):
    return not record.status & ~(_lib.DL_BONDS_NONFINITE | _lib.DL_PHARM_NONFINITE) and record.score is not None


def compute_pharmacophores(records, linker_records=None, shape_records=None):
    """Scores of the ``PharmRecord`` values ``records`` (``pharmacophores_to_host``; A the sample, B its true molecule), in fp64.
    The features are this project's own, after RDKit's ``BaseFeatures.fdef`` and ``FeatMapParams`` defaults, NOT RDKit's: the
    numbers compare runs of this project with each other and nothing else.

    ``feature_molecules``          pairs scored: no status bit but a NaN coordinate's, and features on both sides; the others
                                   are left out of everything below
    ``feature_flagged``            pairs with any other status bit (a cut list of bonds or features, an entry that is no bond,
                                   more than 256 atoms, more than 64 rings)
    ``feature_similarity``         mean feature-map score over the whole ligand.  The sample and its true molecule SHARE THEIR
                                   FRAGMENTS, whose features match at distance 0, so this number is inflated by them and
                                   says little about the linker
    ``feature_similarity_linker``  mean score of ``linker_records``, the match over the features that sit on linker atoms
                                   alone: the informative one (``None`` without ``linker_records``)

    With ``shape_records`` (``shapes_to_host`` of ``analyze_shapes`` for the same pairs), over the pairs both scored:
    ``sc_similarity``, the mean of ``0.5 * feature score + 0.5 * (vol_min / vol_a)`` - where the reference has SC-RDKit - and
    ``sc_similarity_7/8/9``, the percentage of those pairs above 0.7 / 0.8 / 0.9.  A mean or a percentage over nothing is
    ``None``, as in ``compute_shapes``."""
    if shape_records is not None and len(shape_records) != len(records):
        raise ValueError(f'{len(records)} feature records, {len(shape_records)} shape records')
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in records if _pharm_scored(m)]
    flagged = ~(_lib.DL_BONDS_NONFINITE | _lib.DL_PHARM_NONFINITE)
    out = {'feature_molecules': len(good), 'feature_flagged': sum(1 for m in records if m.status & flagged),
           'feature_similarity': mean([m.score for m in good]),
           'feature_similarity_linker': None if linker_records is None else mean([m.score for m in linker_records
                                                                                  if _pharm_scored(m)])}
    if shape_records is not None:
        sc = [0.5 * m.score + 0.5 * (s.vol_min / s.vol_a) for m, s in zip(records, shape_records)
              if _pharm_scored(m) and _shape_scored(s)]
        above = lambda bar: 100.0 * sum(v > bar for v in sc) / len(sc) if sc else None   # noqa: E731
        out.update(sc_similarity=mean(sc), sc_similarity_7=above(0.7), sc_similarity_8=above(0.8), sc_similarity_9=above(0.9))
    return out


PoseChecks = namedtuple('PoseChecks', 'counts atom_flags status refined aromatic')
PoseRecord = namedtuple('PoseRecord', 'counts linker_counts n_flagged_atoms status')
POSE_COUNTS = ('bonds_checked', 'bonds_untabled', 'bonds_short', 'bonds_long', 'angles_checked', 'angles_bad', 'pairs_checked',
               'clashes')
POSE_NAMES = ('bond_lengths_valid', 'bond_angles_valid', 'internal_clash_free', 'pose_valid',
              'bond_lengths_valid_linker', 'bond_angles_valid_linker', 'internal_clash_free_linker', 'pose_valid_linker',
              'bad_bonds_per_molecule', 'bad_angles_per_molecule', 'internal_clashes_per_molecule')
_POSE_TABLES = {}


def _pose_tables(device, is_geom, length_bounds, angle_tolerance, clash_scale):
    key = (device, bool(is_geom), tuple(float(v) for v in length_bounds), float(angle_tolerance), float(clash_scale))
    if key not in _POSE_TABLES:
        _POSE_TABLES[key] = tuple(t.to(device).contiguous() for t in (
            const.length_bounds_table(is_geom, *length_bounds), const.angle_cos_table(angle_tolerance),
            const.internal_clash_table(is_geom, clash_scale)))
    return _POSE_TABLES[key]


def pose_checks(one_hot, x, node_mask, found, is_geom, drop_mask=None, mark_mask=None, atom_planar=None,
                length_bounds=(0.75, 1.25), angle_tolerance=25.0, clash_scale=0.75):
    """ONE launch of ``dl_pose_checks`` (``csrc/pose_checks.hip``) on the bond list ``found`` of ``perceive_bonds`` or
    ``refine_bond_orders`` for the same ``one_hot``, ``x`` and ``node_mask``, without a host synchronisation.  ``drop_mask``
    and ``mark_mask`` are ``[B,N]`` or ``[B,N,1]`` by row, ``atom_planar`` is ``[B,N]`` by atom number.  Returns device int32
    tensors ``(counts [B,2,8], atom_flags [B,N], status [B])``; ``analyze_pose_checks`` states the rule."""
    others = tuple(m for m in (node_mask, drop_mask, mark_mask, atom_planar) if m is not None)
    _lib.require_device('pose_checks', one_hot=one_hot, x=x, node_mask=node_mask, drop_mask=drop_mask, mark_mask=mark_mask,
                        atom_planar=atom_planar)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in others):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in others]}')
    dev = one_hot.device
    given = normalize_bonds(found, B, dev, 'pose_checks')
    one_hot, x, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                   for t in (one_hot, x, node_mask, drop_mask, mark_mask))
    if atom_planar is not None:
        atom_planar = _lib.dense(atom_planar.reshape(B, N) != 0, dev, torch.int32)
    bounds, cosines, clash = _pose_tables(dev, is_geom, length_bounds, angle_tolerance, clash_scale)
    if clash.shape[0] < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {clash.shape[0]}')
    if clash.shape[0] > nf:                                  # the kernel indexes the tables with nf
        bounds, clash = bounds[:nf, :nf].contiguous(), clash[:nf, :nf].contiguous()
    capacity = given.bonds.shape[1]
    counts, atom_flags, status = (_lib.empty_i32(dev, *shape) for shape in ((B, 2, _lib.DL_POSE_COUNTS), (B, N), (B,)))
    args = _lib.DLPoseArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        mark_mask=_lib.ptr(mark_mask), atom_planar=_lib.ptr(atom_planar), length_bounds2=bounds.data_ptr(),
        angle_cos=cosines.data_ptr(), clash2=clash.data_ptr(), capacity=capacity, n_bonds_in=given.n_bonds.data_ptr(),
        bonds=given.bonds.data_ptr() if capacity else None, status_in=_lib.ptr(given.status), counts=counts.data_ptr(),
        atom_flags=atom_flags.data_ptr(), status=status.data_ptr())
    _lib.launch('dl_pose_checks', args, dev)
    return counts, atom_flags, status


def analyze_pose_checks(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM,
                        length_bounds=(0.75, 1.25), angle_tolerance=25.0, clash_scale=0.75):
    """Is the internal 3D geometry of every molecule of a batch plausible?  Three launches on the HIP device and no host round
    trip between them: ``perceive_bonds``, ``refine_bond_orders`` and ``dl_pose_checks``.  The check ALWAYS runs on the
    geometric (Kekule) orders and on ``atom_aromatic``, whatever orders the files are written with: the distance table's
    arbitrary orders inside aromatic rings would misclass ring atoms.

    THE RULE is this project's own, after the idea of PoseBusters' intramolecular checks (``include/difflinker_hip.h`` states
    it in full; ``tests/pose_checks_ref.py`` restates it).  It is NOT PoseBusters and these are NOT PoseBusters' numbers: no
    RDKit distance-geometry bounds, no hydrogens, no energy, no ring or double-bond flatness.  A bond of order k between two
    elements is SHORT below ``length_bounds[0]`` and LONG above ``length_bounds[1]`` times the typical length of that order
    (``const.BOND_LENGTHS``; a pair without one is ``untabled`` and not checked).  An angle j-a-k at an atom with 2 to 4
    neighbours is BAD when it is more than ``angle_tolerance`` degrees from 180 (a triple or two double bonds at a), 120 (a
    double bond at an atom of at most three neighbours, or an aromatic atom) or 109.47 degrees (otherwise); the angles of
    three- and four-rings are exempt.  Two atoms with no path of three or fewer bonds between them CLASH when they are closer
    than ``clash_scale`` times the sum of their van der Waals radii (``const.VDW_RADII``).  fp64 throughout.

    ``linker_mask`` rows are marked - an item counts as the linker's when one of its atoms is a linker atom - and
    ``drop_mask`` rows (the pocket of a pocket model) are left out, both ``[B,N]`` or ``[B,N,1]``.  Returns a ``PoseChecks`` of
    device tensors: ``counts [B,2,8]`` (row 0 all items, row 1 the linker's; ``POSE_COUNTS`` names the eight values),
    ``atom_flags [B,N]`` by atom number (1 an end of a short or long bond, 2 the centre of a bad angle, 4 in a clash),
    ``status [B]`` (the bits of the two launches before plus ``_lib.DL_POSE_*``; more than 256 kept atoms or a non-finite
    coordinate: nothing is counted), and ``refined`` / ``aromatic`` as ``refine_bond_orders`` returns them."""
    _lib.require_device('analyze_pose_checks', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_bonds(one_hot, x, node_mask, is_geom, margins)
    linker = linker_mask.reshape(B, N).to(torch.float32)
    refined, aromatic = refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask, linker)
    counts, atom_flags, status = pose_checks(one_hot, x, node_mask, refined._replace(status=aromatic.status), is_geom, drop_mask,
                                             linker, aromatic.atom_aromatic, length_bounds, angle_tolerance, clash_scale)
    return PoseChecks(counts, atom_flags, status, refined, aromatic)


def pose_checks_to_host(result):
    """One ``PoseRecord`` of plain values per molecule of a ``PoseChecks``: the eight counts over all items and over the
    linker's, the number of flagged atoms, and ``status``."""
    counts, status = result.counts.cpu().tolist(), result.status.cpu().tolist()
    flagged = (result.atom_flags != 0).sum(dim=1).cpu().tolist()
    return [PoseRecord(tuple(counts[b][0]), tuple(counts[b][1]), flagged[b], status[b]) for b in range(len(status))]


def _pose_scores(records, prefix=''):
    short, long_, bad_angles, clashes = (POSE_COUNTS.index(name) for name in ('bonds_short', 'bonds_long', 'angles_bad', 'clashes'))
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    good = [m for m in records if m.status == 0]
    out = {}
    for suffix, row in (('', 'counts'), ('_linker', 'linker_counts')):
        tests = {'bond_lengths_valid': lambda c: c[short] + c[long_] == 0, 'bond_angles_valid': lambda c: c[bad_angles] == 0,
                 'internal_clash_free': lambda c: c[clashes] == 0,
                 'pose_valid': lambda c: c[short] + c[long_] + c[bad_angles] + c[clashes] == 0}
        for name, passes in tests.items():
            out[prefix + name + suffix] = mean([m.status == 0 and passes(getattr(m, row)) for m in records])
    out[prefix + 'bad_bonds_per_molecule'] = mean([m.counts[short] + m.counts[long_] for m in good])
    out[prefix + 'bad_angles_per_molecule'] = mean([m.counts[bad_angles] for m in good])
    out[prefix + 'internal_clashes_per_molecule'] = mean([m.counts[clashes] for m in good])
    return out


def compute_pose_checks(pred, true=None):
    """Scores of the ``PoseRecord`` values ``pred`` (``pose_checks_to_host``), in fp64.  The rule is this project's own, after
    the idea of PoseBusters' intramolecular checks, NOT PoseBusters: the numbers compare runs of this project with each other.

    ``bond_lengths_valid``             share of the records with status 0 and no short or long bond
    ``bond_angles_valid``              share with status 0 and no bad angle
    ``internal_clash_free``            share with status 0 and no internal clash
    ``pose_valid``                     share with status 0 and none of the three
    ``..._linker``                     the same four over the items that touch a linker atom.  THE INFORMATIVE ONES: the
                                       fragments are input, and crystal fragments are noisy
    ``bad_bonds_per_molecule``         mean number of short or long bonds, over the records with status 0
    ``bad_angles_per_molecule``        mean number of bad angles, likewise
    ``internal_clashes_per_molecule``  mean number of clashing pairs, likewise

    A record with any status bit (a cut list, an entry that is no bond, more than 256 atoms, a non-finite coordinate) is valid
    in nothing.  With ``true`` - one record per prediction, the data set's own molecule - the same eleven values of those
    records under ``true_`` + name.  A share or a mean over nothing is ``None``, as in ``compute_aromatic``."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    out = _pose_scores(pred)
    if true is not None:
        out.update(_pose_scores(true, 'true_'))
    return out


# ---- relaxation: what ``molecule_builder.relax`` did to every sample ---------------------------------------------------------------
RelaxRecord = namedtuple('RelaxRecord', 'energy_before energy_after steps_done f_max displacement status bonds_changed converged')
RELAX_TERMS = ('bonds', 'angles', 'repulsion', 'wall', 'restraint')
RELAX_NAMES = ('relax_molecules', 'relax_energy_before', 'relax_energy_after', 'relax_displacement_mean',
               'relax_displacement_max', 'relax_converged', 'relax_bonds_changed')


def bonds_changed(raw, relaxed):
    """Device bool ``[B]``: does the list of ``perceive_bonds`` on the relaxed coordinates differ from the one on the raw
    coordinates - another count, or another entry among those both lists hold?  ``perceive_bonds`` writes its list in a fixed
    order, so equal lists are equal graphs with equal orders."""
    capacity = min(raw.bonds.shape[1], relaxed.bonds.shape[1])
    held = torch.arange(capacity, device=raw.bonds.device)[None, :] < torch.minimum(raw.n_bonds, relaxed.n_bonds)[:, None]
    differ = (raw.bonds[:, :capacity] != relaxed.bonds[:, :capacity]).any(dim=2) & held
    return (raw.n_bonds != relaxed.n_bonds) | differ.any(dim=1)


def relax_to_host(result, raw=None, relaxed=None, f_tol=const.RELAX_DEFAULTS['f_tol']):
    """One ``RelaxRecord`` of plain values per molecule of a ``Relaxed`` (``molecule_builder.relax``): the five energy terms
    (``RELAX_TERMS``) before and after, the steps done, the last largest force on an atom (its length), the largest displacement of an atom
    in Angstrom, ``status``, whether the distance-table bond list changed (``raw`` and ``relaxed``: the ``perceive_bonds`` of
    the two sets of coordinates; ``None`` without them) and whether the run stopped on ``f_tol``."""
    energy, steps, status = result.energy.cpu().tolist(), result.steps_done.cpu().tolist(), result.status.cpu().tolist()
    f_max, moved = result.f_max.cpu().tolist(), result.moved2.sqrt().cpu().tolist()
    changed = bonds_changed(raw, relaxed).cpu().tolist() if raw is not None and relaxed is not None else [None] * len(status)
    return [RelaxRecord(tuple(energy[b][0]), tuple(energy[b][1]), steps[b], f_max[b], moved[b], status[b], changed[b],
                        status[b] == 0 and f_max[b] < f_tol) for b in range(len(status))]


def relax_report(record):
    """The JSON record of one ``RelaxRecord``, as the drivers write it to ``relax.json`` per written file."""
    return {'energy_before': dict(zip(RELAX_TERMS, record.energy_before)), 'energy_after': dict(zip(RELAX_TERMS, record.energy_after)),
            'steps_done': record.steps_done, 'f_max': record.f_max, 'displacement': record.displacement,
            'status': record.status, 'bonds_changed': record.bonds_changed, 'converged': record.converged}


def compute_relaxation(records):
    """Scores of the ``RelaxRecord`` values ``records`` (``relax_to_host``), in fp64, over the records with status 0.  The
    energy is this project's own restraint energy in units of its own, NOT a force field's: the numbers compare runs of this
    project with each other.

    ``relax_molecules``            records with status 0
    ``relax_energy_before``        mean of bonds + angles + repulsion + wall at the sampled coordinates (the restraint is not
                                   a property of the molecule and is left out)
    ``relax_energy_after``         the same at the relaxed coordinates
    ``relax_displacement_mean``    mean over the molecules of the largest displacement of an atom, in Angstrom
    ``relax_displacement_max``     the largest displacement of any atom
    ``relax_converged``            share that stopped on ``f_tol`` before the steps ran out
    ``relax_bonds_changed``        share whose distance-table bond list on the relaxed coordinates differs from the raw one:
                                   the relaxation is a clean-up only while this stays small

    A mean or a share over nothing is ``None``."""
    good = [m for m in records if m.status == 0]
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    judged = [m.bonds_changed for m in good if m.bonds_changed is not None]
    return {'relax_molecules': len(good),
            'relax_energy_before': mean([sum(m.energy_before[:4]) for m in good]),
            'relax_energy_after': mean([sum(m.energy_after[:4]) for m in good]),
            'relax_displacement_mean': mean([m.displacement for m in good]),
            'relax_displacement_max': max([m.displacement for m in good]) if good else None,
            'relax_converged': mean([bool(m.converged) for m in good]),
            'relax_bonds_changed': mean([bool(v) for v in judged])}


PatternMatches = namedtuple('PatternMatches', 'first_root first_root_marked n_hits n_hits_marked status')
FilterRecord = namedtuple('FilterRecord', 'hits linker_hits status')
FILTER_NAMES = ('filters_passed', 'filters_passed_linker', 'filter_hits_per_molecule', 'filters_budget')
MAX_PATTERN_STEPS = 1 << 24
_PATTERN_TABLES = {}
_ELEMENT_TABLES = {}


def _pattern_tables(device, patterns):
    """The compiled tables of ``patterns`` on ``device``, uploaded once per catalogue and device."""
    key = (device, id(patterns))
    if key not in _PATTERN_TABLES:
        _PATTERN_TABLES[key] = (patterns, tuple(t.to(device=device, dtype=torch.int32).contiguous()
                                                for t in (patterns.pat, patterns.atoms, patterns.closures, patterns.preds)))
    return _PATTERN_TABLES[key][1]


def _element_tables(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _ELEMENT_TABLES:
        _ELEMENT_TABLES[key] = (const.atomic_number_table(is_geom).to(device).contiguous(),
                                const.default_valence_table(is_geom).to(device).contiguous())
    return _ELEMENT_TABLES[key]


def match_patterns(one_hot, x, node_mask, found, bond_aromatic, patterns, is_geom, drop_mask=None, mark_mask=None,
                   max_steps=4096):
    """``dl_substructure_match`` (``csrc/substructure.hip``) on the results ``(found, aromatic)`` of ``refine_bond_orders`` for
    the same ``one_hot``, ``x`` and ``node_mask``: ``found`` is the refined ``Bonds`` (any ``Bonds`` does), ``bond_aromatic`` is
    ``aromatic.bond_aromatic`` ``[B,capacity of the list]`` (``None``: no bond is aromatic) and ``patterns`` a catalogue
    compiled by ``patterns.compile_patterns``.  Device tensors in, a ``PatternMatches`` of int32 device tensors out, on torch's
    current stream, no host synchronisation.  ``x`` plays no part in the rule; it is taken so that the call reads like
    ``pharmacophore_features``.

    THE RULE is this project's own (``include/difflinker_hip.h`` states it in full, ``tests/substructure_ref.py`` restates
    it): NOT RDKit's matcher.  For every pattern and every kept atom as root a depth-first search, in the order the pattern is
    written, for an injective map of the pattern's atoms to kept atoms under which every atom predicate holds and every
    pattern bond falls on a kept bond whose predicate holds.  Every candidate tested is one step; a root's search stops after
    ``max_steps`` steps and sets ``_lib.DL_SUB_BUDGET``.

    ``drop_mask`` (the pocket) removes atoms together with their bonds, ``mark_mask`` (the linker) marks atoms, both ``[B,N]``
    or ``[B,N,1]`` by row.  ``first_root [B,P]``: the lowest row that roots a match of pattern ``p``, -1 for none;
    ``first_root_marked``: the same for matches that touch a marked atom (all -1 without ``mark_mask``); ``n_hits``,
    ``n_hits_marked`` ``[B]``; ``status [B]``: the bits of ``found.status`` plus ``_lib.DL_SUB_TOO_LARGE`` (more than 256 kept
    atoms or 2048 kept bonds: nothing is searched), ``_lib.DL_SUB_BAD_BOND`` and ``_lib.DL_SUB_BUDGET``.  An empty catalogue
    gives zero counts and the status of ``found`` (with ``DL_BONDS_OVERFLOW`` for a list cut short, as with any other)."""
    masks = (node_mask,) + tuple(m for m in (drop_mask, mark_mask) if m is not None)
    _lib.require_device('match_patterns', one_hot=one_hot, bond_aromatic=bond_aromatic, bonds=found.bonds, node_mask=node_mask,
                        drop_mask=drop_mask, mark_mask=mark_mask)
    B, N, nf = one_hot.shape
    if any(m.numel() != B * N for m in masks) or found.bonds.dim() != 3 or found.bonds.shape[0] != B \
            or (bond_aromatic is not None and bond_aromatic.shape != found.bonds.shape[:2]):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, masks {[tuple(m.shape) for m in masks]}, bonds '
                         f'{tuple(found.bonds.shape)}, bond_aromatic '
                         f'{None if bond_aromatic is None else tuple(bond_aromatic.shape)}')
    if not 1 <= int(max_steps) <= MAX_PATTERN_STEPS:
        raise ValueError(f'max_steps must be in 1..{MAX_PATTERN_STEPS}, got {max_steps!r}')
    dev = one_hot.device
    found = normalize_bonds(found, B, dev, 'match_patterns')
    one_hot, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                for t in (one_hot, node_mask, drop_mask, mark_mask))
    bond_aromatic = _lib.dense(bond_aromatic, dev, torch.int32)
    numbers, valences = _element_tables(dev, is_geom)
    if numbers.numel() < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {numbers.numel()}')
    P = patterns.n_top
    if P == 0:
        zeros = partial(torch.zeros, dtype=torch.int32, device=dev)
        cut = (found.n_bonds > found.bonds.shape[1]).to(torch.int32) * _lib.DL_BONDS_OVERFLOW      # as the kernel adds it
        return PatternMatches(zeros((B, 0)), zeros((B, 0)), zeros(B), zeros(B), found.status.to(torch.int32) | cut)
    pat, atoms, closures, preds = _pattern_tables(dev, patterns)
    capacity = found.bonds.shape[1]
    i32 = partial(_lib.empty_i32, dev)
    out = PatternMatches(i32(B, P), i32(B, P), i32(B), i32(B), i32(B))
    args = _lib.DLSubstructureArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        mark_mask=_lib.ptr(mark_mask), atomic_number=numbers.data_ptr(), default_valence=valences.data_ptr(), capacity=capacity,
        n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if capacity else None,
        bond_aromatic=bond_aromatic.data_ptr() if capacity and bond_aromatic is not None else None,
        status_in=found.status.data_ptr(), n_sub=patterns.n_sub, n_top=P, n_levels=len(patterns.level_end),
        level_end=(ctypes.c_int32 * _lib.DL_SUB_MAX_LEVELS)(*patterns.level_end),
        pat=pat.data_ptr(), atoms=atoms.data_ptr(), closures=closures.data_ptr() if closures.numel() else None,
        preds=preds.data_ptr() if preds.numel() else None, n_atoms_table=atoms.shape[0], n_closures=closures.shape[0],
        n_preds=preds.numel(), max_steps=int(max_steps), first_root=out.first_root.data_ptr(),
        first_root_marked=out.first_root_marked.data_ptr(), n_hits=out.n_hits.data_ptr(),
        n_hits_marked=out.n_hits_marked.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_substructure_match', args, dev)
    return out


def analyze_patterns(one_hot, x, node_mask, is_geom, linker_mask, patterns, drop_mask=None, margins=const.MARGINS_EDM,
                     max_steps=4096):
    """The catalogue ``patterns`` matched against every molecule of a batch on the HIP device without a host synchronisation:
    ``perceive_bonds``, then ``refine_bond_orders``, then ``match_patterns`` with the ``linker_mask`` rows (``[B,N]`` or
    ``[B,N,1]``) marked and the ``drop_mask`` rows (the pocket) left out.  Returns a ``PatternMatches``.  ``perceive_bonds``
    is used with its default capacity, as in ``analyze_pharmacophores``.  The bond orders and the aromatic flags are those
    of this project's geometric perception of five- and six-rings, NOT RDKit's aromaticity model."""
    _lib.require_device('analyze_patterns', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N or node_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}, linker_mask '
                         f'{tuple(linker_mask.shape)}')
    found = perceive_bonds(one_hot, x, node_mask, is_geom, margins)
    refined, aromatic = refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask, linker_mask)
    return match_patterns(one_hot, x, node_mask, refined, aromatic.bond_aromatic, patterns, is_geom, drop_mask, linker_mask,
                          max_steps)


def patterns_to_host(result, names):
    """One ``FilterRecord`` per molecule of a ``PatternMatches``: ``hits``, the names of the patterns that match, in catalogue
    order; ``linker_hits``, those that match through a marked atom; and ``status``.  Synchronises."""
    first, marked = result.first_root.cpu().tolist(), result.first_root_marked.cpu().tolist()
    status = result.status.cpu().tolist()
    hit = lambda row: [names[p] for p, r in enumerate(row) if r >= 0]                   # noqa: E731
    return [FilterRecord(hit(first[b]), hit(marked[b]), status[b]) for b in range(len(status))]


def compute_filters(pred, true=None):
    """Scores of the ``FilterRecord`` values ``pred`` (``patterns_to_host``), in fp64, over ALL records:

    ``filters_passed``            share of molecules with no hit and no budget bit - the reference's ``pains`` column, as a
                                  fraction, on whatever catalogue was given.  A molecule that was not searched
                                  (``DL_SUB_TOO_LARGE``) does not pass
    ``filters_passed_linker``     share with no hit that touches the linker, and no budget bit: the informative one, because
                                  the fragments are input
    ``filter_hits_per_molecule``  mean number of patterns hit
    ``filters_budget``            share with ``DL_SUB_BUDGET`` set (a search was cut short: raise ``max_steps``)

    With ``true`` - one record per prediction, the data set's own molecule - the same four over those records as ``true_...``.
    A share over nothing is ``None``, as in ``compute_rings``."""
    if true is not None and len(true) != len(pred):
        raise ValueError(f'{len(pred)} predictions, {len(true)} true records')
    mean = lambda values: float(sum(values) / len(values)) if values else None      # noqa: E731
    unsure = _lib.DL_SUB_BUDGET | _lib.DL_SUB_TOO_LARGE

    def scores(records, prefix):
        return {f'{prefix}filters_passed': mean([not m.hits and not m.status & unsure for m in records]),
                f'{prefix}filters_passed_linker': mean([not m.linker_hits and not m.status & unsure for m in records]),
                f'{prefix}filter_hits_per_molecule': mean([len(m.hits) for m in records]),
                f'{prefix}filters_budget': mean([bool(m.status & _lib.DL_SUB_BUDGET) for m in records])}
    out = scores(pred, '')
    if true is not None:
        out.update(scores(true, 'true_'))
    return out


def write_filters_json(path, files, records):
    """``filters.json``: one record per written file (``files``: its name as the other reports give it, with the
    ``FilterRecord`` of its molecule): ``file``, ``hits``, ``linker_hits`` and ``status``."""
    import json
    with open(path, 'w') as f:
        json.dump([{'file': name, 'hits': list(m.hits), 'linker_hits': list(m.linker_hits), 'status': m.status}
                   for name, m in zip(files, records)], f, indent=1)


def load_filters(spec):
    """The catalogue behind ``--filters``: ``'basic'`` (``data/filters_basic.csv``, this project's own short list of structural
    alerts) or the path of a pattern file (CSV: SMARTS, optional name; the reference's PAINS list has this form), compiled."""
    return pattern_compiler.load_catalogue(spec)


# ---- stereo perception from 3D (``dl_stereo_perceive``, ``csrc/stereo.hip``) ---------------------------------------------------
STEREO_COUNTS = ('centres', 'centres_undetermined', 'double_bonds', 'double_bonds_undetermined')
_STEREO_TABLES = {}


def _stereo_valence(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _STEREO_TABLES:
        _STEREO_TABLES[key] = const.default_valence_table(is_geom).to(device).contiguous()
    return _STEREO_TABLES[key]


def stereo(one_hot, x, node_mask, found, is_geom, drop_mask=None, mark_mask=None, atom_planar=None, bond_aromatic=None,
           flat=const.STEREO_DEFAULTS['flat'], twist=const.STEREO_DEFAULTS['twist']):
    """ONE launch of ``dl_stereo_perceive`` (``csrc/stereo.hip``) on the bond list ``found`` of ``perceive_bonds`` or
    ``refine_bond_orders`` for the same ``one_hot``, ``x`` and ``node_mask``, with the input handling of ``pose_checks``;
    device tensors in, a dict of device tensors out, no host synchronisation.  ``drop_mask`` and ``mark_mask`` are ``[B,N]`` or
    ``[B,N,1]`` by row, ``atom_planar`` is ``[B,N]`` by atom number and ``bond_aromatic`` ``[B,capacity of the list]`` (the
    ``atom_aromatic`` and ``bond_aromatic`` of ``refine_bond_orders``); each may be ``None``.

    THE RULE is this project's own (``include/difflinker_hip.h`` states it in full, ``tests/stereo_ref.py`` restates it): NOT
    RDKit's stereo perception and NOT CIP.  A kept atom with single bonds only, four different neighbours (or three and one
    implicit hydrogen) by the colour classes of ``canonical_ranks``' root refinement is a centre; the sign of the determinant
    of the unit vectors to its neighbours in class order is its label 1 or 2, and 3 (undetermined) when the volume is below
    ``flat`` times the ideal one.  A double bond outside aromatic rings and rings of fewer than 8 atoms whose ends each have
    one or two single-bonded other neighbours of different classes is a stereo double bond: label 1 when the two highest-class
    neighbours are on one side (cosine of the torsion above ``twist``), 2 when on opposite sides, 3 in between.  The labels
    are relative to the classes: no R/S, no E/Z.

    ``atom_class``   int32 ``[B,N]`` by atom number: the classes (tied ranks); -1 for dropped atoms and from the atom count on
    ``atom_stereo``  int32 ``[B,N]`` by atom number: 0 no centre, 1, 2, 3; -1 where ``atom_class`` is
    ``bond_stereo``  int32 ``[B,capacity]`` by list entry: the label on the first entry of a stereo double bond's pair, else 0
    ``counts``       int32 ``[B,2,4]``: ``STEREO_COUNTS`` over the kept molecule, and over the items with a marked atom
    ``status``       int32 ``[B]``: the bits of ``found.status`` plus ``_lib.DL_STEREO_*`` (more than 256 kept atoms or 2048
                     kept list entries: classes -1 and nothing perceived; a non-finite coordinate: classes only)"""
    others = tuple(m for m in (node_mask, drop_mask, mark_mask, atom_planar) if m is not None)
    _lib.require_device('stereo', one_hot=one_hot, x=x, node_mask=node_mask, drop_mask=drop_mask, mark_mask=mark_mask,
                        atom_planar=atom_planar, bond_aromatic=bond_aromatic)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in others):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in others]}')
    flat, twist = float(flat), float(twist)
    if not (flat >= 0.0 and twist >= 0.0):
        raise ValueError(f'flat and twist must not be negative or NaN, got {flat!r} and {twist!r}')
    dev = one_hot.device
    given = normalize_bonds(found, B, dev, 'stereo')
    capacity = given.bonds.shape[1]
    if bond_aromatic is not None and tuple(bond_aromatic.shape) != (B, capacity):
        raise ValueError(f'bond_aromatic {tuple(bond_aromatic.shape)} does not go with bonds {tuple(given.bonds.shape)}')
    one_hot, x, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                   for t in (one_hot, x, node_mask, drop_mask, mark_mask))
    if atom_planar is not None:
        atom_planar = _lib.dense(atom_planar.reshape(B, N) != 0, dev, torch.int32)
    bond_aromatic = _lib.dense(bond_aromatic, dev, torch.int32)
    valences = _stereo_valence(dev, is_geom)
    if valences.numel() < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {valences.numel()}')
    out = {'atom_class': _lib.empty_i32(dev, B, N), 'atom_stereo': _lib.empty_i32(dev, B, N),
           'bond_stereo': _lib.empty_i32(dev, B, capacity), 'counts': _lib.empty_i32(dev, B, 2, _lib.DL_STEREO_COUNTS),
           'status': _lib.empty_i32(dev, B)}
    args = _lib.DLStereoArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        mark_mask=_lib.ptr(mark_mask), atom_planar=_lib.ptr(atom_planar), default_valence=valences.data_ptr(), capacity=capacity,
        n_bonds_in=given.n_bonds.data_ptr(), bonds=given.bonds.data_ptr() if capacity else None,
        bond_aromatic=bond_aromatic.data_ptr() if capacity and bond_aromatic is not None else None,
        status_in=_lib.ptr(given.status), flat=flat, twist=twist, v_ideal4=const.STEREO_V_IDEAL[0],
        v_ideal3=const.STEREO_V_IDEAL[1], atom_class=out['atom_class'].data_ptr(), atom_stereo=out['atom_stereo'].data_ptr(),
        bond_stereo=out['bond_stereo'].data_ptr() if capacity else None, counts=out['counts'].data_ptr(),
        status=out['status'].data_ptr())
    _lib.launch('dl_stereo_perceive', args, dev)
    return out


def stereo_types(one_hot, node_mask, found, atom_stereo, bond_stereo, mirror=False):
    """The widened one-hot ``[B,N,16 nf]`` that folds the labels of a ``stereo`` result into the atom types, on the device of
    its inputs (they may be host tensors: the tests build the host codes from it): the type index of a row is
    ``type * 16 + atom_label * 4 + bond_label``, with ``atom_label`` the atom's ``atom_stereo`` (3 and -1 count as 0; 1 and 2
    exchanged with ``mirror``) and ``bond_label`` the label of the atom's stereo double bond (3 counts as 0; an atom has at most
    one, because its other bonds are single)."""
    B, N, nf = one_hot.shape
    if nf * 16 > 256:
        raise ValueError(f'{nf} atom types times 16 labels do not fit the 256 types of dl_canonical_ranks')
    dev = one_hot.device
    real = node_mask.reshape(B, N) != 0
    number = (real.to(torch.int64).cumsum(dim=1) - 1).clamp(min=0)              # the atom number of a real row
    label = atom_stereo.to(torch.int64)
    label = torch.where((label == 1) | (label == 2), 3 - label if mirror else label, torch.zeros_like(label))
    on_bond = bond_stereo.to(torch.int64)
    on_bond = torch.where(on_bond == 3, torch.zeros_like(on_bond), on_bond)
    by_atom = torch.zeros((B, N), dtype=torch.int64, device=dev)
    if on_bond.shape[1]:
        ends = found.bonds.to(torch.int64).clamp(min=0, max=N - 1)              # an entry that is no bond carries label 0
        by_atom.scatter_add_(1, ends[:, :, 0], on_bond)
        by_atom.scatter_add_(1, ends[:, :, 1], on_bond)
    index = one_hot.argmax(dim=2) * 16 + label.gather(1, number) * 4 + by_atom.gather(1, number)
    index = torch.where(real, index, torch.zeros_like(index))
    return torch.nn.functional.one_hot(index, nf * 16).to(torch.float32)


def stereo_codes(result, one_hot, node_mask, found, drop_mask=None, max_leaves=256):
    """Stereo-aware canonical codes from a ``stereo`` result, by TWO launches of the existing ``dl_canonical_ranks`` on the
    widened types of ``stereo_types`` (``csrc/canon.hip`` is unchanged: its atom types come from a one-hot row up to 256 wide).
    Device tensors in and out, no host synchronisation.

    ``stereo_code``  int64 ``[B]``: the canonical code of the graph with its labels; ``stereo_rank`` int32 ``[B,N]``: its ranks
    ``mirror_code``  int64 ``[B]``: the same with the atom labels 1 and 2 exchanged - the mirror image's ``stereo_code``
    ``chiral``       bool ``[B]``: ``stereo_code != mirror_code``; a meso compound is not chiral
    ``complete``     bool ``[B]``: no label was 3 (undetermined labels are left out of the code) and neither launch set
                     ``DL_CANON_BUDGET``, ``DL_CANON_BAD_BOND`` or ``DL_CANON_TOO_LARGE``
    ``status``       int32 ``[B]``: the status bits of the two launches"""
    _lib.require_device('stereo_codes', one_hot=one_hot, node_mask=node_mask, drop_mask=drop_mask,
                        atom_stereo=result['atom_stereo'], bond_stereo=result['bond_stereo'])
    B = one_hot.shape[0]
    given = normalize_bonds(found, B, one_hot.device, 'stereo_codes')
    # (is_geom plays no part in canonical_ranks: the graph carries type indices, here the widened ones of any vocabulary)
    runs = [canonical_ranks(stereo_types(one_hot, node_mask, given, result['atom_stereo'], result['bond_stereo'], mirror),
                            node_mask, given, True, drop_mask, max_leaves) for mirror in (False, True)]
    status = runs[0]['status'] | runs[1]['status']
    undetermined = result['counts'][:, 0, 1] + result['counts'][:, 0, 3]
    flagged = status & (_lib.DL_CANON_BUDGET | _lib.DL_CANON_BAD_BOND | _lib.DL_CANON_TOO_LARGE)
    return {'stereo_code': runs[0]['code'], 'stereo_rank': runs[0]['rank'], 'mirror_code': runs[1]['code'],
            'chiral': runs[0]['code'] != runs[1]['code'], 'complete': (undetermined == 0) & (flagged == 0), 'status': status}


StereoRecord = namedtuple('StereoRecord', 'centres centres_linker double_bonds double_bonds_linker undetermined candidates '
                                          'code stereo_code mirror_code chiral complete isomeric_smiles')
STEREO_NAMES = ('stereocentres_per_molecule', 'stereocentres_per_molecule_linker', 'stereo_bonds_per_molecule',
                'stereo_bonds_per_molecule_linker', 'stereo_undetermined', 'chiral_fraction', 'stereo_uniqueness')
STEREO_TRUE_NAMES = ('stereo_recovery', 'stereo_mirror', 'stereo_recovered_inputs')
STEREO_JSON = ('centres', 'centres_linker', 'double_bonds', 'double_bonds_linker', 'undetermined', 'stereo_code', 'chiral',
               'complete', 'isomeric_smiles')


def isomeric_smiles_to_host(result, codes, one_hot, node_mask, found, drop_mask=None):
    """One isomeric string per molecule from a ``stereo`` result and its ``stereo_codes``, on the host:
    ``molecule_builder.smiles`` on the kept atoms with the ranks of the stereo-aware labelling, the classes and the labels.
    ``None`` as ``smiles_to_host`` answers it.  Synchronises."""
    B, N = one_hot.shape[:2]
    rank, classes, labels = (t.cpu().tolist() for t in (codes['stereo_rank'], result['atom_class'], result['atom_stereo']))
    on_bond = result['bond_stereo'].cpu().tolist()
    too_large = (codes['status'].cpu() & _lib.DL_CANON_TOO_LARGE).tolist()
    n_bonds, bonds = found.n_bonds.cpu().tolist(), found.bonds.cpu()
    real = node_mask.reshape(B, N).cpu() != 0
    types = one_hot.detach().cpu().argmax(dim=2)
    out = []
    for b in range(B):
        t = types[b][real[b]].tolist()
        new = {k: r for k, r in enumerate(rank[b][:len(t)]) if r >= 0}      # atom number -> rank, kept atoms only
        if too_large[b]:
            out.append(None)
            continue
        index = {k: at for at, k in enumerate(new)}
        rows = [(e, row) for e, row in enumerate(bonds[b, :max(0, min(n_bonds[b], bonds.shape[1]))].tolist())
                if row[0] in index and row[1] in index and row[0] != row[1] and 1 <= row[2] <= 3]
        out.append(smiles([t[k] for k in new], [(index[i], index[j], o) for _, (i, j, o) in rows], [new[k] for k in new],
                          [classes[b][k] for k in new], [labels[b][k] for k in new], [on_bond[b][e] for e, _ in rows]))
    return out


def stereo_records(one_hot, x, node_mask, found, is_geom, linker_mask, drop_mask=None, atom_planar=None, bond_aromatic=None,
                   flat=const.STEREO_DEFAULTS['flat'], twist=const.STEREO_DEFAULTS['twist'], max_leaves=256):
    """One ``StereoRecord`` per molecule of a batch on the bond list ``found`` (the geometric orders of
    ``refine_bond_orders``, with its ``atom_aromatic`` and ``bond_aromatic``): one launch of ``dl_stereo_perceive`` and three of
    ``dl_canonical_ranks`` (the plain code, ``stereo_codes``' two).  ``centres`` and ``double_bonds`` count the assigned
    items (label 1 or 2), ``*_linker`` those that touch a ``linker_mask`` atom, ``undetermined`` the label-3 items of both
    kinds and ``candidates`` all items; ``code``, ``stereo_code`` and ``mirror_code`` are 16 hex digits; ``isomeric_smiles`` is
    ``''`` where there is none.  Synchronises."""
    B, N = one_hot.shape[:2]
    linker = linker_mask.reshape(B, N).to(torch.float32)
    result = stereo(one_hot, x, node_mask, found, is_geom, drop_mask, linker, atom_planar, bond_aromatic, flat, twist)
    codes = stereo_codes(result, one_hot, node_mask, found, drop_mask, max_leaves)
    plain = canonical_ranks(one_hot, node_mask, found, is_geom, drop_mask, max_leaves)
    strings = isomeric_smiles_to_host(result, codes, one_hot, node_mask, found, drop_mask)
    counts = result['counts'].cpu().tolist()
    hexed = lambda t: [format(v & 0xFFFFFFFFFFFFFFFF, '016x') for v in t.cpu().tolist()]      # noqa: E731
    code, stereo_code, mirror_code = hexed(plain['code']), hexed(codes['stereo_code']), hexed(codes['mirror_code'])
    chiral, complete = codes['chiral'].cpu().tolist(), codes['complete'].cpu().tolist()
    return [StereoRecord(counts[b][0][0], counts[b][1][0], counts[b][0][2], counts[b][1][2], counts[b][0][1] + counts[b][0][3],
                         sum(counts[b][0]), code[b], stereo_code[b], mirror_code[b], int(chiral[b]),
                         int(complete[b] and strings[b] is not None), strings[b] or '') for b in range(B)]


def analyze_stereo(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM,
                   flat=const.STEREO_DEFAULTS['flat'], twist=const.STEREO_DEFAULTS['twist'], max_leaves=256):
    """The ``StereoRecord`` of every molecule of a batch from its coordinates alone: ``perceive_all_bonds``,
    ``refine_bond_orders`` and ``stereo_records``.  The perception ALWAYS runs on the geometric (Kekule) orders with the
    aromatic atoms as planar and the aromatic bonds flagged, whatever orders the files are written with: the distance table's
    orders inside aromatic rings are arbitrary.  Synchronises."""
    _lib.require_device('analyze_stereo', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    linker = linker_mask.reshape(B, N).to(torch.float32)
    refined, aromatic = refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask, linker)
    return stereo_records(one_hot, x, node_mask, refined._replace(status=aromatic.status), is_geom, linker, drop_mask,
                          aromatic.atom_aromatic, aromatic.bond_aromatic, flat, twist, max_leaves)


def compute_stereo(rows, pred, true=None, true_rows=None, input_index=None):
    """The stereo scores: ``rows`` are the ``StereoRecord`` values of the samples (``stereo_records``), ``pred`` and ``true`` the
    ``Molecule`` records ``compute_metrics`` takes for the same samples, ``true_rows`` the ``StereoRecord`` of every sample's
    true molecule and ``input_index`` the input every sample came from (each its own without it).

    ``stereocentres_per_molecule(_linker)``  assigned centres per sample (those that touch the linker)
    ``stereo_bonds_per_molecule(_linker)``   assigned stereo double bonds per sample
    ``stereo_undetermined``                  share of all candidates (centres and double bonds) with label 3
    ``chiral_fraction``                      share of samples whose code differs from their mirror image's
    ``stereo_uniqueness``                    distinct ``stereo_code`` among the samples ``uniqueness`` counts / their number
    With ``true_rows``, among the samples whose PLAIN canonical ``code`` equals their true molecule's:
    ``stereo_recovery``                      share with the true molecule's ``stereo_code``
    ``stereo_mirror``                        share with its ``mirror_code`` and not its ``stereo_code``: the wrong enantiomer
    ``stereo_recovered_inputs``              share of ALL inputs with at least one stereo-recovered sample
    Every score is 0 where it has nothing to count.  ``recovery``, ``uniqueness`` and the clusters are unchanged by this."""
    n = len(rows)
    share = lambda total: total / n if n else 0.0            # noqa: E731
    candidates = sum(r.candidates for r in rows)
    chosen = [k for k in range(n) if _good(pred[k]) and (true is None or _good(true[k]))]
    out = {'stereocentres_per_molecule': share(sum(r.centres for r in rows)),
           'stereocentres_per_molecule_linker': share(sum(r.centres_linker for r in rows)),
           'stereo_bonds_per_molecule': share(sum(r.double_bonds for r in rows)),
           'stereo_bonds_per_molecule_linker': share(sum(r.double_bonds_linker for r in rows)),
           'stereo_undetermined': sum(r.undetermined for r in rows) / candidates if candidates else 0.0,
           'chiral_fraction': share(sum(1 for r in rows if r.chiral)),
           'stereo_uniqueness': len({rows[k].stereo_code for k in chosen}) / len(chosen) if chosen else 0.0}
    if true_rows is None:
        return out
    if len(true_rows) != n or (input_index is not None and len(input_index) != n):
        raise ValueError(f'{n} samples, {len(true_rows)} true records')
    input_index = list(range(n)) if input_index is None else list(input_index)
    same = [k for k in range(n) if rows[k].code == true_rows[k].code]
    hit = [k for k in same if rows[k].stereo_code == true_rows[k].stereo_code]
    mirror = [k for k in same if rows[k].stereo_code == true_rows[k].mirror_code and rows[k].stereo_code != true_rows[k].stereo_code]
    out['stereo_recovery'] = len(hit) / len(same) if same else 0.0
    out['stereo_mirror'] = len(mirror) / len(same) if same else 0.0
    out['stereo_recovered_inputs'] = len({input_index[k] for k in hit}) / len(set(input_index)) if n else 0.0
    return out


def write_stereo_json(path, files, records):
    """``stereo.json``: one object per written file (``files``: its name as the other reports give it), keys ``STEREO_JSON``."""
    import json
    with open(path, 'w') as f:
        json.dump([dict(file=name, **{key: getattr(record, key) for key in STEREO_JSON}) for name, record in zip(files, records)],
                  f, indent=1)
