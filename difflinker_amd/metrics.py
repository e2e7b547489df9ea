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
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib, const
from .molecule_builder import perceive_all_bonds

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
    if not (one_hot.is_cuda and node_mask.is_cuda and (drop_mask is None or drop_mask.is_cuda)):
        raise _lib.HipLibraryError('molecule_keys runs on the HIP device only (no CPU fallback): '
                                   f'got tensors on {one_hot.device}, {node_mask.device}')
    B, N, nf = one_hot.shape
    if node_mask.numel() != B * N or (drop_mask is not None and drop_mask.numel() != B * N):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}')
    dev = one_hot.device
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()     # noqa: E731
    one_hot, node_mask = f32(one_hot), f32(node_mask)
    drop_mask = None if drop_mask is None else f32(drop_mask)
    limits = _max_valence(dev, is_geom)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)  # noqa: E731
    out = Analysis(i32(B), i32(B), i32(B), i32(B), i64(B), i64(B, N), i32(B), found)
    capacity = found.bonds.shape[1]
    args = _lib.DLMolKeysArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(),
        drop_mask=None if drop_mask is None else drop_mask.data_ptr(), capacity=capacity,
        n_bonds_in=found.n_bonds.data_ptr(), bonds=found.bonds.data_ptr() if capacity else None,
        valence_in=found.valence.data_ptr(), n_components_in=found.n_components.data_ptr(),
        status_in=found.status.data_ptr(), max_valence=limits.data_ptr(), max_valence_len=limits.numel(),
        n_atoms=out.n_atoms.data_ptr(), n_over=out.n_over.data_ptr(), n_components=out.n_components.data_ptr(),
        n_bonds=out.n_bonds.data_ptr(), key=out.key.data_ptr(), colour=out.colour.data_ptr(), status=out.status.data_ptr())
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().dl_molecule_keys(ctypes.byref(args), stream), 'dl_molecule_keys')
    return out


def analyze(one_hot, x, node_mask, is_geom, drop_mask=None, margins=const.MARGINS_EDM):
    """Bonds, then scores and keys, of every molecule of a batch on the HIP device: ``one_hot [B,N,nf]``, ``x [B,N,3]``,
    ``node_mask`` and the optional ``drop_mask`` (the pocket atoms of a pocket model) ``[B,N,1]`` or ``[B,N]``.

    Returns an ``Analysis`` of device tensors: ``n_atoms``, ``n_over``, ``n_components``, ``n_bonds`` (int32 ``[B]``, all over the
    atoms that are not dropped), ``key`` (int64 ``[B]``: the 64 bits of the key), ``colour`` (int64 ``[B,N]`` by atom number, 0
    for dropped atoms and beyond the atom count), ``status`` (int32 ``[B]``: ``_lib.DL_BONDS_*`` / ``_lib.DL_KEYS_*`` bits) and
    ``bonds``, the ``perceive_all_bonds`` result it was computed from.  The bond list is never cut short
    (``perceive_all_bonds`` widens it), and nothing synchronises beyond what that call does."""
    if not (one_hot.is_cuda and x.is_cuda and node_mask.is_cuda):
        raise _lib.HipLibraryError('analyze runs on the HIP device only (no CPU fallback): '
                                   f'got tensors on {one_hot.device}, {x.device}, {node_mask.device}')
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
