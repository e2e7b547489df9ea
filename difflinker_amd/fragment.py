"""Linker-design examples from molecules: matched-pair double cuts (``dl_fragment_cuts``) and cuts at three to five bonds
(``dl_fragment_multicuts``) on the HIP device (``csrc/fragment.hip``), and their assembly into the per-example dicts
``ZincDataset`` loads.

In place of the reference's two RDKit steps: fragmentation by ``FragmentMol`` with ``minCuts = maxCuts = 2`` and DeLinker's
pattern (``data/geom/generate_geom_multifrag.py:199-206``), and the re-assembly of fragments, linker and anchors per example
(``data/zinc/prepare_dataset.py``, ``src/datasets.py:56-100``).  Not here: SMILES (symmetric cuts are not merged: every kept
pair is its own example), conformers, BRICS, aromaticity perception, hydrogens.  Pockets around the molecules:
``difflinker_amd.pocket``.

``multi_cuts`` / ``multi_all`` / ``multi_examples`` are the same three steps for the reference's MULTI-fragment sets
(``fragment_by_mmpa(min_cuts=3, max_cuts=5, min_frag_size=3)`` on molecules of at most 40 atoms with three rings,
``data/geom/generate_geom_multifrag.py:227-231``): one linker joined to three, four or five fragments.  Their rule is stated in
``include/difflinker_hip.h`` and restated in ``tests/multicut_ref.py``; no run of the reference pins it."""
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import _lib, const

Cuts = namedtuple('Cuts', 'n_atoms n_bonds n_cuttable n_cuts status bond_side cuts labels')
CUT_FIELDS = ('e1', 'e2', 'anchor_1', 'exit_1', 'anchor_2', 'exit_2', 'n_frag_1', 'n_frag_2', 'n_linker', 'path_atoms')
FRAGMENT_1, FRAGMENT_2, LINKER, NO_ATOM = 0, 1, 2, 255           # values of ``Cuts.labels``
MultiCuts = namedtuple('MultiCuts', 'n_atoms n_bonds n_cuttable n_cuts status n_cuts_k cuts labels')
MULTI_E, MULTI_ANCHOR, MULTI_EXIT, MULTI_N_FRAG = 2, 7, 12, 17   # where the rows of five start in a record: k, n_linker, 4 x 5
MULTI_LINKER = _lib.DL_FRAG_MULTI_LINKER                         # value of ``MultiCuts.labels``; fragment q is q


def fragment_cuts(one_hot, node_mask, bonds, n_bonds, *, charge=None, is_geom, capacity, min_linker=3, min_fragment=5,
                  min_path_atoms=2, linker_leq_frags=True, status=None):
    """``dl_fragment_cuts`` on a batch: ``one_hot [B,N,nf]``, ``node_mask [B,N]`` or ``[B,N,1]``, ``bonds [B,E,3]`` int32 rows
    ``(i, j, order)`` with ``n_bonds [B]`` in the layout of ``perceive_bonds``, ``charge [B,N]`` formal charges by row (None:
    all 0), ``status [B]`` the status of ``perceive_bonds`` to carry forward (None: 0).  ``capacity`` is ``R``, the records
    kept per molecule.  Device tensors in, a ``Cuts`` of device tensors out, no host synchronisation.

    THE RULE.  Atom ``k`` is the k-th row with ``node_mask != 0``, its type the first largest entry of its ``one_hot`` row.
    An entry is a bond when ``0 <= i, j < atoms``, ``i != j`` and ``1 <= order <= 4`` (4: aromatic), in either orientation;
    any other entry is skipped and sets ``DL_FRAG_BAD_BOND``; a repeated pair counts once, as its first entry, and sets it too.
    A bond is CUTTABLE when its order is 1, it lies in no ring, and at least one end is a carbon of charge 0 without an
    order-2 or order-3 bond to a non-carbon atom.  The molecule must be one piece (otherwise ``DL_FRAG_DISCONNECTED`` and no
    cuts).  Every pair of cuttable bonds ``e1 < e2`` (list positions) splits it into fragment 1 beyond ``e1``, fragment 2
    beyond ``e2`` and the linker that touches both; ``anchor_k`` is the fragment atom of bond ``e_k``, ``exit_k`` its linker
    atom, ``path_atoms`` the atoms on the shortest path from ``exit_1`` to ``exit_2``, both counted.  A pair is KEPT when
    ``n_linker >= min_linker``, both fragments have ``min_fragment`` atoms, ``path_atoms >= min_path_atoms`` and, with
    ``linker_leq_frags``, ``n_linker <= min(n_frag_1, n_frag_2)``; the defaults are DeLinker's.  Kept pairs are numbered in
    lexicographic order of ``(e1, e2)``.

    ``n_atoms``, ``n_bonds`` (distinct pairs), ``n_cuttable``, ``n_cuts`` (ALL kept pairs, also beyond ``capacity``),
    ``status`` are int32 ``[B]``; ``bond_side [B,E]``: for the first entry of a cuttable bond the atoms on the side of its
    atom ``i``, else 0; ``cuts [B,R,10]``: ``CUT_FIELDS`` of the first ``min(n_cuts, R)`` kept pairs, zeros after them;
    ``labels`` uint8 ``[B,R,N]`` by atom number: 0 fragment 1, 1 fragment 2, 2 linker, 255 from the atom count on and in unused
    records.  More than 256 atoms: ``DL_FRAG_TOO_LARGE`` and nothing but ``n_atoms``."""
    _lib.require_device('fragment_cuts', one_hot=one_hot, node_mask=node_mask, bonds=bonds, n_bonds=n_bonds, charge=charge,
                        status=status)
    if one_hot.dim() != 3 or bonds.dim() != 3 or bonds.shape[2] != 3:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, bonds {tuple(bonds.shape)}')
    B, N, nf = one_hot.shape
    E, R = bonds.shape[1], int(capacity)
    if node_mask.numel() != B * N or bonds.shape[0] != B or n_bonds.numel() != B or R < 0 or \
            any(t is not None and t.numel() != n for t, n in ((charge, B * N), (status, B))):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}, '
                         f'bonds {tuple(bonds.shape)}, n_bonds {tuple(n_bonds.shape)}, capacity {capacity}')
    dev = one_hot.device
    one_hot, node_mask = _lib.dense(one_hot, dev, torch.float32), _lib.dense(node_mask, dev, torch.float32)
    bonds, n_bonds, charge, status = (_lib.dense(t, dev, torch.int32) for t in (bonds, n_bonds, charge, status))
    i32 = partial(_lib.empty_i32, dev)
    out = Cuts(i32(B), i32(B), i32(B), i32(B), i32(B), i32(B, E), i32(B, R, _lib.DL_FRAG_CUT_FIELDS),
               torch.empty((B, R, N), dtype=torch.uint8, device=dev))
    args = _lib.DLFragmentArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), charge=_lib.ptr(charge),
        carbon_type=(const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX)['C'], capacity=E, n_bonds_in=n_bonds.data_ptr(),
        bonds=bonds.data_ptr() if E else None, status_in=_lib.ptr(status), min_linker=int(min_linker),
        min_fragment=int(min_fragment), min_path_atoms=int(min_path_atoms), linker_leq_frags=int(bool(linker_leq_frags)), R=R,
        n_atoms=out.n_atoms.data_ptr(), n_bonds=out.n_bonds.data_ptr(), n_cuttable=out.n_cuttable.data_ptr(),
        n_cuts=out.n_cuts.data_ptr(), status=out.status.data_ptr(),
        bond_side=out.bond_side.data_ptr() if E else None, cuts=out.cuts.data_ptr() if R else None,
        labels=out.labels.data_ptr() if R else None)
    _lib.launch('dl_fragment_cuts', args, dev)
    return out


def fragment_all(one_hot, node_mask, bonds, n_bonds, *, is_geom, capacity=64, **rule):
    """``fragment_cuts`` whose records hold every kept cut of every molecule: while a molecule is truncated the launch is
    repeated with the largest ``n_cuts`` as capacity (one repeat: ``n_cuts`` does not depend on the capacity).  Reads
    ``n_cuts`` on the host, so it synchronises."""
    found = fragment_cuts(one_hot, node_mask, bonds, n_bonds, is_geom=is_geom, capacity=capacity, **rule)
    most = int(found.n_cuts.max()) if found.n_cuts.numel() else 0
    if most > found.cuts.shape[1]:
        found = fragment_cuts(one_hot, node_mask, bonds, n_bonds, is_geom=is_geom, capacity=most, **rule)
    return found


def examples(result, symbols, positions, names, is_geom, with_rows=False):
    """One dict per kept cut of a ``Cuts`` (on the host), exactly as the reference builds it (``src/datasets.py:88-98``):
    atoms reordered fragment 1, fragment 2, linker, each in atom order; ``uuid`` (running number), ``name``, ``positions``
    ``[n,3]``, ``one_hot [n,types]``, ``charges [n]`` (the atomic numbers of ``const``), ``anchors [n]`` (1 at the two
    anchors), ``fragment_mask``, ``linker_mask`` (fp32 tensors) and ``num_atoms``.  ``symbols[b]``, ``positions[b]`` and
    ``names[b]`` describe molecule ``b`` by atom number.  With ``with_rows`` returns ``(dicts, rows)``: ``rows[k]`` is
    ``(molecule index, anchor_1, anchor_2, n_frag_1, n_frag_2, n_linker)`` of example ``k``, the anchors in the NEW order:
    what the reference keeps in ``<prefix>_table.csv``."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    number = const.GEOM_CHARGES if is_geom else const.CHARGES
    n_cuts, cuts, labels = (torch.as_tensor(t).cpu().numpy() for t in (result.n_cuts, result.cuts, result.labels))
    if int((n_cuts > cuts.shape[1]).sum()):
        raise ValueError(f'{int((n_cuts > cuts.shape[1]).sum())} molecules have more cuts than the {cuts.shape[1]} records '
                         'hold: use fragment_all')
    data, rows = [], []
    for b in range(len(n_cuts)):
        n = len(symbols[b])
        pos = np.asarray(positions[b], dtype=np.float64).reshape(n, 3)
        one_hot = np.zeros((n, len(atom2idx)))
        one_hot[np.arange(n), [atom2idx[s] for s in symbols[b]]] = 1
        charges = np.array([number[s] for s in symbols[b]], dtype=np.float64)
        for r in range(int(n_cuts[b])):
            label = labels[b, r, :n]
            order = np.concatenate([np.nonzero(label == part)[0] for part in (FRAGMENT_1, FRAGMENT_2, LINKER)])
            if len(order) != n:
                raise ValueError(f'molecule {b} ({names[b]}): the labels of cut {r} cover {len(order)} of {n} atoms')
            new = np.empty(n, dtype=np.int64)
            new[order] = np.arange(n)
            anchors = np.zeros(n)
            anchors[new[cuts[b, r, 2]]] = 1
            anchors[new[cuts[b, r, 4]]] = 1
            linker = (label[order] == LINKER).astype(np.float64)
            tensor = lambda v: torch.tensor(v, dtype=const.TORCH_FLOAT)                            # noqa: E731
            data.append({'uuid': len(data), 'name': names[b], 'positions': tensor(pos[order]), 'one_hot': tensor(one_hot[order]),
                         'charges': tensor(charges[order]), 'anchors': tensor(anchors), 'fragment_mask': tensor(1 - linker),
                         'linker_mask': tensor(linker), 'num_atoms': n})
            rows.append((b, int(new[cuts[b, r, 2]]), int(new[cuts[b, r, 4]]), int(cuts[b, r, 6]), int(cuts[b, r, 7]),
                         int(cuts[b, r, 8])))
    return (data, rows) if with_rows else data


def multi_cuts(one_hot, node_mask, bonds, n_bonds, *, charge=None, is_geom, capacity, min_cuts=3, max_cuts=5, min_linker=3,
               min_fragment=3, max_atoms=40, min_rings=3, status=None):
    """``dl_fragment_multicuts`` on a batch; the inputs are those of ``fragment_cuts``.  Device tensors in, a ``MultiCuts`` of
    device tensors out, no host synchronisation.

    THE RULE.  Atoms, bonds, cuttable bonds, ``DL_FRAG_BAD_BOND``, ``DL_FRAG_DISCONNECTED`` and ``DL_FRAG_TOO_LARGE`` are those
    of ``fragment_cuts``.  A molecule is cut only when ``n_atoms <= max_atoms`` and ``n_bonds - n_atoms + 1 >= min_rings``
    (a gate sets no status bit); with more than 64 cuttable bonds it sets ``DL_FRAG_MANY_CUTTABLE`` and is not cut.  A set of
    ``k`` cuttable bonds ``e_1 < ... < e_k``, ``min_cuts <= k <= max_cuts`` within 3..5, is a STAR when one of the ``k + 1``
    pieces left without them touches all ``k``: the linker.  Fragment ``q`` is the piece beyond ``e_q``, ``anchor_q`` its atom
    of that bond and ``exit_q`` the linker's.  A star is KEPT when ``n_linker >= min_linker`` and every fragment has
    ``min_fragment`` atoms; the defaults are the reference's.  Kept stars are numbered by ``k``, then in lexicographic order.

    ``n_cuts`` counts ALL kept stars, ``n_cuts_k [B,3]`` those of 3, 4 and 5 bonds; ``cuts [B,R,22]``: ``k, n_linker, e[5],
    anchor[5], exit[5], n_frag[5]`` with -1 in the slots from ``k`` on, zeros in unused records; ``labels`` uint8 ``[B,R,N]``:
    ``q`` for fragment ``q``, 5 for the linker, 255 from the atom count on and in unused records."""
    _lib.require_device('multi_cuts', one_hot=one_hot, node_mask=node_mask, bonds=bonds, n_bonds=n_bonds, charge=charge,
                        status=status)
    if one_hot.dim() != 3 or bonds.dim() != 3 or bonds.shape[2] != 3:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, bonds {tuple(bonds.shape)}')
    B, N, nf = one_hot.shape
    E, R = bonds.shape[1], int(capacity)
    if node_mask.numel() != B * N or bonds.shape[0] != B or n_bonds.numel() != B or R < 0 or \
            any(t is not None and t.numel() != n for t, n in ((charge, B * N), (status, B))):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, node_mask {tuple(node_mask.shape)}, '
                         f'bonds {tuple(bonds.shape)}, n_bonds {tuple(n_bonds.shape)}, capacity {capacity}')
    dev = one_hot.device
    one_hot, node_mask = _lib.dense(one_hot, dev, torch.float32), _lib.dense(node_mask, dev, torch.float32)
    bonds, n_bonds, charge, status = (_lib.dense(t, dev, torch.int32) for t in (bonds, n_bonds, charge, status))
    i32 = partial(_lib.empty_i32, dev)
    out = MultiCuts(i32(B), i32(B), i32(B), i32(B), i32(B), i32(B, 3), i32(B, R, _lib.DL_FRAG_MULTI_FIELDS),
                    torch.empty((B, R, N), dtype=torch.uint8, device=dev))
    args = _lib.DLFragmentMultiArgs(
        B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), charge=_lib.ptr(charge),
        carbon_type=(const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX)['C'], capacity=E, n_bonds_in=n_bonds.data_ptr(),
        bonds=bonds.data_ptr() if E else None, status_in=_lib.ptr(status), min_cuts=int(min_cuts), max_cuts=int(max_cuts),
        min_linker=int(min_linker), min_fragment=int(min_fragment), max_atoms=int(max_atoms), min_rings=int(min_rings), R=R,
        n_atoms=out.n_atoms.data_ptr(), n_bonds=out.n_bonds.data_ptr(), n_cuttable=out.n_cuttable.data_ptr(),
        n_cuts=out.n_cuts.data_ptr(), status=out.status.data_ptr(), n_cuts_k=out.n_cuts_k.data_ptr(),
        cuts=out.cuts.data_ptr() if R else None, labels=out.labels.data_ptr() if R else None)
    _lib.launch('dl_fragment_multicuts', args, dev)
    return out


def multi_all(one_hot, node_mask, bonds, n_bonds, *, is_geom, capacity=64, **rule):
    """``multi_cuts`` whose records hold every kept star of every molecule: widened once to the largest ``n_cuts``, like
    ``fragment_all``.  Reads ``n_cuts`` on the host, so it synchronises."""
    found = multi_cuts(one_hot, node_mask, bonds, n_bonds, is_geom=is_geom, capacity=capacity, **rule)
    most = int(found.n_cuts.max()) if found.n_cuts.numel() else 0
    if most > found.cuts.shape[1]:
        found = multi_cuts(one_hot, node_mask, bonds, n_bonds, is_geom=is_geom, capacity=most, **rule)
    return found


def multi_examples(result, symbols, positions, names, is_geom, with_rows=False):
    """One dict per kept star of a ``MultiCuts`` (on the host), with the keys of ``examples`` and the atoms reordered fragment 0,
    ..., fragment k-1, linker, each in atom order, as the reference builds its multi-fragment examples (``src/datasets.py:88-98``,
    ``data/geom/prepare_geom_dataset.py:270-298``); ``anchors`` has ``k`` ones.  With ``with_rows`` returns ``(dicts, rows)``:
    ``rows[r]`` is ``(molecule index, k, anchors, fragment sizes, n_linker)``, the anchors a tuple in the NEW order."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    number = const.GEOM_CHARGES if is_geom else const.CHARGES
    n_cuts, cuts, labels = (torch.as_tensor(t).cpu().numpy() for t in (result.n_cuts, result.cuts, result.labels))
    if int((n_cuts > cuts.shape[1]).sum()):
        raise ValueError(f'{int((n_cuts > cuts.shape[1]).sum())} molecules have more cuts than the {cuts.shape[1]} records '
                         'hold: use multi_all')
    data, rows = [], []
    for b in range(len(n_cuts)):
        n = len(symbols[b])
        pos = np.asarray(positions[b], dtype=np.float64).reshape(n, 3)
        one_hot = np.zeros((n, len(atom2idx)))
        one_hot[np.arange(n), [atom2idx[s] for s in symbols[b]]] = 1
        charges = np.array([number[s] for s in symbols[b]], dtype=np.float64)
        for r in range(int(n_cuts[b])):
            k, label = int(cuts[b, r, 0]), labels[b, r, :n]
            order = np.concatenate([np.nonzero(label == part)[0] for part in list(range(k)) + [MULTI_LINKER]])
            if len(order) != n:
                raise ValueError(f'molecule {b} ({names[b]}): the labels of cut {r} cover {len(order)} of {n} atoms')
            new = np.empty(n, dtype=np.int64)
            new[order] = np.arange(n)
            at = tuple(int(new[a]) for a in cuts[b, r, MULTI_ANCHOR:MULTI_ANCHOR + k])
            anchors = np.zeros(n)
            anchors[list(at)] = 1
            linker = (label[order] == MULTI_LINKER).astype(np.float64)
            tensor = lambda v: torch.tensor(v, dtype=const.TORCH_FLOAT)                            # noqa: E731
            data.append({'uuid': len(data), 'name': names[b], 'positions': tensor(pos[order]), 'one_hot': tensor(one_hot[order]),
                         'charges': tensor(charges[order]), 'anchors': tensor(anchors), 'fragment_mask': tensor(1 - linker),
                         'linker_mask': tensor(linker), 'num_atoms': n})
            rows.append((b, k, at, tuple(int(v) for v in cuts[b, r, MULTI_N_FRAG:MULTI_N_FRAG + k]), int(cuts[b, r, 1])))
    return (data, rows) if with_rows else data
