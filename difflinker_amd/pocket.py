"""Pockets of a batch of (ligand, protein) pairs on the HIP device (``dl_pocket_select``, ``csrc/pocket.hip``) and their assembly
with ``fragment.examples`` into the per-example dicts ``MOADDataset`` loads.

In place of the pocket half of the reference's preparation: ``get_pocket`` of ``data/pocket/prepare_dataset.py`` (Bio.PDB and a
numpy distance matrix, once per ligand) and ``MOADDataset.preprocess`` (``src/datasets.py:131-222``).  Not here: SMILES and the
matching of table rows to substructures, cuts at three or more bonds, the reference's list of skipped PDB codes, protein cleaning
(``clean_and_split.py``), hydrogens."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, const

Pockets = namedtuple('Pockets', 'n_ligand n_contact_atoms n_groups_selected n_pocket status member index')
CONTACT_ATOM, POCKET_ATOM = 1, 2                                  # bits of ``Pockets.member``
BACKBONE = ('N', 'CA', 'C', 'O')
DEAD = _lib.DL_POCKET_NONFINITE | _lib.DL_POCKET_TOO_LARGE | _lib.DL_POCKET_TOO_MANY_GROUPS | _lib.DL_POCKET_BAD_PROTEIN


def select_pockets(protein_x, protein_group, protein_offset, pair_protein, ligand_x, ligand_mask, *, cutoff=6.0, capacity,
                   max_atoms=None):
    """``dl_pocket_select`` on a batch of pairs.  Proteins are concatenated: ``protein_x [M_total,3]`` (kept in fp32, as Bio.PDB
    keeps coordinates), ``protein_group [M_total]`` dense group ids within each protein (``io.groups``), ``protein_offset
    [P+1]``; pair ``b`` is protein ``pair_protein[b]`` and the rows of ``ligand_x [B,L,3]`` (fp64) with ``ligand_mask [B,L]``
    ``!= 0``.  ``capacity`` is ``R``, the positions kept per pair; ``max_atoms`` the row width of ``member``, at least the
    largest protein (None: ``M_total``, which always is).  Device tensors in, a ``Pockets`` of device tensors out, no host
    synchronisation.

    THE RULE.  With ``dx = (double)xp - xl`` and ``d2 = ((dx*dx) + (dy*dy)) + (dz*dz)`` in fp64, protein atom ``j`` is a CONTACT
    atom when ``d2 <= cutoff * cutoff`` for some ligand atom, a group is SELECTED when it holds a contact atom, and an atom is a
    POCKET atom when its group is selected.

    ``n_ligand``, ``n_contact_atoms``, ``n_groups_selected``, ``n_pocket`` (ALL pocket atoms, also beyond ``capacity``) and
    ``status`` are int32 ``[B]``; ``member`` uint8 ``[B,max_atoms]`` by position within the protein: bit 0 contact atom, bit 1
    pocket atom; ``index [B,R]``: the positions of the first ``min(n_pocket, R)`` pocket atoms in file order, -1 after them.
    ``DL_POCKET_TRUNCATED``: ``n_pocket > R``.  More than 256 ligand atoms (``DL_POCKET_TOO_LARGE``), a group id outside
    ``[0, DL_POCKET_MAX_GROUPS)`` (``_TOO_MANY_GROUPS``), a non-finite coordinate (``_NONFINITE``) or a protein that is not
    there or wider than ``max_atoms`` (``_BAD_PROTEIN``): nothing but ``n_ligand``."""
    _lib.require_device('select_pockets', protein_x=protein_x, protein_group=protein_group, protein_offset=protein_offset,
                        pair_protein=pair_protein, ligand_x=ligand_x, ligand_mask=ligand_mask)
    if protein_x.dim() != 2 or protein_x.shape[1] != 3 or ligand_x.dim() != 3 or ligand_x.shape[2] != 3:
        raise ValueError(f'shapes disagree: protein_x {tuple(protein_x.shape)}, ligand_x {tuple(ligand_x.shape)}')
    M_total, (B, L) = protein_x.shape[0], ligand_x.shape[:2]
    P, R = protein_offset.numel() - 1, int(capacity)
    Mmax = M_total if max_atoms is None else int(max_atoms)
    if protein_group.numel() != M_total or P < 0 or pair_protein.numel() != B or ligand_mask.numel() != B * L or R < 0 or Mmax < 0:
        raise ValueError(f'shapes disagree: protein_x {tuple(protein_x.shape)}, protein_group {tuple(protein_group.shape)}, '
                         f'protein_offset {tuple(protein_offset.shape)}, pair_protein {tuple(pair_protein.shape)}, ligand_x '
                         f'{tuple(ligand_x.shape)}, ligand_mask {tuple(ligand_mask.shape)}, capacity {capacity}, max_atoms {max_atoms}')
    dev = protein_x.device
    protein_x, ligand_mask = _lib.dense(protein_x, dev, torch.float32), _lib.dense(ligand_mask, dev, torch.float32)
    ligand_x = _lib.dense(ligand_x, dev, torch.float64)
    protein_group, protein_offset, pair_protein = (_lib.dense(t, dev, torch.int32)
                                                   for t in (protein_group, protein_offset, pair_protein))
    out = Pockets(*(_lib.empty_i32(dev, B) for _ in range(5)), torch.empty((B, Mmax), dtype=torch.uint8, device=dev),
                  _lib.empty_i32(dev, B, R))
    opt = lambda t: t.data_ptr() if t.numel() else None            # noqa: E731  (NULL for an EMPTY tensor, not for None)
    args = _lib.DLPocketArgs(
        B=B, L=L, P=P, M_total=M_total, protein_x=opt(protein_x), protein_group=opt(protein_group),
        protein_offset=protein_offset.data_ptr(), pair_protein=opt(pair_protein), ligand_x=opt(ligand_x),
        ligand_mask=opt(ligand_mask), cutoff=float(cutoff), Mmax=Mmax, capacity=R, n_ligand=opt(out.n_ligand),
        n_contact_atoms=opt(out.n_contact_atoms), n_groups_selected=opt(out.n_groups_selected), n_pocket=opt(out.n_pocket),
        status=opt(out.status), member=opt(out.member), index=opt(out.index))
    _lib.launch('dl_pocket_select', args, dev)
    return out


def select_all(protein_x, protein_group, protein_offset, pair_protein, ligand_x, ligand_mask, *, cutoff=6.0, capacity=512,
               max_atoms=None):
    """``select_pockets`` whose ``index`` holds every pocket atom of every pair: when a pair is truncated the launch is repeated
    with the largest ``n_pocket`` as capacity (one repeat: ``n_pocket`` does not depend on the capacity).  Reads ``n_pocket`` on
    the host, so it synchronises."""
    found = select_pockets(protein_x, protein_group, protein_offset, pair_protein, ligand_x, ligand_mask, cutoff=cutoff,
                           capacity=capacity, max_atoms=max_atoms)
    most = int(found.n_pocket.max()) if found.n_pocket.numel() else 0
    if most > found.index.shape[1]:
        found = select_pockets(protein_x, protein_group, protein_offset, pair_protein, ligand_x, ligand_mask, cutoff=cutoff,
                               capacity=most, max_atoms=max_atoms)
    return found


def pocket_atoms(positions, names, elements, mode):
    """Of the pocket atoms of one pair (by ``index``: fp32 ``positions [n,3]``, atom ``names`` and ``elements`` as
    ``io.read_pdb_arrays`` gives them) those a data set keeps, as ``io.get_pocket`` keeps them: mode ``'full'`` every atom whose
    element is in the GEOM vocabulary, mode ``'bb'`` of those the ones named N, CA, C, O.  Returns ``(positions [m,3] fp32,
    one_hot [m,types], charges [m])``."""
    from .io import _symbol
    if mode not in ('full', 'bb'):
        raise ValueError(f"pocket mode {mode!r}: 'full' or 'bb'")
    keep, keys = [], []
    for k, (name, element) in enumerate(zip(names, elements)):
        if mode == 'bb' and name not in BACKBONE:
            continue
        key = element if element in const.GEOM_ATOM2IDX else _symbol(element)
        if key in const.GEOM_ATOM2IDX:
            keep.append(k)
            keys.append(key)
    one_hot = np.zeros((len(keep), len(const.GEOM_ATOM2IDX)))
    one_hot[np.arange(len(keep)), [const.GEOM_ATOM2IDX[key] for key in keys]] = 1
    charges = np.array([const.GEOM_CHARGES[key] for key in keys], dtype=np.float64)
    return np.asarray(positions, dtype=np.float32).reshape(-1, 3)[keep], one_hot, charges


def pocket_examples(items, pockets):
    """The dicts of ``MOADDataset.preprocess`` (``src/datasets.py:175-220``) from ``fragment.examples`` dicts (GEOM vocabulary)
    and, for each, its pocket ``(positions, one_hot, charges)`` as ``pocket_atoms`` gives it.  The atoms are reordered fragments,
    pocket, linker; ``fragment_mask`` covers fragments AND pocket, ``fragment_only_mask`` and ``pocket_mask`` one of them each;
    the anchors keep their indices, because the fragments stay in front.  All tensors are ``const.TORCH_FLOAT``."""
    data = []
    for item, (pocket_pos, pocket_one_hot, pocket_charges) in zip(items, pockets):
        linker = item['linker_mask'].bool()
        n_frag, n_link, n_pock = int((~linker).sum()), int(linker.sum()), len(pocket_charges)
        if bool(linker[:n_frag].any()):
            raise ValueError(f"example {item['uuid']} ({item['name']}): the linker atoms do not come last")
        if item['one_hot'].shape[1] != len(const.GEOM_ATOM2IDX):
            raise ValueError(f"example {item['uuid']} ({item['name']}): pocket data sets use the GEOM vocabulary")
        tensor = lambda v: torch.as_tensor(np.asarray(v), dtype=const.TORCH_FLOAT)                                   # noqa: E731
        between = lambda key, middle: torch.cat([item[key][:n_frag], middle, item[key][n_frag:]])                     # noqa: E731
        ones = lambda *counts: torch.cat([torch.full((n,), float(v), dtype=const.TORCH_FLOAT)                          # noqa: E731
                                          for n, v in zip((n_frag, n_pock, n_link), counts)])
        data.append({'uuid': item['uuid'], 'name': item['name'],
                     'positions': between('positions', tensor(pocket_pos).reshape(n_pock, 3)),
                     'one_hot': between('one_hot', tensor(pocket_one_hot).reshape(n_pock, len(const.GEOM_ATOM2IDX))),
                     'charges': between('charges', tensor(pocket_charges).reshape(n_pock)),
                     'anchors': between('anchors', torch.zeros(n_pock, dtype=const.TORCH_FLOAT)),
                     'fragment_only_mask': ones(1, 0, 0), 'pocket_mask': ones(0, 1, 0), 'fragment_mask': ones(1, 1, 0),
                     'linker_mask': ones(0, 0, 1), 'num_atoms': n_frag + n_pock + n_link})
    return data
