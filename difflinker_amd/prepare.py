"""``python -m difflinker_amd.prepare``: a linker-design data set from an SDF of 3D molecules, without RDKit or Bio.PDB.

    python -m difflinker_amd.prepare --sdf mols.sdf --out DIR --prefix NAME [--geom] [--min_linker 3 --min_fragment 5
        --min_path_atoms 2 --no_linker_leq_frags] [--max_per_molecule K] [--val_fraction F --seed S] [--device cuda:0]
        [--proteins PDB_DIR [--pocket_cutoff 6.0] [--pocket_by number|residue]]
        [--multi_cuts MIN MAX [--multi_min_size 3] [--multi_max_atoms 40] [--multi_min_rings 3]]

The molecules are batched, padded to the batch's largest, and cut by one ``dl_fragment_cuts`` launch per batch
(``fragment.fragment_all``); every kept double cut becomes one example (``fragment.examples``).  ``DIR/NAME.pt`` is the list of
dicts ``ZincDataset`` loads, here and in the reference; ``DIR/NAME_table.csv`` has the columns ``uuid, molecule, anchor_1,
anchor_2, n_frag_1, n_frag_2, n_linker``.  With ``--val_fraction`` the MOLECULES are split, so that no molecule feeds both
``NAME_train`` and ``NAME_val``.  In place of ``data/geom/generate_geom_multifrag.py`` (its double cuts only) and
``data/zinc/prepare_dataset.py``; see ``fragment`` for what this is not.

With ``--proteins PDB_DIR`` the set is pocket-conditioned (``--geom`` is implied: pocket models use the GEOM vocabulary).  The
protein of a record is ``PDB_DIR/<code>_protein.pdb`` with ``code = name.split('_')[0]``, the reference's convention; every
protein is parsed ONCE per run (``io.read_pdb_arrays``), and the pocket of every ligand - the residues with an atom within
``--pocket_cutoff`` of one of its atoms - is selected by one ``dl_pocket_select`` launch per batch (``pocket.select_all``).
``DIR/NAME_full.pt`` and ``DIR/NAME_bb.pt`` are the lists ``MOADDataset`` loads as ``NAME.full`` and ``NAME.bb``, and the table
gains the reference's columns ``pocket_full_size, pocket_bb_size, molecule_size, fragments_size, linker_size``.  In place of
``data/pocket/prepare_dataset.py`` and ``MOADDataset.preprocess``; see ``pocket`` for what this is not.

With ``--multi_cuts MIN MAX`` (3 <= MIN <= MAX <= 5) the run writes the MULTI-fragment set only, as
``data/geom/generate_geom_multifrag.py:227-231`` does: every molecule of at most ``--multi_max_atoms`` atoms with at least
``--multi_min_rings`` rings (the cyclomatic number) is cut at MIN to MAX bonds by one ``dl_fragment_multicuts`` launch per batch
(``fragment.multi_all``), a linker and every fragment of at least ``--multi_min_size`` atoms; the double-cut options do not
apply.  Every kept star becomes one example (``fragment.multi_examples``), and the table has the columns ``uuid, molecule,
n_cuts, anchors, n_frags, n_linker``, the anchors and the fragment sizes joined by ``-`` like the reference's ``anchors``."""
import argparse
import csv
import json
import os
import random
import time

import numpy as np
import torch

from . import _lib, const
from .fragment import examples, fragment_all, multi_all, multi_examples
from .io import groups, read_pdb_arrays, read_sdf_molecules
from .pocket import DEAD, pocket_atoms, pocket_examples, select_all

SKIP_REASONS = ('malformed', 'unknown_element', 'too_large', 'not_one_piece', 'no_3d')
POCKET_SKIP_REASONS = ('no_protein_file', 'empty_pocket')         # with --proteins, beside SKIP_REASONS
TABLE_COLUMNS = ('uuid', 'molecule', 'anchor_1', 'anchor_2', 'n_frag_1', 'n_frag_2', 'n_linker')
MULTI_TABLE_COLUMNS = ('uuid', 'molecule', 'n_cuts', 'anchors', 'n_frags', 'n_linker')    # with --multi_cuts
POCKET_TABLE_COLUMNS = TABLE_COLUMNS + ('pocket_full_size', 'pocket_bb_size', 'molecule_size', 'fragments_size', 'linker_size')


def pad_batch(molecules, is_geom, device):
    """``(one_hot [B,N,nf], node_mask [B,N], bonds [B,E,3], n_bonds [B], charge [B,N])`` of a list of ``BondedMolecule``,
    padded to the largest of the batch, on ``device``."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    B = len(molecules)
    N = max(max(len(m) for m in molecules), 1)
    E = max(max(len(m.bonds) for m in molecules), 1)
    one_hot, mask = torch.zeros(B, N, len(atom2idx)), torch.zeros(B, N)
    bonds, n_bonds = torch.zeros(B, E, 3, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    charge = torch.zeros(B, N, dtype=torch.int32)
    for b, m in enumerate(molecules):
        n = len(m)
        one_hot[b, torch.arange(n), torch.tensor([atom2idx[s] for s in m.symbols], dtype=torch.long)] = 1
        mask[b, :n] = 1
        charge[b, :n] = torch.tensor(m.charges, dtype=torch.int32)
        if m.bonds:
            bonds[b, :len(m.bonds)] = torch.tensor(m.bonds, dtype=torch.int32)
        n_bonds[b] = len(m.bonds)
    return tuple(t.to(device) for t in (one_hot, mask, bonds, n_bonds, charge))


class _Clock:
    """Seconds per named share of a run; ``device`` is synchronised before a reading, so a share holds its launches."""

    def __init__(self, device, seconds):
        self.device, self.seconds = device, seconds

    def lap(self, share, since):
        if self.seconds is None:
            return since
        if torch.device(self.device).type == 'cuda':
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.seconds[share] = self.seconds.get(share, 0.0) + now - since
        return now


def prepare(molecules, is_geom, device, batch_size=256, max_per_molecule=None, seconds=None, multi=False, **rule):
    """Examples of a list of ``BondedMolecule``: ``(dicts, rows, skipped)``; ``rows`` as ``fragment.examples`` gives them with
    the molecule index into ``molecules``, ``skipped`` a count per reason of ``SKIP_REASONS``.  A dict given as ``seconds``
    gathers the time of the shares ``'gpu'`` (upload, launches, until the device is idle) and ``'assembly'``.  With ``multi``
    the cuts are those of ``fragment.multi_all``, ``rule`` is its rule and the rows are those of ``fragment.multi_examples``."""
    cut_all, assemble = (multi_all, multi_examples) if multi else (fragment_all, examples)
    clock = _Clock(device, seconds)
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    skipped = {reason: 0 for reason in SKIP_REASONS}
    usable = []
    for index, m in enumerate(molecules):
        if any(s not in atom2idx for s in m.symbols):
            skipped['unknown_element'] += 1
        elif len(m) > _lib.DL_FRAG_MAX_ATOMS:
            skipped['too_large'] += 1
        elif not m.is_3d:
            skipped['no_3d'] += 1
        else:
            usable.append(index)
    data, rows = [], []
    for start in range(0, len(usable), batch_size):
        batch = [molecules[i] for i in usable[start:start + batch_size]]
        began = time.perf_counter()
        one_hot, mask, bonds, n_bonds, charge = pad_batch(batch, is_geom, device)
        found = cut_all(one_hot, mask, bonds, n_bonds, is_geom=is_geom, charge=charge, **rule)
        began = clock.lap('gpu', began)
        skipped['not_one_piece'] += int((found.status & _lib.DL_FRAG_DISCONNECTED != 0).sum())
        got, got_rows = assemble(found, [m.symbols for m in batch], [m.positions for m in batch], [m.name for m in batch],
                                 is_geom, with_rows=True)
        taken = {}
        for item, row in zip(got, got_rows):
            taken[row[0]] = taken.get(row[0], 0) + 1
            if max_per_molecule is not None and taken[row[0]] > max_per_molecule:
                continue
            item['uuid'] = len(data)
            data.append(item)
            rows.append((usable[start + row[0]],) + row[1:])
        clock.lap('assembly', began)
    return data, rows, skipped


def protein_path(directory, name):
    """``DIR/<code>_protein.pdb`` of the record ``name``, ``code`` its part before the first underscore."""
    return os.path.join(directory, f"{name.split('_')[0]}_protein.pdb")


def select_ligand_pockets(ligands, proteins, which, device, cutoff=6.0, by='number', batch_size=256):
    """Pocket atoms of every ligand: ``ligands[k]`` is a ``[n,3]`` array of fp64 positions, ``proteins`` a list of
    ``io.PdbArrays`` and ``which[k]`` the protein of ligand ``k``.  The proteins go to the device once, the pairs in batches of
    ``batch_size`` through ``pocket.select_all``.  Returns a list of int64 arrays: the positions within its protein of the
    pocket atoms of every ligand, in file order."""
    sizes = [len(p.resseq) for p in proteins]
    offset = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=device)
    protein_x = torch.from_numpy(np.concatenate([p.coords for p in proteins] + [np.zeros((0, 3), np.float32)])).to(device)
    group = torch.from_numpy(np.concatenate([groups(p, by) for p in proteins] + [np.zeros(0, np.int32)])).to(device)
    chosen = []
    for start in range(0, len(ligands), batch_size):
        batch = ligands[start:start + batch_size]
        width = max(max(len(x) for x in batch), 1)
        ligand_x, mask = np.zeros((len(batch), width, 3)), np.zeros((len(batch), width), np.float32)
        for b, x in enumerate(batch):
            ligand_x[b, :len(x)] = x
            mask[b, :len(x)] = 1
        found = select_all(protein_x, group, offset, torch.tensor(which[start:start + batch_size], dtype=torch.int32, device=device),
                           torch.from_numpy(ligand_x).to(device), torch.from_numpy(mask).to(device), cutoff=cutoff,
                           max_atoms=max(sizes))
        status, n_pocket, index = (t.cpu().numpy() for t in (found.status, found.n_pocket, found.index))
        if (status & DEAD).any():
            b = int(np.nonzero(status & DEAD)[0][0])
            raise ValueError(f'ligand {start + b}: dl_pocket_select status {int(status[b])} (a coordinate that is no number, more '
                             'than 256 ligand atoms or more than 32768 residues)')
        chosen.extend(index[b, :n_pocket[b]].astype(np.int64) for b in range(len(batch)))
    return chosen


def prepare_pockets(molecules, proteins_dir, device, batch_size=256, max_per_molecule=None, cutoff=6.0, by='number', seconds=None,
                    **rule):
    """Pocket-conditioned examples of a list of ``BondedMolecule``: ``(full, bb, rows, skipped)``.  ``full`` and ``bb`` are the
    dicts of ``pocket.pocket_examples`` with every pocket atom and with the backbone atoms; ``rows`` as ``prepare`` gives them,
    followed by the sizes of the full pocket, the backbone pocket, the molecule, both fragments and the linker; ``skipped``
    counts MOLECULES per reason of ``SKIP_REASONS`` and ``POCKET_SKIP_REASONS``.  A dict given as ``seconds`` gathers the shares
    ``'parse'`` (the proteins), ``'gpu'`` and ``'assembly'`` of the run."""
    clock = _Clock(device, seconds)
    with_file = [k for k, m in enumerate(molecules) if os.path.exists(protein_path(proteins_dir, m.name))]
    data, rows, skipped = prepare([molecules[k] for k in with_file], True, device, batch_size, max_per_molecule, seconds, **rule)
    skipped.update(no_protein_file=len(molecules) - len(with_file), empty_pocket=0)
    rows = [(with_file[row[0]],) + row[1:] for row in rows]
    began = time.perf_counter()
    ligands = sorted({row[0] for row in rows})                   # the molecules that gave examples
    paths = sorted({protein_path(proteins_dir, molecules[k].name) for k in ligands})
    proteins = [read_pdb_arrays(path) for path in paths]          # every protein ONCE
    began = clock.lap('parse', began)
    chosen = {}
    if ligands:
        which = [paths.index(protein_path(proteins_dir, molecules[k].name)) for k in ligands]
        found = select_ligand_pockets([molecules[k].positions for k in ligands], proteins, which, device, cutoff, by, batch_size)
        chosen = {k: (proteins[p], idx) for k, p, idx in zip(ligands, which, found)}
    began = clock.lap('gpu', began)
    pockets = {}
    for k, (protein, idx) in chosen.items():
        names, elements = [protein.name[j] for j in idx], [protein.element[j] for j in idx]
        pockets[k] = tuple(pocket_atoms(protein.coords[idx], names, elements, mode) for mode in ('full', 'bb'))
        if not len(pockets[k][0][2]) or not len(pockets[k][1][2]):
            skipped['empty_pocket'] += 1
            del pockets[k]
    kept = [(dict(item, uuid=uuid), row) for uuid, (item, row) in
            enumerate((item, row) for item, row in zip(data, rows) if row[0] in pockets)]
    full = pocket_examples([item for item, _ in kept], [pockets[row[0]][0] for _, row in kept])
    bb = pocket_examples([item for item, _ in kept], [pockets[row[0]][1] for _, row in kept])
    rows = [row + (len(pockets[row[0]][0][2]), len(pockets[row[0]][1][2]), item['num_atoms'], row[3] + row[4], row[5])
            for item, row in kept]
    clock.lap('assembly', began)
    return full, bb, rows, skipped


def write(out, prefix, data, rows, bb=None, multi=False):
    """``prefix.pt`` and ``prefix_table.csv``; with ``bb`` (a pocket set) ``prefix_full.pt`` and ``prefix_bb.pt`` instead; with
    ``multi`` the rows are those of ``fragment.multi_examples`` and the table has ``MULTI_TABLE_COLUMNS``."""
    if bb is None:
        torch.save(data, os.path.join(out, f'{prefix}.pt'))
    else:
        torch.save(data, os.path.join(out, f'{prefix}_full.pt'))
        torch.save(bb, os.path.join(out, f'{prefix}_bb.pt'))
    with open(os.path.join(out, f'{prefix}_table.csv'), 'w', newline='') as f:
        table = csv.writer(f)
        table.writerow(MULTI_TABLE_COLUMNS if multi else TABLE_COLUMNS if bb is None else POCKET_TABLE_COLUMNS)
        for item, row in zip(data, rows):
            if multi:
                row = (row[0], row[1], '-'.join(map(str, row[2])), '-'.join(map(str, row[3])), row[4])
            table.writerow((item['uuid'], item['name']) + tuple(row[1:]))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--sdf', required=True)
    p.add_argument('--out', required=True)
    p.add_argument('--prefix', required=True)
    p.add_argument('--geom', action='store_true', help='the GEOM vocabulary (with P) in place of the ZINC one')
    p.add_argument('--min_linker', type=int, default=3)
    p.add_argument('--min_fragment', type=int, default=5)
    p.add_argument('--min_path_atoms', type=int, default=2)
    p.add_argument('--no_linker_leq_frags', action='store_true', help='keep linkers larger than the smaller fragment')
    p.add_argument('--max_per_molecule', type=int, default=None, help='keep the first K cuts of every molecule')
    p.add_argument('--val_fraction', type=float, default=0.0, help='share of the MOLECULES that goes to NAME_val')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--batch_size', type=int, default=256)
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--proteins', default=None, help='directory of <code>_protein.pdb files: write the pocket-conditioned sets '
                                                    'NAME_full and NAME_bb (GEOM vocabulary)')
    p.add_argument('--pocket_cutoff', type=float, default=6.0, help='a residue with an atom this close to the ligand is pocket')
    p.add_argument('--pocket_by', choices=('number', 'residue'), default='number',
                   help="what is selected as a whole: all atoms with a residue NUMBER (the reference's rule), or one residue "
                        'of one chain')
    p.add_argument('--multi_cuts', type=int, nargs=2, metavar=('MIN', 'MAX'), default=None,
                   help='write the multi-fragment set instead: one linker joined to MIN..MAX fragments, 3 <= MIN <= MAX <= 5')
    p.add_argument('--multi_min_size', type=int, default=3, help='with --multi_cuts: atoms of the linker and of every fragment')
    p.add_argument('--multi_max_atoms', type=int, default=40, help='with --multi_cuts: larger molecules are not cut')
    p.add_argument('--multi_min_rings', type=int, default=3, help='with --multi_cuts: molecules with fewer rings are not cut')
    args = p.parse_args(argv)
    multi = args.multi_cuts is not None
    if multi and args.proteins is not None:
        p.error('--multi_cuts writes no pocket-conditioned sets: it cannot go with --proteins')
    if multi and not _lib.DL_FRAG_MULTI_MIN_CUTS <= args.multi_cuts[0] <= args.multi_cuts[1] <= _lib.DL_FRAG_MULTI_MAX_CUTS:
        p.error(f'--multi_cuts MIN MAX: {_lib.DL_FRAG_MULTI_MIN_CUTS} <= MIN <= MAX <= {_lib.DL_FRAG_MULTI_MAX_CUTS}')

    molecules, malformed = read_sdf_molecules(args.sdf)
    rule = dict(min_linker=args.min_linker, min_fragment=args.min_fragment, min_path_atoms=args.min_path_atoms,
                linker_leq_frags=not args.no_linker_leq_frags)
    bb = None
    if multi:
        data, rows, skipped = prepare(molecules, args.geom, torch.device(args.device), args.batch_size, args.max_per_molecule,
                                      multi=True, min_cuts=args.multi_cuts[0], max_cuts=args.multi_cuts[1],
                                      min_linker=args.multi_min_size, min_fragment=args.multi_min_size,
                                      max_atoms=args.multi_max_atoms, min_rings=args.multi_min_rings)
    elif args.proteins is None:
        data, rows, skipped = prepare(molecules, args.geom, torch.device(args.device), args.batch_size, args.max_per_molecule, **rule)
    else:
        data, bb, rows, skipped = prepare_pockets(molecules, args.proteins, torch.device(args.device), args.batch_size,
                                                  args.max_per_molecule, args.pocket_cutoff, args.pocket_by, **rule)
    skipped['malformed'] = malformed
    os.makedirs(args.out, exist_ok=True)
    summary = {'molecules_read': len(molecules) + malformed, 'molecules_skipped': skipped, 'examples': len(data),
               'molecules_with_examples': len({row[0] for row in rows}), 'files': {}}
    if multi:
        summary['examples_by_cuts'] = {str(k): sum(row[1] == k for row in rows)
                                       for k in range(args.multi_cuts[0], args.multi_cuts[1] + 1)}
    if args.val_fraction > 0:
        order = sorted({row[0] for row in rows})
        random.Random(args.seed).shuffle(order)
        held_out = set(order[:int(round(args.val_fraction * len(order)))])
        for name, wanted in (('train', False), ('val', True)):
            chosen = [k for k, row in enumerate(rows) if (row[0] in held_out) == wanted]
            part, part_bb = ([dict(items[k], uuid=uuid) for uuid, k in enumerate(chosen)] if items is not None else None
                             for items in (data, bb))
            write(args.out, f'{args.prefix}_{name}', part, [rows[k] for k in chosen], part_bb, multi)
            summary['files'][f'{args.prefix}_{name}'] = len(part)
    else:
        write(args.out, args.prefix, data, rows, bb, multi)
        summary['files'][args.prefix] = len(data)
    print(json.dumps(summary))
    return summary


if __name__ == '__main__':
    main()
