"""``python -m difflinker_amd.prepare``: a linker-design data set from an SDF of 3D molecules, without RDKit.

    python -m difflinker_amd.prepare --sdf mols.sdf --out DIR --prefix NAME [--geom] [--min_linker 3 --min_fragment 5
        --min_path_atoms 2 --no_linker_leq_frags] [--max_per_molecule K] [--val_fraction F --seed S] [--device cuda:0]

The molecules are batched, padded to the batch's largest, and cut by one ``dl_fragment_cuts`` launch per batch
(``fragment.fragment_all``); every kept double cut becomes one example (``fragment.examples``).  ``DIR/NAME.pt`` is the list of
dicts ``ZincDataset`` loads, here and in the reference; ``DIR/NAME_table.csv`` has the columns ``uuid, molecule, anchor_1,
anchor_2, n_frag_1, n_frag_2, n_linker``.  With ``--val_fraction`` the MOLECULES are split, so that no molecule feeds both
``NAME_train`` and ``NAME_val``.  In place of ``data/geom/generate_geom_multifrag.py`` (its double cuts only) and
``data/zinc/prepare_dataset.py``; see ``fragment`` for what this is not."""
import argparse
import csv
import json
import os
import random

import torch

from . import _lib, const
from .fragment import examples, fragment_all
from .io import read_sdf_molecules

SKIP_REASONS = ('malformed', 'unknown_element', 'too_large', 'not_one_piece', 'no_3d')
TABLE_COLUMNS = ('uuid', 'molecule', 'anchor_1', 'anchor_2', 'n_frag_1', 'n_frag_2', 'n_linker')


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


def prepare(molecules, is_geom, device, batch_size=256, max_per_molecule=None, **rule):
    """Examples of a list of ``BondedMolecule``: ``(dicts, rows, skipped)``; ``rows`` as ``fragment.examples`` gives them with
    the molecule index into ``molecules``, ``skipped`` a count per reason of ``SKIP_REASONS``."""
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
        one_hot, mask, bonds, n_bonds, charge = pad_batch(batch, is_geom, device)
        found = fragment_all(one_hot, mask, bonds, n_bonds, is_geom=is_geom, charge=charge, **rule)
        skipped['not_one_piece'] += int((found.status & _lib.DL_FRAG_DISCONNECTED != 0).sum())
        got, got_rows = examples(found, [m.symbols for m in batch], [m.positions for m in batch], [m.name for m in batch],
                                 is_geom, with_rows=True)
        taken = {}
        for item, row in zip(got, got_rows):
            taken[row[0]] = taken.get(row[0], 0) + 1
            if max_per_molecule is not None and taken[row[0]] > max_per_molecule:
                continue
            item['uuid'] = len(data)
            data.append(item)
            rows.append((usable[start + row[0]],) + row[1:])
    return data, rows, skipped


def write(out, prefix, data, rows):
    torch.save(data, os.path.join(out, f'{prefix}.pt'))
    with open(os.path.join(out, f'{prefix}_table.csv'), 'w', newline='') as f:
        table = csv.writer(f)
        table.writerow(TABLE_COLUMNS)
        for item, row in zip(data, rows):
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
    args = p.parse_args(argv)

    molecules, malformed = read_sdf_molecules(args.sdf)
    data, rows, skipped = prepare(molecules, args.geom, torch.device(args.device), args.batch_size, args.max_per_molecule,
                                  min_linker=args.min_linker, min_fragment=args.min_fragment,
                                  min_path_atoms=args.min_path_atoms, linker_leq_frags=not args.no_linker_leq_frags)
    skipped['malformed'] = malformed
    os.makedirs(args.out, exist_ok=True)
    summary = {'molecules_read': len(molecules) + malformed, 'molecules_skipped': skipped, 'examples': len(data),
               'molecules_with_examples': len({row[0] for row in rows}), 'files': {}}
    if args.val_fraction > 0:
        order = sorted({row[0] for row in rows})
        random.Random(args.seed).shuffle(order)
        held_out = set(order[:int(round(args.val_fraction * len(order)))])
        for name, wanted in (('train', False), ('val', True)):
            part = [(dict(item), row) for item, row in zip(data, rows) if (row[0] in held_out) == wanted]
            for uuid, (item, _) in enumerate(part):
                item['uuid'] = uuid
            write(args.out, f'{args.prefix}_{name}', [item for item, _ in part], [row for _, row in part])
            summary['files'][f'{args.prefix}_{name}'] = len(part)
    else:
        write(args.out, args.prefix, data, rows)
        summary['files'][args.prefix] = len(data)
    print(json.dumps(summary))
    return summary


if __name__ == '__main__':
    main()
