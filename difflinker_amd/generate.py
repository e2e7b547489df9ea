"""Generation drivers — the ``main()`` bodies of the reference's ``generate.py`` (:62-167),
``generate_with_pocket.py`` (:116-283) and ``generate_with_protein.py`` (:151-300) as importable functions on top of
``DDPM.sample_chain`` (HIP), ``SizeClassifier`` (HIP) and the RDKit-free I/O of ``io.py``.

Differences from the scripts, all outside the sampling path: the functions return the list of written files instead of
printing, and the ``obabel xyz -> sdf`` conversion (generate.py:179-180) is replaced by ``output_format='sdf'`` /
``'both'``: bonds perceived on the GPU by the reference's own ``molecule_builder`` rule (``molecule_builder.py``, not
OpenBabel's rules) and written by ``io.save_sdf_file``.  The default ``'xyz'`` writes what the scripts write before that call.  ``python -m difflinker_amd.generate --help`` exposes the same
flags as the three scripts (``--pocket`` / ``--protein`` select the pocket-conditioned variants).
"""
import argparse
import json
import os
import random

import numpy as np
import torch

from . import const
from . import metrics as mol_metrics
from .datasets import MOADDataset, collate_with_fragment_edges, collate_with_fragment_without_pocket_edges
from .io import get_pocket, get_protein_atoms, parse_molecule, pocket_arrays, read_molecule, read_pocket, save_sdf_file, save_xyz_file
from .lightning import DDPM
from .linker_size import SizeClassifier
from .molecule_builder import add_hydrogens, perceive_all_bonds, perceive_bonds, refine_bond_orders, relax_samples, summary
from .utils import FoundNaNException


def set_deterministic(seed):
    """src/utils.py:263-271."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def make_sample_fn(linker_size, device, with_pocket=False):
    """``linker_size``: an integer, ``"lo,hi"`` bounds (uniform, inclusive) or the path of a size-predictor checkpoint
    (generate.py:69-99).  A ``SizeClassifier`` instance is accepted in place of the path."""
    if isinstance(linker_size, SizeClassifier):
        size_nn = linker_size.eval().to(device)
        return lambda _data: size_nn.sample_sizes(_data, with_pocket=with_pocket)
    linker_size = str(linker_size)
    if linker_size.isdigit():
        size = int(linker_size)
        return lambda _data: torch.ones(_data['positions'].shape[0], device=device, dtype=const.TORCH_INT) * size
    boundaries = [x.strip() for x in linker_size.split(',')]
    if len(boundaries) == 2 and boundaries[0].isdigit() and boundaries[1].isdigit():
        left, right = int(boundaries[0]), int(boundaries[1])
        return lambda _data: torch.randint(left, right + 1, (len(_data['positions']),), device=device,
                                           dtype=const.TORCH_INT)
    size_nn = SizeClassifier.load_from_checkpoint(linker_size, map_location=device).eval().to(device)
    return lambda _data: size_nn.sample_sizes(_data, with_pocket=with_pocket)


def _load_ddpm(model, device, n_steps):
    ddpm = model if isinstance(model, DDPM) else DDPM.load_from_checkpoint(model, map_location=device)
    ddpm = ddpm.eval().to(device)
    if n_steps is not None:
        ddpm.edm.T = n_steps
    return ddpm


def _anchor_flags(charges, anchors):
    flags = np.zeros_like(charges)
    if anchors is not None:
        for anchor in str(anchors).split(','):
            flags[int(anchor.strip()) - 1] = 1
    return flags


def _batches(dataset, batch_size, collate_fn):
    for start in range(0, len(dataset), batch_size):
        yield collate_fn(dataset[start:start + batch_size])


OUTPUT_FORMATS = ('xyz', 'sdf', 'both')
BOND_ORDERS = ('distance', 'geometric')


def _check_hydrogens(hydrogens, output_format):
    if hydrogens and output_format == 'xyz':
        raise ValueError('hydrogens are written to the .sdf files: pass output_format sdf or both (--output_format); the '
                         '.xyz files stay the heavy-atom format of the reference')


def _sample_and_save(ddpm, dataset, collate_fn, sample_fn, batch_size, output_dir, name, com_key, hide_pocket,
                     output_format='xyz', metrics=False, clashes=False, protein=None, rings=False, bond_orders='distance',
                     aromatic=False, diversity=False, interactions=False, typed_protein=None, hydrogens=False,
                     pose_checks=False, cluster=None, pick=None, select_view='linker', relax=None, smiles=False,
                     filters=None, stereo=False):
    if output_format not in OUTPUT_FORMATS:
        raise ValueError(f'output_format must be one of {OUTPUT_FORMATS}, got {output_format!r}')
    if bond_orders not in BOND_ORDERS:
        raise ValueError(f'bond_orders must be one of {BOND_ORDERS}, got {bond_orders!r}')
    _check_hydrogens(hydrogens, output_format)
    select = _check_selection(cluster, pick, select_view)
    n_hydrogens = []
    written, found, scored, clash_records, ring_records, aromatic_records = [], [], [], [], [], []
    prints, contact_records, pose_records, eligible = [], [], [], []
    relax_records, relaxed_pose_records = [], []
    smiles_rows, stereo_rows = [], []
    catalogue, filter_records = (mol_metrics.load_filters(filters) if filters is not None else None), []
    for batch_i, data in enumerate(_batches(dataset, batch_size, collate_fn)):
        n = len(data['positions'])
        chain = None
        for _ in range(5):                                    # generate.py:152-160
            try:
                chain, node_mask = ddpm.sample_chain(data, sample_fn=sample_fn, keep_frames=1)
                break
            except FoundNaNException:
                continue
        if chain is None:
            raise Exception('Could not generate in 5 attempts')
        x = chain[0][:, :, :ddpm.n_dims]
        h = chain[0][:, :, ddpm.n_dims:]
        # put the molecule back to the initial frame (generate.py:165-170): the chain lives in the COM frame of the
        # fragments / anchors; `mean` broadcasts over the template width (linker rows included)
        com_mask = data[com_key] if ddpm.center_of_mass == 'fragments' else data['anchors']
        pos_masked = data['positions'] * com_mask
        mean = torch.sum(pos_masked, dim=1, keepdim=True) / com_mask.sum(1, keepdims=True)
        x = x + mean * node_mask
        offset = batch_i * batch_size
        names = [f'output_{offset + i}_{name}' for i in range(n)]
        if clashes:                                           # in the input frame, where the protein's atoms are: the template's
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            generated = node_mask * (1 - pad(data['fragment_mask']))                        # linker rows against the pocket rows,
            pocket_rows = pad(data['pocket_mask']) if protein is None else None            # or against the whole protein
            scored_x = x
            if pocket_rows is not None:                       # the pocket atoms where the file has them, not where the trip
                scored_x = torch.where(pocket_rows.bool(), pad(data['positions']), x)      # through the COM frame left them
            clash_records += mol_metrics.clashes_to_host(mol_metrics.analyze_clashes(
                h[:, :, :ddpm.num_classes], scored_x, generated, pocket_rows, protein=protein, is_geom=ddpm.is_geom))
        if interactions:                                      # the same rows and frame; the linker typed within the whole ligand
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            pocket_rows = pad(data['pocket_mask'])
            scored_x = torch.where(pocket_rows.bool(), pad(data['positions']), x)
            contact_records += mol_metrics.interactions_to_host(mol_metrics.analyze_interactions(
                h[:, :, :ddpm.num_classes], scored_x, node_mask * (1 - pad(data['fragment_mask'])), node_mask * (1 - pocket_rows),
                pocket_rows if typed_protein is None else None, protein=typed_protein, is_geom=ddpm.is_geom))
        shown_x = x                                           # what the files are written with; every score stays on x
        if relax is not None:                                 # the linker cleaned up, the pocket rows of the batch as the wall
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            linker_rows = node_mask * (1 - pad(data['fragment_mask']))
            pocket_rows = pad(data['pocket_mask']) if 'pocket_mask' in data else None
            wall_x = x if pocket_rows is None else torch.where(pocket_rows.bool(), pad(data['positions']), x)
            relaxed = relax_samples(h[:, :, :ddpm.num_classes], wall_x, node_mask, ddpm.is_geom, linker_rows,
                                    drop_mask=pocket_rows, steps=relax)
            shown_x = torch.where(linker_rows.bool(), relaxed.x, x)      # every other row as it was, bit for bit
        if hide_pocket:                                       # generate_with_pocket.py:272
            node_mask = node_mask.clone()
            width = data['pocket_mask'].shape[1]
            node_mask[:, :width][data['pocket_mask'].bool()] = 0
        if relax is not None:                                 # did the clean-up change the distance table's bond list?
            types = h[:, :, :ddpm.num_classes]
            relax_records += mol_metrics.relax_to_host(relaxed, perceive_bonds(types, x, node_mask, ddpm.is_geom),
                                                       perceive_bonds(types, shown_x, node_mask, ddpm.is_geom))
        if output_format != 'sdf':
            save_xyz_file(output_dir, h, shown_x, node_mask, names=names, is_geom=ddpm.is_geom, suffix='')
            written += [os.path.join(output_dir, f'{nm}_.xyz') for nm in names]
        if output_format != 'xyz':                            # on the chain's output, before it leaves the device
            found.append(perceive_all_bonds(h, shown_x, node_mask, ddpm.is_geom))
            shown = found[-1]
            planar = None
            if bond_orders == 'geometric':                    # Kekule orders for the planar rings, from the same geometry
                shown, ring_atoms = refine_bond_orders(shown, h[:, :, :ddpm.num_classes], shown_x, node_mask, ddpm.is_geom)
                planar = ring_atoms.atom_aromatic
            more = {}
            if hydrogens:                                     # on the list the file is written with
                more['hydrogens'] = add_hydrogens(shown, h[:, :, :ddpm.num_classes], shown_x, node_mask, ddpm.is_geom,
                                                  atom_planar=planar)
                n_hydrogens.append(more['hydrogens'].n_h)
            save_sdf_file(output_dir, h, shown_x, node_mask, shown.bonds, shown.n_bonds, names=names,
                          is_geom=ddpm.is_geom, suffix='', **more)
            written += [os.path.join(output_dir, f'{nm}_.sdf') for nm in names]
        if smiles:                                            # of the bond list the .sdf files carry (or would carry)
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            types = h[:, :, :ddpm.num_classes]
            listed = perceive_all_bonds(h, shown_x, node_mask, ddpm.is_geom)
            if bond_orders == 'geometric':
                listed = refine_bond_orders(listed, types, shown_x, node_mask, ddpm.is_geom)[0]
            smiles_rows += mol_metrics.smiles_records(types, node_mask, listed, node_mask * (1 - pad(data['fragment_mask'])),
                                                      drop_mask=pad(data['pocket_mask']) if 'pocket_mask' in data else None)
        if stereo:                                            # on the coordinates the files carry; always on the geometric orders
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            stereo_rows += mol_metrics.analyze_stereo(
                h[:, :, :ddpm.num_classes], shown_x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask'])),
                drop_mask=pad(data['pocket_mask']) if 'pocket_mask' in data else None)
        if filters is not None:                               # on the raw sample and the geometric orders, whatever the files hold
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            filter_records += mol_metrics.patterns_to_host(mol_metrics.analyze_patterns(
                h[:, :, :ddpm.num_classes], x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask'])), catalogue,
                drop_mask=pad(data['pocket_mask']) if 'pocket_mask' in data else None), catalogue.names)
        if metrics:                                           # the molecules as written: without the pocket
            types = h[:, :, :ddpm.num_classes]
            scored += mol_metrics.to_host(mol_metrics.analyze(types, x, node_mask, ddpm.is_geom), types, node_mask)
        if rings:                                             # likewise without the pocket; the linker rows marked
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            ring_records += mol_metrics.rings_to_host(*mol_metrics.analyze_rings(
                h[:, :, :ddpm.num_classes], x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask']))))
        if aromatic:                                          # likewise
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            aromatic_records += mol_metrics.aromatic_to_host(mol_metrics.analyze_aromatic(
                h[:, :, :ddpm.num_classes], x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask']))))
        if pose_checks:                                       # likewise; always on the geometric orders
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            pose_records += mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                h[:, :, :ddpm.num_classes], x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask'])),
                drop_mask=pad(data['pocket_mask']) if 'pocket_mask' in data else None))
            if relax is not None:                             # the same checks once more, on what the files hold
                relaxed_pose_records += mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                    h[:, :, :ddpm.num_classes], shown_x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask'])),
                    drop_mask=pad(data['pocket_mask']) if 'pocket_mask' in data else None))
        if diversity or select:                               # likewise; the bits stay on the device
            pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, x.shape[1] - m.shape[1]))     # noqa: E731
            drop = pad(data['pocket_mask']) if select and 'pocket_mask' in data else None      # as pose_checks passes them
            prints.append(mol_metrics.analyze_fingerprints(
                h[:, :, :ddpm.num_classes], x, node_mask, ddpm.is_geom, node_mask * (1 - pad(data['fragment_mask'])),
                drop_mask=drop))
            if select:                                        # only valid molecules in one piece are clustered and picked
                types = h[:, :, :ddpm.num_classes]
                eligible += mol_metrics.good_molecules(mol_metrics.to_host(
                    mol_metrics.analyze(types, x, node_mask, ddpm.is_geom, drop_mask=drop), types, node_mask, drop))
    if found:
        line = summary(found)
        if hydrogens:
            line['hydrogens_per_molecule'] = float(torch.cat(n_hydrogens).float().mean()) if line['molecules'] else 0.0
        print(json.dumps(line))
    if select:                                                # one input: its samples are one group
        whole, linker = (mol_metrics.cat_fingerprints([p[k] for p in prints]) for k in range(2))
        selection = mol_metrics.select_records(whole, linker, [0] * whole.bits.shape[0], eligible, view=select_view,
                                               threshold=cluster, k=pick)
    if metrics or clashes or rings or aromatic or diversity or interactions or pose_checks or select or relax is not None:
        scores = {}
        if metrics:                                           # no true molecule here: no novelty, no recovery
            scores = dict(mol_metrics.compute_metrics(scored), molecules=len(scored))
        if clashes:
            scores.update(mol_metrics.compute_clashes(clash_records))
        if interactions:
            scores.update(mol_metrics.compute_interactions(contact_records))
        if rings:                                             # no true molecule here either
            scores.update(mol_metrics.compute_rings(ring_records))
        if aromatic:
            scores.update(mol_metrics.compute_aromatic(aromatic_records))
        if pose_checks:                                       # no true molecule here either
            scores.update(mol_metrics.compute_pose_checks(pose_records))
            if relax is not None:
                scores.update({f'{k}_relaxed': v for k, v in mol_metrics.compute_pose_checks(relaxed_pose_records).items()})
        if relax is not None:
            scores.update(mol_metrics.compute_relaxation(relax_records))
        if diversity:                                         # one input: every sample against every other
            whole, linker = (mol_metrics.cat_fingerprints([p[k] for p in prints]) for k in range(2))
            records = mol_metrics.diversity_records(whole, linker, [0] * whole.bits.shape[0])
            scores.update(mol_metrics.compute_diversity(records, with_true=False, with_reference=False))
        if select:
            scores.update(mol_metrics.compute_selection(selection))
        if smiles and metrics:
            scores.update(mol_metrics.compute_smiles(smiles_rows, scored))     # the samples uniqueness counts
        if filters is not None and metrics:
            scores.update(mol_metrics.compute_filters(filter_records))
        if stereo and metrics:                                # no true molecule here: no stereo recovery
            scores.update(mol_metrics.compute_stereo(stereo_rows, scored))
        with open(os.path.join(output_dir, 'metrics.json'), 'w') as f:
            json.dump(scores, f, indent=1)
    if clashes:                                               # one record per written file, by its name
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(clash_records)}
        finite = lambda d: d if np.isfinite(d) else None      # noqa: E731  (no pair, or a flagged molecule: JSON has no inf / NaN)
        with open(os.path.join(output_dir, 'clashes.json'), 'w') as f:
            json.dump({os.path.basename(path): {'n_clashes': m.n_clashes, 'n_clash_atoms': m.n_clash_atoms,
                                                'min_distance': finite(m.min_distance)}
                       for path in written for m in [by_name[os.path.basename(path).rsplit('_.', 1)[0]]]}, f, indent=1)
    if interactions:                                          # likewise
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(contact_records)}
        with open(os.path.join(output_dir, 'interactions.json'), 'w') as f:
            json.dump({os.path.basename(path): {'score': m.score, 'terms': dict(zip(mol_metrics.INTERACTION_TERMS, m.terms)),
                                                'n_pairs': m.n_pairs, 'n_hbonds': m.n_hbonds,
                                                'n_hydrophobic': m.n_hydrophobic, 'status': m.status}
                       for path in written for m in [by_name[os.path.basename(path).rsplit('_.', 1)[0]]]}, f, indent=1)
    if pose_checks:                                           # likewise
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(pose_records)}
        with open(os.path.join(output_dir, 'pose_checks.json'), 'w') as f:
            json.dump({os.path.basename(path): {'counts': dict(zip(mol_metrics.POSE_COUNTS, m.counts)),
                                                'linker_counts': dict(zip(mol_metrics.POSE_COUNTS, m.linker_counts)),
                                                'n_flagged_atoms': m.n_flagged_atoms, 'status': m.status}
                       for path in written for m in [by_name[os.path.basename(path).rsplit('_.', 1)[0]]]}, f, indent=1)
    if relax is not None:                                     # likewise
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(relax_records)}
        with open(os.path.join(output_dir, 'relax.json'), 'w') as f:
            json.dump({os.path.basename(path): mol_metrics.relax_report(by_name[os.path.basename(path).rsplit('_.', 1)[0]])
                       for path in written}, f, indent=1)
    if smiles:                                                # likewise: one row per written file
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(smiles_rows)}
        by_stereo = {f'output_{i}_{name}': m.isomeric_smiles for i, m in enumerate(stereo_rows)}
        mol_metrics.write_smiles_csv(os.path.join(output_dir, 'smiles.csv'), [os.path.basename(path) for path in written],
                                     [by_name[os.path.basename(path).rsplit('_.', 1)[0]] for path in written],
                                     *([[by_stereo[os.path.basename(path).rsplit('_.', 1)[0]] for path in written]] if stereo else []))
    if stereo:                                                # likewise: one record per written file
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(stereo_rows)}
        mol_metrics.write_stereo_json(os.path.join(output_dir, 'stereo.json'), [os.path.basename(path) for path in written],
                                      [by_name[os.path.basename(path).rsplit('_.', 1)[0]] for path in written])
    if filters is not None:                                   # likewise: one record per written file
        by_name = {f'output_{i}_{name}': m for i, m in enumerate(filter_records)}
        mol_metrics.write_filters_json(os.path.join(output_dir, 'filters.json'), [os.path.basename(path) for path in written],
                                       [by_name[os.path.basename(path).rsplit('_.', 1)[0]] for path in written])
    if select:                                                # likewise, and the two answers a reader came for
        with open(os.path.join(output_dir, 'selection.json'), 'w') as f:
            json.dump(mol_metrics.selection_report(selection, _files_of_samples(written, name, len(selection))), f, indent=1)
    return written


def _selection_arguments(cluster, pick, select_view):
    """The keyword arguments ``_sample_and_save`` takes for a selection; none when none is asked for."""
    if not _check_selection(cluster, pick, select_view):
        return {}
    return {'cluster': cluster, 'pick': pick, 'select_view': select_view}


def _check_selection(cluster, pick, select_view):
    """Is a selection asked for?  Raises ``ValueError`` for a threshold, a number of picks or a view that cannot be."""
    if select_view not in mol_metrics.SELECT_VIEWS:
        raise ValueError(f'select_view must be one of {mol_metrics.SELECT_VIEWS}, got {select_view!r}')
    if cluster is not None:
        mol_metrics.threshold_fraction(cluster)
    if pick is not None and int(pick) < 1:
        raise ValueError(f'pick must be at least 1, got {pick!r}')
    return cluster is not None or pick is not None


def _files_of_samples(written, name, n):
    """The base names of the files sample ``0 .. n - 1`` wrote (``output_{i}_{name}_.*``; two with ``output_format='both'``)."""
    files = {}
    for path in written:
        base = os.path.basename(path)
        files.setdefault(base.rsplit('_.', 1)[0], []).append(base)
    return [files.get(f'output_{i}_{name}', []) for i in range(n)]


def generate(input_path, model, output_dir, n_samples, n_steps, linker_size, anchors=None, device=None, output_format='xyz',
             metrics=False, clashes=False, rings=False, bond_orders='distance', aromatic=False, diversity=False,
             hydrogens=False, pose_checks=False, cluster=None, pick=None, select_view='linker', relax=None, smiles=False,
             filters=None, stereo=False):
    """``generate.py`` main(): fragments file -> ``n_samples`` molecules with a sampled linker, as ``.xyz`` files
    (``output_format='sdf'``: ``.sdf`` files with perceived bonds instead, ``'both'``: both; one JSON line with the number of
    molecules, the share in one piece and the mean bond count is printed then).  ``metrics=True`` also writes
    ``metrics.json`` to ``output_dir``: valence rule, connectivity and uniqueness of the samples (``metrics.compute_metrics``).
    ``rings=True`` adds the ring scores of the samples to ``metrics.json`` (``metrics.analyze_rings`` / ``compute_rings``: the
    linker's ring count, small rings, macrocycles; the pocket variants take it as well).  ``bond_orders='geometric'`` writes
    the ``.sdf`` files with the Kekule orders of ``molecule_builder.refine_bond_orders`` (planar five- and six-rings
    alternate; 1, 2 or 3, never 4) and ``aromatic=True`` adds ``aromatic_rings_n``, ``ring_filter`` and
    ``valence_validity_geometric`` to ``metrics.json`` (``metrics.analyze_aromatic`` / ``compute_aromatic``); both rest on a
    geometric rule of this project's own, not on OpenBabel's or RDKit's, and the pocket variants take them as well.
    ``diversity=True`` adds ``internal_diversity`` and ``internal_diversity_linker`` of the samples of this one input
    (``metrics.analyze_fingerprints`` / ``compute_diversity``): one minus the mean pairwise Tanimoto similarity on this
    project's own circular fingerprint, not RDKit's Morgan fingerprint.  ``hydrogens=True`` adds explicit hydrogens with 3D
    positions to the ``.sdf`` files (``molecule_builder.add_hydrogens`` on the bond list the files are written with, a rule
    of this project's own, not RDKit's ``AddHs`` and not OpenBabel's; ``bond_orders='geometric'`` is recommended, because the
    distance table's arbitrary orders inside aromatic rings give arbitrary counts there) and ``hydrogens_per_molecule`` to
    the JSON line; with ``output_format='xyz'`` it raises ``ValueError``, and the pocket variants take it as well.
    ``pose_checks=True`` checks the internal geometry of every sample - bond lengths, bond angles, clashes between atoms four
    or more bonds apart - on the geometric bond orders, whatever ``bond_orders`` says about the files
    (``metrics.analyze_pose_checks`` / ``compute_pose_checks``: a rule of this project's own after the idea of PoseBusters'
    intramolecular checks, NOT PoseBusters' numbers), adds ``pose_valid``, ``bond_lengths_valid``, ``bond_angles_valid``,
    ``internal_clash_free``, their ``_linker`` variants and the per-molecule means to ``metrics.json`` and writes
    ``pose_checks.json`` with the counts per written file; the pocket variants take it as well, pocket atoms left out.
    ``cluster='0.65'`` (a similarity threshold) and / or ``pick=K`` say which few of the samples to look at: the valid samples
    in one piece are clustered (Taylor-Butina) and a diverse subset of ``K`` is picked (MaxMin, starting from the most typical
    sample) on the fingerprint ``select_view`` names (``metrics.select_records``: this project's own statement of both rules
    on this project's own fingerprint, NOT RDKit's ``Butina.ClusterData`` or ``MaxMinPicker``).  ``selection.json`` gets the
    record of every written file, ``picked`` and ``clusters`` (``metrics.selection_report``), ``metrics.json`` the
    ``metrics.compute_selection`` keys; no file is removed, renamed or rewritten.  The pocket variants take them as well,
    pocket atoms left out.
    ``relax=STEPS`` cleans the linker of every sample up before the files are written (``molecule_builder.relax_samples``:
    ``STEPS`` steps of a restrained FIRE minimisation in fp64 under a rule of this project's own, NOT UFF, MMFF or RDKit's or
    OpenBabel's optimiser; the fragments stay bit for bit, the topology is frozen, heavy atoms only, no torsion term): the
    ``.xyz`` and ``.sdf`` files carry the relaxed linker, and bonds, ``bond_orders='geometric'`` and ``hydrogens`` run on it;
    ``relax.json`` gets one record per written file and ``metrics.json`` the ``metrics.compute_relaxation`` keys.  EVERY
    OTHER SCORE STAYS A SCORE OF THE RAW SAMPLE, because the scores measure the model; with ``pose_checks=True`` the pose
    keys are written a second time, on the relaxed coordinates, under ``<key>_relaxed``.  The pocket variants take it as
    well: there the wall is the pocket rows of the batch, not the whole protein of ``generate_with_protein``.
    ``smiles=True`` writes ``smiles.csv`` with one row per written file: ``file``, ``smiles`` (the whole molecule, pocket atoms
    left out), ``linker_smiles`` (the linker atoms as a molecule of their own), ``code`` (the canonical 64-bit code, hex) and
    ``canonical`` (0 when a search budget was hit or the bond list was flagged).  The strings describe the bond list the
    ``.sdf`` files carry - ``bond_orders='geometric'`` and ``relax`` apply to them - canonical under this project's own rule
    (``metrics.canonical_ranks``, ``molecule_builder.smiles``), NOT RDKit's canonical SMILES: Kekule orders as perceived, no
    aromatic lower case, brackets only on over-valent atoms, no charges, no stereo.  With ``metrics=True`` ``metrics.json``
    gains ``smiles_uniqueness`` and ``smiles_canonical`` (``metrics.compute_smiles``).  The pocket variants take it as well.

    ``filters='basic'`` or ``filters=FILE`` matches a catalogue of structural alerts against every sample
    (``metrics.analyze_patterns``: ``'basic'`` is this project's own short list, ``data/filters_basic.csv``; a file is CSV
    with a SMARTS and an optional name per row, the form of the reference's PAINS list) and writes ``filters.json`` with one
    record per written file: ``file``, ``hits``, ``linker_hits`` (the alerts matched through a linker atom) and ``status``.
    Always on the geometric bond orders and on the raw sample, whatever ``bond_orders`` and ``relax`` say.  With
    ``metrics=True`` ``metrics.json`` gains ``filters_passed``, ``filters_passed_linker``, ``filter_hits_per_molecule`` and
    ``filters_budget`` (``metrics.compute_filters``).  A SMARTS subset and a matcher of this project's own, NOT RDKit's.  The
    pocket variants take it as well."""
    _check_hydrogens(hydrogens, output_format)
    selection = _selection_arguments(cluster, pick, select_view)
    if clashes:
        raise ValueError('clashes are scored against a protein: pass a pocket or a protein file (--pocket / --protein)')
    device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
    os.makedirs(output_dir, exist_ok=True)
    sample_fn = make_sample_fn(linker_size, device)
    ddpm = _load_ddpm(model, device, n_steps)
    if ddpm.center_of_mass == 'anchors' and anchors is None:
        raise ValueError('Please pass anchor atoms indices or use another DiffLinker model that does not require '
                         'information about anchors')
    if input_path.split('.')[-1] not in ['sdf', 'pdb', 'mol', 'mol2']:
        raise ValueError('Please upload the file in one of the following formats: .pdb, .sdf, .mol, .mol2')
    molecule = read_molecule(input_path)
    name = '.'.join(input_path.split('/')[-1].split('.')[:-1])
    positions, one_hot, charges = parse_molecule(molecule, is_geom=ddpm.is_geom)
    t = lambda a: torch.tensor(a, dtype=const.TORCH_FLOAT, device=device)     # noqa: E731
    dataset = [{
        'uuid': '0', 'name': '0', 'positions': t(positions), 'one_hot': t(one_hot), 'charges': t(charges),
        'anchors': t(_anchor_flags(charges, anchors)), 'fragment_mask': t(np.ones_like(charges)),
        'linker_mask': t(np.zeros_like(charges)), 'num_atoms': len(positions),
    }] * n_samples
    return _sample_and_save(ddpm, dataset, collate_with_fragment_edges, sample_fn, min(n_samples, 64), output_dir, name,
                            com_key='fragment_mask', hide_pocket=False, output_format=output_format, metrics=metrics,
                            rings=rings, bond_orders=bond_orders, aromatic=aromatic, diversity=diversity,
                            **({'hydrogens': True} if hydrogens else {}), **({'pose_checks': True} if pose_checks else {}),
                            **({'relax': relax} if relax is not None else {}), **({'smiles': True} if smiles else {}),
                            **({'filters': filters} if filters is not None else {}), **({'stereo': True} if stereo else {}),
                            **selection)


def _generate_pocket_common(frag, pocket, ddpm, sample_fn, output_dir, name, n_samples, anchors, max_batch_size, device,
                            output_format, metrics=False, clashes=False, protein=None, rings=False, bond_orders='distance',
                            aromatic=False, interactions=False, typed_protein=None, hydrogens=False, pose_checks=False,
                            selection=None, relax=None, smiles=False, filters=None, stereo=False):
    frag_pos, frag_one_hot, frag_charges = frag
    pocket_pos, pocket_one_hot, pocket_charges = pocket
    positions = np.concatenate([frag_pos, pocket_pos], axis=0)
    one_hot = np.concatenate([frag_one_hot, pocket_one_hot], axis=0)
    charges = np.concatenate([frag_charges, pocket_charges], axis=0)
    ones_f, zeros_f = np.ones_like(frag_charges), np.zeros_like(frag_charges)
    ones_p, zeros_p = np.ones_like(pocket_charges), np.zeros_like(pocket_charges)
    t = lambda a: torch.tensor(a, dtype=const.TORCH_FLOAT, device=device)     # noqa: E731
    dataset = [{
        'uuid': '0', 'name': '0', 'positions': t(positions), 'one_hot': t(one_hot), 'charges': t(charges),
        'anchors': t(_anchor_flags(charges, anchors)),
        'fragment_only_mask': t(np.concatenate([ones_f, zeros_p])), 'pocket_mask': t(np.concatenate([zeros_f, ones_p])),
        'fragment_mask': t(np.concatenate([ones_f, ones_p])), 'linker_mask': t(np.concatenate([zeros_f, zeros_p])),
        'num_atoms': len(positions),
    }] * n_samples
    dataset = MOADDataset(data=dataset)                   # generate_with_pocket.py:249-250: DDPM.sample_chain keys the
    ddpm.val_dataset = dataset                            # centre-of-mass mask on the dataset type (lightning.py:443)
    return _sample_and_save(ddpm, dataset, collate_with_fragment_without_pocket_edges, sample_fn,
                            min(n_samples, max_batch_size), output_dir, name, com_key='fragment_only_mask',
                            hide_pocket=True, output_format=output_format, metrics=metrics, clashes=clashes, protein=protein,
                            rings=rings, bond_orders=bond_orders, aromatic=aromatic, interactions=interactions,
                            typed_protein=typed_protein, **({'hydrogens': True} if hydrogens else {}),
                            **({'pose_checks': True} if pose_checks else {}), **({'relax': relax} if relax is not None else {}),
                            **({'smiles': True} if smiles else {}), **({'filters': filters} if filters is not None else {}),
                            **({'stereo': True} if stereo else {}), **(selection or {}))


def generate_with_pocket(input_path, pocket_path, backbone_atoms_only, model, output_dir, n_samples, n_steps, linker_size,
                         anchors=None, max_batch_size=64, random_seed=None, device=None, output_format='xyz',
                         metrics=False, clashes=False, rings=False, bond_orders='distance', aromatic=False, interactions=False,
                         hydrogens=False, pose_checks=False, cluster=None, pick=None, select_view='linker', relax=None,
                         smiles=False, filters=None, stereo=False):
    """``generate_with_pocket.py`` main(): the pocket is given as its own PDB file.  ``clashes=True`` scores every sample's
    generated atoms against the pocket atoms (``metrics.analyze_clashes``), adds the ``metrics.compute_clashes`` keys to
    ``metrics.json`` and writes ``clashes.json``: ``n_clashes``, ``n_clash_atoms`` and ``min_distance`` per written file.
    ``interactions=True`` scores the contacts of the generated atoms, typed within the whole ligand, with the pocket atoms
    (``metrics.analyze_interactions``: the intermolecular terms of Trott & Olson under this project's own typing, not
    AutoDock Vina's numbers), adds the ``metrics.compute_interactions`` keys to ``metrics.json`` and writes
    ``interactions.json``: ``score``, the five fixed-point ``terms`` (units of 2^-32), ``n_pairs``, ``n_hbonds``,
    ``n_hydrophobic`` and ``status`` per written file.  ``hydrogens=True`` as in ``generate``: the scores above keep counting
    heavy atoms alone.  ``pose_checks=True`` as in ``generate``, on the ligand without the pocket atoms; ``cluster``, ``pick``
    and ``select_view`` likewise; ``relax=STEPS`` as in ``generate``, the pocket atoms as the wall; ``smiles=True`` as in
    ``generate``, the pocket atoms left out of the strings."""
    _check_hydrogens(hydrogens, output_format)
    selection = _selection_arguments(cluster, pick, select_view)
    device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
    os.makedirs(output_dir, exist_ok=True)
    if random_seed is not None:
        set_deterministic(random_seed)
    sample_fn = make_sample_fn(linker_size, device, with_pocket=True)
    ddpm = _load_ddpm(model, device, n_steps)
    if ddpm.center_of_mass == 'anchors' and anchors is None:
        raise ValueError('Please pass anchor atoms indices or use another DiffLinker model that does not require '
                         'information about anchors')
    if input_path.split('.')[-1] not in ['sdf', 'pdb', 'mol', 'mol2']:
        raise ValueError('Please upload the fragments file in one of the following formats: .pdb, .sdf, .mol, .mol2')
    if pocket_path.split('.')[-1] != 'pdb':
        raise ValueError('Please upload the pocket file in .pdb format')
    molecule = read_molecule(input_path)
    name = '.'.join(input_path.split('/')[-1].split('.')[:-1])
    frag = parse_molecule(molecule, is_geom=ddpm.is_geom)
    pocket = pocket_arrays(read_pocket(pocket_path), backbone_atoms_only)
    return _generate_pocket_common(frag, pocket, ddpm, sample_fn, output_dir, name, n_samples, anchors, max_batch_size,
                                   device, output_format, metrics, clashes, rings=rings, bond_orders=bond_orders,
                                   aromatic=aromatic, interactions=interactions, **({'hydrogens': True} if hydrogens else {}),
                                   **({'pose_checks': True} if pose_checks else {}),
                                   **({'relax': relax} if relax is not None else {}),
                                   **({'smiles': True} if smiles else {}),
                                   **({'filters': filters} if filters is not None else {}),
                                   **({'stereo': True} if stereo else {}),
                                   **({'selection': selection} if selection else {}))


def generate_with_protein(input_path, protein_path, backbone_atoms_only, model, output_dir, n_samples, n_steps,
                          linker_size, anchors=None, max_batch_size=64, random_seed=None, device=None, output_format='xyz',
                          metrics=False, clashes=False, rings=False, bond_orders='distance', aromatic=False,
                          interactions=False, hydrogens=False, pose_checks=False, cluster=None, pick=None,
                          select_view='linker', relax=None, smiles=False, filters=None, stereo=False):
    """``generate_with_protein.py`` main(): the pocket = residues of the protein within 6 A of the fragments.
    ``clashes=True`` as in ``generate_with_pocket``, but against ALL protein atoms whose element is in the vocabulary
    (``io.get_protein_atoms``), residues outside the pocket the model saw included; the pocket rows of the batch are then not
    targets, so no atom counts twice.  ``interactions=True`` likewise scores against the whole protein, which is typed once
    (``metrics.protein_types``), so no residue is cut at a pocket boundary.  ``hydrogens=True``, ``pose_checks=True``,
    ``cluster``, ``pick`` and ``select_view`` as in ``generate``; ``relax=STEPS`` likewise, with the pocket rows of the batch
    as the wall, not the whole protein; ``smiles=True`` as in ``generate_with_pocket``."""
    _check_hydrogens(hydrogens, output_format)
    selection = _selection_arguments(cluster, pick, select_view)
    device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
    os.makedirs(output_dir, exist_ok=True)
    if random_seed is not None:
        set_deterministic(random_seed)
    sample_fn = make_sample_fn(linker_size, device, with_pocket=True)
    ddpm = _load_ddpm(model, device, n_steps)
    if ddpm.center_of_mass == 'anchors' and anchors is None:
        raise ValueError('Please pass anchor atoms indices or use another DiffLinker model that does not require '
                         'information about anchors')
    molecule = read_molecule(input_path)
    name = '.'.join(input_path.split('/')[-1].split('.')[:-1])
    frag = parse_molecule(molecule, is_geom=ddpm.is_geom)
    pocket = get_pocket(molecule, protein_path, backbone_atoms_only)
    protein, typed_protein = None, None
    if clashes or interactions:
        positions, types = get_protein_atoms(protein_path, ddpm.is_geom)
        protein = (torch.tensor(positions, dtype=const.TORCH_FLOAT, device=device),
                   torch.tensor(types, dtype=torch.int32, device=device))
    if interactions:
        typed_protein = protein + (mol_metrics.protein_types(*protein, is_geom=ddpm.is_geom),)
    return _generate_pocket_common(frag, pocket, ddpm, sample_fn, output_dir, name, n_samples, anchors, max_batch_size,
                                   device, output_format, metrics, clashes, protein if clashes else None, rings=rings,
                                   bond_orders=bond_orders, aromatic=aromatic, interactions=interactions,
                                   typed_protein=typed_protein, **({'hydrogens': True} if hydrogens else {}),
                                   **({'pose_checks': True} if pose_checks else {}),
                                   **({'relax': relax} if relax is not None else {}),
                                   **({'smiles': True} if smiles else {}),
                                   **({'filters': filters} if filters is not None else {}),
                                   **({'stereo': True} if stereo else {}),
                                   **({'selection': selection} if selection else {}))


def add_relax_argument(p):
    """``--relax [STEPS]``, shared with ``sample``."""
    p.add_argument('--relax', type=int, nargs='?', const=const.RELAX_STEPS, default=None, metavar='STEPS',
                   help='clean the linker of every sample up on the GPU before the files are written: STEPS steps (default '
                        f'{const.RELAX_STEPS}, at most 1000) of a restrained FIRE minimisation in fp64 of bonds, angles, internal '
                        'repulsion, the pocket rows as a wall and a restraint to the sampled position, the fragments fixed and '
                        'the topology frozen (a rule of this project, NOT UFF, MMFF or RDKit\'s or OpenBabel\'s optimiser; heavy '
                        'atoms only, no torsion term).  Writes relax.json and the relax_* keys of metrics.json; every other '
                        'score stays a score of the raw sample')


def add_filters_argument(p):
    """``--filters``, shared with ``sample``."""
    p.add_argument('--filters', default=None, metavar='FILE|basic',
                   help='match structural alerts against every sample on the GPU and write filters.json with one record per '
                        'written file (the alerts hit, those hit through a linker atom, the status): "basic" is this '
                        'project\'s own short catalogue, FILE a CSV with a SMARTS and an optional name per row (the form of a '
                        'PAINS list).  A SMARTS subset and a matching rule of this project\'s own (NOT RDKit\'s matcher: no '
                        'charges, no stereo, no explicit hydrogens, no SSSR counts), always on the geometric bond orders.  With '
                        '--metrics adds filters_passed, filters_passed_linker, filter_hits_per_molecule and filters_budget to '
                        'metrics.json')


def add_smiles_argument(p):
    """``--smiles``, shared with ``sample``."""
    p.add_argument('--smiles', action='store_true',
                   help='write smiles.csv with one row per written file: the SMILES of the molecule (pocket atoms left out) and '
                        'of its linker, the canonical 64-bit code and whether the search stayed within its budgets.  Atoms are '
                        'ranked on the GPU by an individualisation-refinement search; the strings are canonical under this '
                        'project\'s own rule, NOT RDKit\'s canonical SMILES (Kekule orders as the .sdf files carry them, no '
                        'aromatic lower case, no charges, no stereo, at most 256 atoms).  With --metrics adds smiles_uniqueness '
                        'and smiles_canonical to metrics.json')


def add_stereo_argument(p):
    """``--stereo``, shared with ``sample``."""
    p.add_argument('--stereo', action='store_true',
                   help='perceive stereo from the 3D coordinates the files carry, on the GPU, and write stereo.json with one '
                        'record per written file: assigned tetrahedral centres and stereo double bonds (all, and those that '
                        'touch the linker), the undetermined ones (a centre too flat, a double bond too twisted to call), a '
                        'stereo-aware canonical code, whether the molecule is chiral, and an isomeric SMILES.  A rule of this '
                        'project\'s own, NOT RDKit\'s stereo perception and NOT CIP: labels relative to this project\'s '
                        'symmetry classes, no R/S or E/Z names, no trivalent N, P or sulfoxide centres, no allenes or '
                        'atropisomers, always on the geometric bond orders.  With --metrics adds stereocentres_per_molecule, '
                        'stereo_bonds_per_molecule, stereo_undetermined, chiral_fraction and stereo_uniqueness to metrics.json; '
                        'with --smiles adds an isomeric_smiles column to smiles.csv')


def add_selection_arguments(p):
    """``--cluster``, ``--pick`` and ``--select_view``, shared with ``sample``."""
    p.add_argument('--cluster', default=None, metavar='S',
                   help='cluster the valid samples of every input on the GPU at the Tanimoto similarity threshold S, a decimal '
                        'such as 0.65 (Taylor-Butina sphere exclusion, this project\'s own statement of the rule on this '
                        'project\'s circular fingerprint, not RDKit\'s Butina.ClusterData) and add the cluster scores to '
                        'metrics.json')
    p.add_argument('--pick', type=int, default=None, metavar='K',
                   help='pick a diverse subset of K of the valid samples of every input on the GPU (MaxMin from the most typical '
                        'sample, this project\'s own tie rules on this project\'s fingerprint, not RDKit\'s MaxMinPicker)')
    p.add_argument('--select_view', choices=mol_metrics.SELECT_VIEWS, default='linker',
                   help='the fingerprint --cluster and --pick compare: linker (the centres are the linker atoms) or whole (all '
                        'samples of an input share their fragments, so this mostly measures the fragments)')


def selection_arguments(a):
    """The keyword arguments the parsed ``--cluster`` / ``--pick`` / ``--select_view`` stand for; none when neither is given."""
    if a.cluster is None and a.pick is None:
        return {}
    return {'cluster': a.cluster, 'pick': a.pick, 'select_view': a.select_view}


def main(argv=None):
    p = argparse.ArgumentParser(description='DiffLinker sampling on MI355X (generate.py / generate_with_pocket.py / '
                                            'generate_with_protein.py of the reference)')
    p.add_argument('--fragments', required=True, help='file with the input fragments (.sdf .mol .mol2 .pdb)')
    p.add_argument('--pocket', default=None, help='PDB file of the pocket residues (generate_with_pocket.py)')
    p.add_argument('--protein', default=None, help='PDB file of the whole protein (generate_with_protein.py)')
    p.add_argument('--backbone_atoms_only', action='store_true', default=False)
    p.add_argument('--model', required=True, help='DiffLinker checkpoint')
    p.add_argument('--linker_size', required=True, help='integer, "lo,hi", or a size-predictor checkpoint')
    p.add_argument('--output', default='./')
    p.add_argument('--n_samples', type=int, default=5)
    p.add_argument('--n_steps', type=int, default=None)
    p.add_argument('--anchors', default=None, help='comma-separated 1-based indices of the anchor atoms')
    p.add_argument('--max_batch_size', type=int, default=64)
    p.add_argument('--random_seed', type=int, default=None)
    p.add_argument('--output_format', choices=OUTPUT_FORMATS, default='xyz',
                   help='xyz: element symbols and coordinates; sdf: V2000 mol blocks with bonds perceived on the GPU '
                        '(the molecule_builder rule of the reference, in place of its obabel call); both: both')
    p.add_argument('--metrics', action='store_true',
                   help='score the generated molecules on the GPU (valence rule, connectivity, uniqueness) and write '
                        'metrics.json to the output directory')
    p.add_argument('--clashes', action='store_true',
                   help='with --pocket / --protein: count the steric clashes of the generated atoms with the pocket atoms / '
                        'with all protein atoms on the GPU (0.75 x the sum of the van der Waals radii), add the scores to '
                        'metrics.json and write clashes.json with one record per written file')
    p.add_argument('--interactions', action='store_true',
                   help='with --pocket / --protein: score the contacts of the generated atoms with the pocket atoms / with all '
                        'protein atoms on the GPU (the intermolecular terms of Trott & Olson under this project\'s heavy-atom '
                        'typing, not AutoDock Vina\'s numbers), add the scores to metrics.json and write interactions.json with '
                        'one record per written file')
    p.add_argument('--rings', action='store_true',
                   help='perceive the rings of the generated molecules on the GPU (ring count of the linker, small rings, '
                        'macrocycles; the cyclomatic number, no aromaticity) and add the scores to metrics.json')
    p.add_argument('--bond_orders', choices=BOND_ORDERS, default='distance',
                   help='bond orders of the .sdf files: distance (the distance table of the reference\'s molecule_builder) or '
                        'geometric (planar five- and six-rings get Kekule orders 1 / 2 from the 3D geometry, so aromatic rings '
                        'alternate; a rule of this project, not OpenBabel\'s bond typing)')
    p.add_argument('--aromatic', action='store_true',
                   help='perceive aromatic rings from the geometry on the GPU (a rule of this project, not RDKit\'s) and add '
                        'aromatic_rings_n, ring_filter and valence_validity_geometric to metrics.json')
    p.add_argument('--diversity', action='store_true',
                   help='without --pocket / --protein: fingerprint the generated molecules on the GPU (this project\'s '
                        'circular fingerprint, not RDKit\'s Morgan) and add internal_diversity and internal_diversity_linker '
                        'to metrics.json')
    p.add_argument('--hydrogens', action='store_true',
                   help='add explicit hydrogens with 3D positions to the .sdf files on the GPU (needs --output_format sdf or '
                        'both; a rule of this project, not RDKit\'s AddHs and not OpenBabel\'s).  --bond_orders geometric is '
                        'recommended: the distance table\'s arbitrary orders inside aromatic rings give arbitrary hydrogen '
                        'counts there')
    p.add_argument('--pose_checks', action='store_true',
                   help='check the internal geometry of the generated molecules on the GPU - bond lengths, bond angles, '
                        'clashes between atoms four or more bonds apart, always on the geometric bond orders (a rule of this '
                        'project after the idea of PoseBusters\' intramolecular checks, NOT PoseBusters\' numbers) - add '
                        'pose_valid and its parts to metrics.json and write pose_checks.json with one record per written file')
    add_relax_argument(p)
    add_selection_arguments(p)
    add_smiles_argument(p)
    add_filters_argument(p)
    add_stereo_argument(p)
    a = p.parse_args(argv)
    if a.clashes and a.pocket is None and a.protein is None:
        raise ValueError('--clashes scores the generated atoms against a protein: pass --pocket or --protein')
    if a.interactions and a.pocket is None and a.protein is None:
        raise ValueError('--interactions scores the generated atoms against a protein: pass --pocket or --protein')
    extra = {'clashes': True} if a.clashes else {}
    if a.interactions:
        extra['interactions'] = True
    more = {'rings': True} if a.rings else {}
    if a.bond_orders != 'distance':
        more['bond_orders'] = a.bond_orders
    if a.aromatic:
        more['aromatic'] = True
    if a.hydrogens:
        more['hydrogens'] = True
    if a.pose_checks:
        more['pose_checks'] = True
    if a.relax is not None:
        more['relax'] = a.relax
    more.update(selection_arguments(a))
    if a.smiles:
        more['smiles'] = True
    if a.filters is not None:
        more['filters'] = a.filters
    if a.stereo:
        more['stereo'] = True
    if a.pocket is not None:
        files = generate_with_pocket(a.fragments, a.pocket, a.backbone_atoms_only, a.model, a.output, a.n_samples,
                                     a.n_steps, a.linker_size, a.anchors, a.max_batch_size, a.random_seed,
                                     output_format=a.output_format, metrics=a.metrics, **extra, **more)
    elif a.protein is not None:
        files = generate_with_protein(a.fragments, a.protein, a.backbone_atoms_only, a.model, a.output, a.n_samples,
                                      a.n_steps, a.linker_size, a.anchors, a.max_batch_size, a.random_seed,
                                      output_format=a.output_format, metrics=a.metrics, **extra, **more)
    else:
        files = generate(a.fragments, a.model, a.output, a.n_samples, a.n_steps, a.linker_size, a.anchors,
                         output_format=a.output_format, metrics=a.metrics, **more,
                         **({'diversity': True} if a.diversity else {}))
    if a.output_format == 'xyz':
        print(f'Saved {len(files)} generated molecules in .xyz format in directory {a.output}')
    else:
        print(f'Saved {len(files)} files ({a.output_format}) of generated molecules in directory {a.output}')


if __name__ == '__main__':
    main()
