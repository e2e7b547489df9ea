"""Dataset sampling drivers — the bodies of the reference's ``sample.py`` (:26-200) and ``sample_trajectories.py``
(:19-110) as importable functions: walk a preprocessed validation / test set, write the ground truth, the
fragments (and the pocket) once, then ``n_samples`` sampled molecules per entry as ``<uuid>/<i>_.xyz``; resumable the
way the script is (``check_if_generated``).  The matplotlib rendering of ``sample_trajectories.py`` (``visualize_chain``)
is presentation and is not provided; the per-frame ``.xyz`` files it renders from are.

``python -m difflinker_amd.sample --help`` exposes ``sample.py``'s flags; ``--keep_frames K`` switches to the
trajectory mode.
"""
import argparse
import json
import os

import torch

from . import metrics as mol_metrics
from . import utils
from .datasets import MOADDataset, collate, collate_with_fragment_edges, get_dataloader
from .generate import (BOND_ORDERS, OUTPUT_FORMATS, _check_selection, add_relax_argument, add_selection_arguments,
                       add_filters_argument, add_smiles_argument, add_stereo_argument, selection_arguments)
from .io import save_sdf_file, save_xyz_file
from .lightning import DDPM
from .linker_size import SizeClassifier
from .molecule_builder import add_hydrogens, perceive_all_bonds, perceive_bonds, refine_bond_orders, relax_samples, summary


def check_if_generated(_output_dir, _uuids, n_samples):
    """``(everything already there, first sample index to (re)generate)`` — sample.py:37-60, including its
    restart-two-back rule."""
    generated = True
    starting_points = []
    for _uuid in _uuids:
        numbers = []
        for fname in os.listdir(os.path.join(_output_dir, _uuid)):
            try:
                numbers.append(int(fname.split('_')[0]))
            except ValueError:
                continue
        if len(numbers) == 0 or max(numbers) != n_samples - 1:
            generated = False
            starting_points.append(0 if len(numbers) == 0 else max(numbers) - 1)
    starting = min(starting_points) if len(starting_points) > 0 else None
    return generated, starting


def _prepare(checkpoint, prefix, data, n_steps, device):
    model = checkpoint if isinstance(checkpoint, DDPM) else DDPM.load_from_checkpoint(checkpoint, map_location=device)
    model.val_data_prefix = prefix
    if data is not None:
        model.data_path = data
    if n_steps is not None:
        model.edm.T = n_steps
    model = model.eval().to(device)
    model.torch_device = device
    model.setup(stage='val')
    return model


def sample(checkpoint, samples, prefix, n_samples, device, data=None, n_steps=None, linker_size_model=None,
           output_format='xyz', metrics=False, geometry=False, clashes=False, shape=False, rings=False,
           bond_orders='distance', aromatic=False, diversity=False, diversity_reference=None, pharmacophore=False,
           interactions=False, hydrogens=False, pose_checks=False, cluster=None, pick=None, select_view='linker', relax=None,
           smiles=False, filters=None, stereo=False):
    """``sample.py``.  Returns the output directory.  ``metrics=True`` scores the molecules sampled in this call against
    the data set's own (``metrics.compute_metrics``: valence rule, connectivity, uniqueness, novelty, recovery) and writes
    the result to ``metrics.json`` in the output directory; with ``geometry=True`` as well, the symmetry-aware RMSD of the
    recovered samples (``metrics.compute_geometry``: ``rmsd``, ``rmsd_molecules``, ``rmsd_truncated``) joins it.  ``output_format`` 'sdf' / 'both' writes the sampled molecules (not
    the ground truth, fragments or pocket) as ``<uuid>/<i>_.sdf`` with bonds perceived on the GPU, instead of / beside the
    ``.xyz`` files, and prints one JSON line with the number of molecules, the share in one piece and the mean bond count.
    ``clashes=True`` (pocket data sets only; others raise ``ValueError``) counts the steric clashes of every sample's linker
    atoms with its pocket atoms, and of the data set's own linker in the same pocket as ``true``
    (``metrics.analyze_clashes`` / ``compute_clashes``); the keys go into ``metrics.json``, beside the ``metrics`` keys when
    both are asked for and alone otherwise.  ``shape=True`` scores EVERY sample's gridded van der Waals volume against its
    true molecule's, in the centred frame the two share and without the pocket rows (``metrics.analyze_shapes`` /
    ``compute_shapes``: once over the ligand rows, once over the linker rows alone); its keys go into ``metrics.json`` in the
    same way, with ``shape_tanimoto_valid`` when ``metrics`` is asked for as well.  ``rings=True`` perceives the rings of
    every sample and of its true molecule, pocket rows left out (``metrics.analyze_rings`` / ``compute_rings``: the linker's
    ring count ``rings_n``, small rings, macrocycles), and writes those keys in the same way.  ``bond_orders='geometric'``
    writes the ``.sdf`` files with the Kekule orders of ``molecule_builder.refine_bond_orders`` (planar five- and six-rings
    alternate; 1, 2 or 3, never 4); ``aromatic=True`` adds ``aromatic_rings_n``, ``ring_filter`` and
    ``valence_validity_geometric`` of the samples and of their true molecules (``metrics.analyze_aromatic`` /
    ``compute_aromatic``).  Both rest on a geometric rule of this project's own, not on OpenBabel's or RDKit's.
    ``diversity=True`` fingerprints every sample and every true molecule, pocket rows left out
    (``metrics.analyze_fingerprints``: once with every atom as a centre, once with the linker atoms), keeps the bits on the
    device across the batches and writes ``metrics.compute_diversity``'s keys in the same way: ``internal_diversity`` and
    ``internal_diversity_linker`` among the samples of each input, ``similarity_to_true`` and ``similarity_to_true_linker``.
    ``diversity_reference`` names another data set under ``data`` (typically the training set); it is fingerprinted once,
    in batches, and ``nearest_reference_similarity`` / ``nearest_reference_identical`` join the keys.  All of these are
    Tanimoto similarities on this project's own circular fingerprint, not on RDKit's Morgan fingerprint.
    ``pharmacophore=True`` perceives the pharmacophore features of every sample and of its true molecule and matches them
    (``metrics.analyze_pharmacophores`` / ``compute_pharmacophores``), on the pairs and rows of ``shape=True``: ligand rows
    without the pocket, the linker marked.  ``feature_similarity`` and ``feature_similarity_linker`` go into ``metrics.json``,
    and with ``shape=True`` as well ``sc_similarity`` and ``sc_similarity_7/8/9``, where the reference has SC-RDKit.  The
    features are this project's own, after RDKit's ``BaseFeatures.fdef`` and ``FeatMapParams`` defaults, not RDKit's numbers.
    ``interactions=True`` (pocket data sets only; others raise ``ValueError``) scores the contacts of every sample's LINKER
    atoms, typed in the context of the whole ligand, with its pocket atoms, and of the data set's own linker in the same
    pocket as ``true`` (``metrics.analyze_interactions`` / ``compute_interactions``: the intermolecular terms of Trott &
    Olson under this project's own heavy-atom typing - not AutoDock Vina's numbers); the keys go into ``metrics.json``.
    ``hydrogens=True`` adds explicit hydrogens with 3D positions to the ``.sdf`` files (``molecule_builder.add_hydrogens`` on
    the bond list the files are written with; a rule of this project's own, not RDKit's ``AddHs`` and not OpenBabel's;
    ``bond_orders='geometric'`` is recommended, because the distance table's arbitrary orders inside aromatic rings give
    arbitrary counts there) and ``hydrogens_per_molecule`` to the JSON line; with ``output_format='xyz'`` it raises
    ``ValueError``.  No score counts them.
    ``pose_checks=True`` checks the internal geometry of every sample and of its true molecule, pocket rows left out and the
    linker rows marked - bond lengths, bond angles, clashes between atoms four or more bonds apart, always on the geometric
    bond orders (``metrics.analyze_pose_checks`` / ``compute_pose_checks``: a rule of this project's own after the idea of
    PoseBusters' intramolecular checks, NOT PoseBusters' numbers) - and writes ``pose_valid``, ``bond_lengths_valid``,
    ``bond_angles_valid``, ``internal_clash_free``, their ``_linker`` variants, the per-molecule means and the ``true_``
    values of all of them to ``metrics.json``.
    ``cluster='0.65'`` (a similarity threshold) clusters the valid samples in one piece of every input (Taylor-Butina) on the
    fingerprint ``select_view`` names and writes ``metrics.compute_selection``'s keys to ``metrics.json``; ``pick=K`` picks a
    diverse subset of ``K`` of them per input (MaxMin from the most typical sample) and writes ``selection.json``
    (``metrics.selection_report``: every sample's record by ``<uuid>/<i>_.<format>``, ``picked``, ``clusters``).  Both are
    ``metrics.select_records``: this project's own statement of the rules on this project's own fingerprint, NOT RDKit's
    ``Butina.ClusterData`` or ``MaxMinPicker``.  No file is removed, renamed or rewritten.
    ``relax=STEPS`` cleans the linker of every sample up before its files are written (``molecule_builder.relax_samples``:
    ``STEPS`` steps of a restrained FIRE minimisation in fp64 under a rule of this project's own, NOT UFF, MMFF or RDKit's or
    OpenBabel's optimiser; fragments fixed bit for bit, topology frozen, heavy atoms only, no torsion term; the pocket rows of
    a pocket data set are the wall).  The sample files carry the relaxed linker, and bonds, ``bond_orders='geometric'`` and
    ``hydrogens`` run on it; ``relax.json`` gets one record per written file and ``metrics.json`` the
    ``metrics.compute_relaxation`` keys.  EVERY OTHER SCORE STAYS A SCORE OF THE RAW SAMPLE; with ``pose_checks=True`` the
    pose keys of the samples are written a second time, on the relaxed coordinates, under ``<key>_relaxed``.
    ``smiles=True`` writes ``smiles.csv`` to the output directory with one row per written sample file
    (``<uuid>/<i>_.<format>``): ``smiles`` of the sample without its pocket rows, ``linker_smiles`` of its linker as a molecule
    of its own, ``code`` (the canonical 64-bit code, hex) and ``canonical`` (0 when a search budget was hit or the bond list
    was flagged).  The strings describe the bond list the ``.sdf`` files carry (``bond_orders='geometric'`` and ``relax``
    apply), canonical under this project's own rule (``metrics.canonical_ranks``, ``molecule_builder.smiles``), NOT RDKit's
    canonical SMILES.  With ``metrics=True`` ``metrics.json`` gains ``smiles_uniqueness`` and ``smiles_canonical``
    (``metrics.compute_smiles``).

    ``filters='basic'`` or ``filters=FILE`` matches a catalogue of structural alerts against every sample and its true
    molecule, pocket rows left out (``metrics.analyze_patterns``; ``generate`` describes the catalogue), and writes
    ``filters.json`` to the output directory with one record per written sample file: ``file``, ``hits``, ``linker_hits`` and
    ``status``.  Always on the geometric bond orders and on the raw sample, whatever ``bond_orders`` and ``relax`` say.  With
    ``metrics=True`` ``metrics.json`` gains ``filters_passed`` (the reference's ``pains`` column as a fraction, on the catalogue
    given), ``filters_passed_linker``, ``filter_hits_per_molecule``, ``filters_budget`` and their ``true_`` values
    (``metrics.compute_filters``).  A SMARTS subset and a matcher of this project's own, NOT RDKit's."""
    select = _check_selection(cluster, pick, select_view)
    if hydrogens and output_format == 'xyz':
        raise ValueError('hydrogens are written to the .sdf files: pass output_format sdf or both (--output_format); the '
                         '.xyz files stay the heavy-atom format of the reference')
    n_hydrogens = []
    if output_format not in OUTPUT_FORMATS:
        raise ValueError(f'output_format must be one of {OUTPUT_FORMATS}, got {output_format!r}')
    if bond_orders not in BOND_ORDERS:
        raise ValueError(f'bond_orders must be one of {BOND_ORDERS}, got {bond_orders!r}')
    pred_aromatic, true_aromatic = [], []
    pred_poses, true_poses = [], []
    relax_records, relaxed_poses, relax_names = [], [], []
    found, pred, true, input_index = [], [], [], []
    pred_x, true_x, n_linker = [], [], []
    pred_clashes, true_clashes = [], []
    pred_contacts, true_contacts = [], []
    shapes, linker_shapes = [], []
    pharm, linker_pharm = [], []
    pred_rings, true_rings = [], []
    catalogue = mol_metrics.load_filters(filters) if filters is not None else None
    pred_filters, true_filters, filter_names = [], [], []
    pred_prints, true_prints, print_input = [], [], []
    eligible, select_input, select_names = [], [], []
    smiles_rows, smiles_names = [], []
    stereo_rows, true_stereo_rows, stereo_names, stereo_input = [], [], [], []
    diversity = diversity or diversity_reference is not None
    geometry = geometry and metrics
    exp = 'model' if isinstance(checkpoint, DDPM) else checkpoint.split('/')[-1].replace('.ckpt', '')
    collate_fn, sample_fn = collate, None
    if linker_size_model is None:
        output_dir = os.path.join(samples, prefix, exp)
    else:
        if isinstance(linker_size_model, SizeClassifier):
            size_nn, size_name = linker_size_model, 'size_model'
        else:
            size_nn = SizeClassifier.load_from_checkpoint(linker_size_model, map_location=device)
            size_name = linker_size_model.split('/')[-1].replace('.ckpt', '')
        size_nn = size_nn.eval().to(device)
        output_dir = os.path.join(samples, prefix, 'sampled_size', size_name, exp)
        collate_fn = collate_with_fragment_edges

        def sample_fn(_data):                                  # sample.py:70-80 (long sizes, loss discarded)
            output, _ = size_nn.forward(_data)
            samples_ = torch.distributions.Categorical(probs=torch.softmax(output, dim=1)).sample()
            sizes = [size_nn.linker_id2size[label] for label in samples_.detach().cpu().numpy()]
            return torch.tensor(sizes, device=samples_.device, dtype=torch.long)
    os.makedirs(output_dir, exist_ok=True)

    model = _prepare(checkpoint, prefix, data, n_steps, device)
    moad = isinstance(model.val_dataset, MOADDataset)
    if clashes and not (len(model.val_dataset) and 'pocket_mask' in model.val_dataset[0]):
        raise ValueError('clashes are scored against the pocket atoms: this data set has no pocket_mask')
    if interactions and not (len(model.val_dataset) and 'pocket_mask' in model.val_dataset[0]):
        raise ValueError('interactions are scored against the pocket atoms: this data set has no pocket_mask')
    for batch_idx, batch in enumerate(model.val_dataloader(collate_fn=collate_fn)):
        uuids = [str(u) for u in batch['uuid']]
        for u in uuids:
            os.makedirs(os.path.join(output_dir, u), exist_ok=True)
        generated, starting_point = check_if_generated(output_dir, uuids, n_samples)
        if generated:
            continue
        h, x, node_mask, frag_mask = batch['one_hot'], batch['positions'], batch['atom_mask'], batch['fragment_mask']
        if moad and model.center_of_mass == 'fragments':
            com_mask = batch['fragment_only_mask']
        elif model.center_of_mass == 'fragments':
            com_mask = batch['fragment_mask']
        elif model.center_of_mass == 'anchors':
            com_mask = batch['anchors']
        else:
            raise NotImplementedError(model.center_of_mass)
        x = utils.remove_partial_mean_with_mask(x, node_mask, com_mask)
        if moad:
            node_mask = batch['atom_mask'] - batch['pocket_mask']
            frag_mask = batch['fragment_only_mask']
            save_xyz_file(output_dir, h, x, batch['pocket_mask'], [f'{u}/pock' for u in uuids], is_geom=model.is_geom)
        save_xyz_file(output_dir, h, x, node_mask, [f'{u}/true' for u in uuids], is_geom=model.is_geom)
        save_xyz_file(output_dir, h, x, frag_mask, [f'{u}/frag' for u in uuids], is_geom=model.is_geom)
        if metrics:                                            # the true molecules as the files show them: without the pocket
            true_batch = mol_metrics.to_host(mol_metrics.analyze(h, x, node_mask, model.is_geom), h, node_mask)
        if clashes:                                            # the data set's own linker in the same pocket
            true_clash_batch = mol_metrics.clashes_to_host(mol_metrics.analyze_clashes(
                h[:, :, :model.num_classes], x, batch['linker_mask'], batch['pocket_mask'], is_geom=model.is_geom))
        if interactions:                                       # likewise; typed in the context of the whole true ligand
            true_contact_batch = mol_metrics.interactions_to_host(mol_metrics.analyze_interactions(
                h[:, :, :model.num_classes], x, batch['linker_mask'], batch['atom_mask'] - batch['pocket_mask'],
                batch['pocket_mask'], is_geom=model.is_geom))
        if rings:                                              # the data set's own molecule, without the pocket
            true_ring_batch = mol_metrics.rings_to_host(*mol_metrics.analyze_rings(
                h[:, :, :model.num_classes], x, node_mask, model.is_geom, batch['linker_mask']))
        if aromatic:
            true_aromatic_batch = mol_metrics.aromatic_to_host(mol_metrics.analyze_aromatic(
                h[:, :, :model.num_classes], x, node_mask, model.is_geom, batch['linker_mask']))
        if filters is not None:                                # the data set's own molecule, without the pocket
            true_filter_batch = mol_metrics.patterns_to_host(mol_metrics.analyze_patterns(
                h[:, :, :model.num_classes], x, node_mask, model.is_geom, batch['linker_mask'], catalogue,
                drop_mask=batch['pocket_mask'] if moad else None), catalogue.names)
        if stereo:                                             # the data set's own molecule, without the pocket
            true_stereo_batch = mol_metrics.analyze_stereo(h[:, :, :model.num_classes], x, node_mask, model.is_geom,
                                                           batch['linker_mask'], drop_mask=batch['pocket_mask'] if moad else None)
        if pose_checks:
            true_pose_batch = mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                h[:, :, :model.num_classes], x, node_mask, model.is_geom, batch['linker_mask'],
                drop_mask=batch['pocket_mask'] if moad else None))
        if diversity:                                          # likewise; one row per input, kept on the device
            true_prints.append(mol_metrics.analyze_fingerprints(
                h[:, :, :model.num_classes], x, node_mask, model.is_geom, batch['linker_mask']))
        if geometry:
            true_x_batch = list(mol_metrics.kept_positions(x, node_mask)[0])
            n_linker_batch = batch['linker_mask'].reshape(len(uuids), -1).sum(1).long().tolist()
        for i in range(starting_point, n_samples):
            chain, out_mask = model.sample_chain(batch, sample_fn=sample_fn, keep_frames=1)
            xs, hs = chain[0][:, :, :model.n_dims], chain[0][:, :, model.n_dims:]
            if clashes:                                        # the template's linker rows against its pocket rows
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_clashes += mol_metrics.clashes_to_host(mol_metrics.analyze_clashes(
                    hs[:, :, :model.num_classes], xs, out_mask * (1 - pad(batch['fragment_mask'])), pad(batch['pocket_mask']),
                    is_geom=model.is_geom))
                true_clashes += true_clash_batch
            if interactions:                                   # the same rows; the ligand is the template without its pocket
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_contacts += mol_metrics.interactions_to_host(mol_metrics.analyze_interactions(
                    hs[:, :, :model.num_classes], xs, out_mask * (1 - pad(batch['fragment_mask'])),
                    out_mask * (1 - pad(batch['pocket_mask'])), pad(batch['pocket_mask']), is_geom=model.is_geom))
                true_contacts += true_contact_batch
            shown_xs = xs                                      # what the files are written with; every score stays on xs
            if relax is not None:                              # the linker cleaned up, the template's pocket rows as the wall
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                linker_rows = out_mask * (1 - pad(batch['fragment_mask']))
                relaxed = relax_samples(hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, linker_rows,
                                        drop_mask=pad(batch['pocket_mask']) if moad else None, steps=relax)
                shown_xs = torch.where(linker_rows.bool(), relaxed.x, xs)       # every other row as it was, bit for bit
            if moad:
                pock = batch['pocket_mask']
                if pock.shape[1] < out_mask.shape[1]:          # template wider than the input (sampled sizes)
                    pock = torch.nn.functional.pad(pock, (0, 0, 0, out_mask.shape[1] - pock.shape[1]))
                out_mask = out_mask - pock
            if relax is not None:                              # did the clean-up change the distance table's bond list?
                types = hs[:, :, :model.num_classes]
                relax_records += mol_metrics.relax_to_host(relaxed, perceive_bonds(types, xs, out_mask, model.is_geom),
                                                           perceive_bonds(types, shown_xs, out_mask, model.is_geom))
                relax_names += [[f'{u}/{i}_.{ext}' for ext in ('xyz', 'sdf') if output_format in (ext, 'both')] for u in uuids]
            if shape:                                          # the sample against the true molecule, where both lie
                types, true_types = hs[:, :, :model.num_classes], h[:, :, :model.num_classes]
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                shapes += mol_metrics.shapes_to_host(mol_metrics.analyze_shapes(
                    types, xs, out_mask, true_types, x, node_mask, is_geom=model.is_geom))
                linker_shapes += mol_metrics.shapes_to_host(mol_metrics.analyze_shapes(
                    types, xs, out_mask * (1 - pad(batch['fragment_mask'])), true_types, x, batch['linker_mask'],
                    is_geom=model.is_geom))
            if pharmacophore:                                  # the same pairs and rows; the linker rows marked
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                whole, linker = mol_metrics.pharmacophores_to_host(mol_metrics.analyze_pharmacophores(
                    hs[:, :, :model.num_classes], xs, out_mask, out_mask * (1 - pad(batch['fragment_mask'])),
                    h[:, :, :model.num_classes], x, node_mask, batch['linker_mask'], is_geom=model.is_geom))
                pharm += whole
                linker_pharm += linker
            if rings:                                          # out_mask holds no pocket row here
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_rings += mol_metrics.rings_to_host(*mol_metrics.analyze_rings(
                    hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask']))))
                true_rings += true_ring_batch
            if filters is not None:                            # on the raw sample and the geometric orders, always
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_filters += mol_metrics.patterns_to_host(mol_metrics.analyze_patterns(
                    hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask'])),
                    catalogue), catalogue.names)
                true_filters += true_filter_batch
                filter_names += [[f'{u}/{i}_.{ext}' for ext in ('xyz', 'sdf') if output_format in (ext, 'both')] for u in uuids]
            if aromatic:                                       # likewise
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_aromatic += mol_metrics.aromatic_to_host(mol_metrics.analyze_aromatic(
                    hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask']))))
                true_aromatic += true_aromatic_batch
            if pose_checks:                                    # likewise; the pocket rows, gone from out_mask, dropped as well
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_poses += mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                    hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask'])),
                    drop_mask=pad(batch['pocket_mask']) if moad else None))
                true_poses += true_pose_batch
                if relax is not None:                          # the same checks once more, on what the files hold
                    relaxed_poses += mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                        hs[:, :, :model.num_classes], shown_xs, out_mask, model.is_geom,
                        out_mask * (1 - pad(batch['fragment_mask'])), drop_mask=pad(batch['pocket_mask']) if moad else None))
            if diversity or select:                            # likewise
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                pred_prints.append(mol_metrics.analyze_fingerprints(
                    hs[:, :, :model.num_classes], xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask']))))
                print_input += [(batch_idx, k) for k in range(len(uuids))]
            if select:                                         # only valid molecules in one piece are clustered and picked
                types = hs[:, :, :model.num_classes]
                eligible += mol_metrics.good_molecules(mol_metrics.to_host(
                    mol_metrics.analyze(types, xs, out_mask, model.is_geom), types, out_mask))
                select_input += uuids
                select_names += [[f'{u}/{i}_.{ext}' for ext in ('xyz', 'sdf') if output_format in (ext, 'both')] for u in uuids]
            if output_format != 'sdf':
                save_xyz_file(output_dir, hs, shown_xs, out_mask, [f'{u}/{i}' for u in uuids], is_geom=model.is_geom)
            if output_format != 'xyz':
                found.append(perceive_all_bonds(hs, shown_xs, out_mask, model.is_geom))
                shown = found[-1]
                planar = None
                if bond_orders == 'geometric':                 # Kekule orders for the planar rings, from the same geometry
                    shown, ring_atoms = refine_bond_orders(shown, hs[:, :, :model.num_classes], shown_xs, out_mask, model.is_geom)
                    planar = ring_atoms.atom_aromatic
                more = {}
                if hydrogens:                                  # on the list the file is written with
                    more['hydrogens'] = add_hydrogens(shown, hs[:, :, :model.num_classes], shown_xs, out_mask, model.is_geom,
                                                      atom_planar=planar)
                    n_hydrogens.append(more['hydrogens'].n_h)
                save_sdf_file(output_dir, hs, shown_xs, out_mask, shown.bonds, shown.n_bonds, [f'{u}/{i}' for u in uuids],
                              is_geom=model.is_geom, **more)
            if smiles:                                         # of the bond list the .sdf files carry (or would carry)
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                types = hs[:, :, :model.num_classes]
                listed = perceive_all_bonds(hs, shown_xs, out_mask, model.is_geom)
                if bond_orders == 'geometric':
                    listed = refine_bond_orders(listed, types, shown_xs, out_mask, model.is_geom)[0]
                smiles_rows += mol_metrics.smiles_records(types, out_mask, listed, out_mask * (1 - pad(batch['fragment_mask'])))
                smiles_names += [[f'{u}/{i}_.{ext}' for ext in ('xyz', 'sdf') if output_format in (ext, 'both')] for u in uuids]
            if stereo:                                         # on the coordinates the files carry; always the geometric orders
                pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, out_mask.shape[1] - m.shape[1]))      # noqa: E731
                stereo_rows += mol_metrics.analyze_stereo(
                    hs[:, :, :model.num_classes], shown_xs, out_mask, model.is_geom, out_mask * (1 - pad(batch['fragment_mask'])),
                    drop_mask=pad(batch['pocket_mask']) if moad else None)
                true_stereo_rows += true_stereo_batch
                stereo_input += [(batch_idx, k) for k in range(len(uuids))]
                stereo_names += [[f'{u}/{i}_.{ext}' for ext in ('xyz', 'sdf') if output_format in (ext, 'both')] for u in uuids]
            if metrics:
                types = hs[:, :, :model.num_classes]
                pred += mol_metrics.to_host(mol_metrics.analyze(types, xs, out_mask, model.is_geom), types, out_mask)
                true += true_batch
                input_index += [(batch_idx, k) for k in range(len(uuids))]
            if geometry:
                pred_x += list(mol_metrics.kept_positions(xs, out_mask)[0])
                true_x += true_x_batch
                n_linker += n_linker_batch
    if found:
        line = summary(found)
        if hydrogens:
            line['hydrogens_per_molecule'] = float(torch.cat(n_hydrogens).float().mean()) if line['molecules'] else 0.0
        print(json.dumps(line))
    if select:                                                 # groups are the inputs
        selection = _selection_records(pred_prints, select_input, eligible, select_view, cluster, pick)
        if pick is not None:
            with open(os.path.join(output_dir, 'selection.json'), 'w') as f:
                json.dump(mol_metrics.selection_report(selection, select_names), f, indent=1)
    if smiles:                                                 # one row per written file
        mol_metrics.write_smiles_csv(os.path.join(output_dir, 'smiles.csv'), [path for paths in smiles_names for path in paths],
                                     [m for m, paths in zip(smiles_rows, smiles_names) for _ in paths],
                                     *([[m.isomeric_smiles for m, paths in zip(stereo_rows, stereo_names) for _ in paths]]
                                       if stereo else []))
    if stereo:                                                 # one record per written file
        mol_metrics.write_stereo_json(os.path.join(output_dir, 'stereo.json'), [path for paths in stereo_names for path in paths],
                                      [m for m, paths in zip(stereo_rows, stereo_names) for _ in paths])
    if filters is not None:                                    # one record per written file
        mol_metrics.write_filters_json(os.path.join(output_dir, 'filters.json'),
                                       [path for paths in filter_names for path in paths],
                                       [m for m, paths in zip(pred_filters, filter_names) for _ in paths])
    if relax is not None:                                      # one record per written file
        with open(os.path.join(output_dir, 'relax.json'), 'w') as f:
            json.dump({path: mol_metrics.relax_report(m) for m, paths in zip(relax_records, relax_names) for path in paths}, f, indent=1)
    if (metrics or clashes or shape or rings or aromatic or diversity or pharmacophore or interactions or pose_checks or select
            or relax is not None):
        with open(os.path.join(output_dir, 'metrics.json'), 'w') as f:
            scores = {}
            if metrics:
                scores = dict(mol_metrics.compute_metrics(pred, true, input_index), molecules=len(pred))
            if geometry:
                scores.update(mol_metrics.compute_geometry(pred, true, pred_x, true_x, n_linker))
            if clashes:
                scores.update(mol_metrics.compute_clashes(pred_clashes, true_clashes))
            if interactions:
                scores.update(mol_metrics.compute_interactions(pred_contacts, true_contacts))
            if shape:
                scores.update(mol_metrics.compute_shapes(shapes, linker_shapes, pred if metrics else None))
            if pharmacophore:
                scores.update(mol_metrics.compute_pharmacophores(pharm, linker_pharm, shapes if shape else None))
            if rings:
                scores.update(mol_metrics.compute_rings(pred_rings, true_rings))
            if aromatic:
                scores.update(mol_metrics.compute_aromatic(pred_aromatic, true_aromatic))
            if pose_checks:
                scores.update(mol_metrics.compute_pose_checks(pred_poses, true_poses))
                if relax is not None:
                    scores.update({f'{k}_relaxed': v for k, v in mol_metrics.compute_pose_checks(relaxed_poses).items()})
            if relax is not None:
                scores.update(mol_metrics.compute_relaxation(relax_records))
            if diversity:
                reference = None if diversity_reference is None else reference_fingerprints(model, diversity_reference)
                scores.update(_diversity_scores(pred_prints, true_prints, print_input, reference))
            if select:
                scores.update(mol_metrics.compute_selection(selection))
            if smiles and metrics:                             # over the samples uniqueness counts
                scores.update(mol_metrics.compute_smiles(smiles_rows, pred, true))
            if filters is not None and metrics:
                scores.update(mol_metrics.compute_filters(pred_filters, true_filters))
            if stereo and metrics:
                scores.update(mol_metrics.compute_stereo(stereo_rows, pred, true, true_stereo_rows, stereo_input))
            json.dump(scores, f, indent=1)
    return output_dir


def reference_fingerprints(model, prefix, radius=2, n_bits=2048):
    """The whole-molecule fingerprints (``metrics.fingerprints``, every atom a centre, pocket rows left out) of the data set
    ``prefix`` under the model's data path, computed once, batch by batch, and kept on the device: int32 ``[R, n_bits / 32]``,
    the molecules with a status bit left out."""
    from .datasets import ZincDataset
    dataset_type = MOADDataset if '.' in prefix else ZincDataset
    dataset = dataset_type(data_path=model.data_path, prefix=prefix, device=model.torch_device)
    rows = []
    for batch in get_dataloader(dataset, model.batch_size, collate_fn=collate):
        node_mask = batch['atom_mask'] - batch['pocket_mask'] if 'pocket_mask' in batch else batch['atom_mask']
        types = batch['one_hot'][:, :, :model.num_classes]
        found = perceive_all_bonds(types, batch['positions'], node_mask, model.is_geom)
        prints = mol_metrics.fingerprints(types, node_mask, found, radius=radius, n_bits=n_bits)
        rows.append(prints.bits[prints.status == 0])
    if not rows:
        return torch.zeros(0, n_bits // 32, dtype=torch.int32, device=model.torch_device)
    return torch.cat(rows).contiguous()


def _selection_records(pred_prints, input_index, eligible, view, cluster, pick):
    """``metrics.select_records`` of the per-batch ``(whole, linker)`` fingerprint pairs gathered while sampling."""
    if not pred_prints:
        return []
    whole, linker = (mol_metrics.cat_fingerprints([p[k] for p in pred_prints]) for k in range(2))
    return mol_metrics.select_records(whole, linker, input_index, eligible, view=view, threshold=cluster, k=pick)


def _diversity_scores(pred_prints, true_prints, input_index, reference=None):
    """``metrics.compute_diversity`` of the per-batch ``(whole, linker)`` fingerprint pairs gathered while sampling."""
    if not pred_prints:
        return mol_metrics.compute_diversity([], with_true=bool(true_prints) or None, with_reference=reference is not None)
    whole, linker = (mol_metrics.cat_fingerprints([p[k] for p in pred_prints]) for k in range(2))
    true = [None, None] if not true_prints else [mol_metrics.cat_fingerprints([p[k] for p in true_prints]) for k in range(2)]
    records = mol_metrics.diversity_records(whole, linker, input_index, true[0], true[1], reference)
    return mol_metrics.compute_diversity(records, with_true=bool(true_prints), with_reference=reference is not None)


def sample_trajectories(checkpoint, chains, prefix, keep_frames, device, data=None, n_steps=None, batch_size=32):
    """``sample_trajectories.py``: ``keep_frames`` frames of every chain as ``chains/<k>/<k>_<frame>_.xyz`` plus the
    final prediction and the ground truth under ``final_states/``.  The feature slice ``3:-1`` is the script's own
    (it assumes a trailing charge column)."""
    exp = 'model' if isinstance(checkpoint, DDPM) else checkpoint.split('/')[-1].replace('.ckpt', '')
    chains_dir = os.path.join(chains, exp, prefix, 'chains')
    final_dir = os.path.join(chains, exp, prefix, 'final_states')
    os.makedirs(chains_dir, exist_ok=True)
    os.makedirs(final_dir, exist_ok=True)
    model = _prepare(checkpoint, prefix, data, n_steps, device)
    start = 0
    for batch in get_dataloader(model.val_dataset, batch_size=batch_size):
        chain_batch, node_mask = model.sample_chain(batch, keep_frames=keep_frames)
        for i in range(len(batch['positions'])):
            chain = chain_batch[:, i, :, :]
            assert chain.shape[0] == keep_frames and chain.shape[1] == batch['positions'].shape[1]
            name = str(i + start)
            out = os.path.join(chains_dir, name)
            os.makedirs(out, exist_ok=True)
            frames_mask = torch.cat([node_mask[i].unsqueeze(0) for _ in range(keep_frames)], dim=0)
            save_xyz_file(out, chain[:, :, 3:-1], chain[:, :, :3], frames_mask,
                          names=[f'{name}_{j}' for j in range(keep_frames)], is_geom=model.is_geom)
            save_xyz_file(final_dir, batch['one_hot'][i].unsqueeze(0), batch['positions'][i].unsqueeze(0),
                          batch['atom_mask'][i].unsqueeze(0), names=[f'{name}_true'], is_geom=model.is_geom)
            save_xyz_file(final_dir, chain[0, :, 3:-1].unsqueeze(0), chain[0, :, :3].unsqueeze(0),
                          frames_mask[0].unsqueeze(0), names=[f'{name}_pred'], is_geom=model.is_geom)
        start += len(batch['positions'])
    return chains_dir, final_dir


def main(argv=None):
    p = argparse.ArgumentParser(description='DiffLinker dataset sampling on MI355X (sample.py / sample_trajectories.py)')
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--samples', required=True, help='output root (sample.py --samples / sample_trajectories.py --chains)')
    p.add_argument('--data', default=None)
    p.add_argument('--prefix', required=True)
    p.add_argument('--n_samples', type=int, default=1)
    p.add_argument('--n_steps', type=int, default=None)
    p.add_argument('--linker_size_model', default=None)
    p.add_argument('--keep_frames', type=int, default=None, help='trajectory mode: frames kept per chain')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--output_format', choices=OUTPUT_FORMATS, default='xyz',
                   help='format of the sampled molecules: xyz, sdf (V2000 with bonds perceived on the GPU) or both')
    p.add_argument('--metrics', action='store_true',
                   help='score the sampled molecules on the GPU (valence rule, connectivity, uniqueness, novelty, recovery) '
                        'and write metrics.json next to them')
    p.add_argument('--geometry', action='store_true',
                   help='with --metrics: add the symmetry-aware RMSD of the recovered samples against their true molecules '
                        '(rmsd, rmsd_molecules, rmsd_truncated)')
    p.add_argument('--clashes', action='store_true',
                   help='pocket data sets: count the steric clashes of the sampled linkers (and of the true ones) with the '
                        'pocket atoms on the GPU and write the scores to metrics.json')
    p.add_argument('--shape', action='store_true',
                   help='score every sample\'s gridded van der Waals volume against its true molecule on the GPU (this '
                        'project\'s grid after RDKit\'s defaults, not SC-RDKit) and write the scores to metrics.json')
    p.add_argument('--rings', action='store_true',
                   help='perceive the rings of every sample and of its true molecule on the GPU (ring count of the linker, '
                        'small rings, macrocycles; the cyclomatic number, no aromaticity) and write the scores to metrics.json')
    p.add_argument('--bond_orders', choices=BOND_ORDERS, default='distance',
                   help='bond orders of the .sdf files: distance (the distance table of the reference\'s molecule_builder) or '
                        'geometric (planar five- and six-rings get Kekule orders 1 / 2 from the 3D geometry; a rule of this '
                        'project, not OpenBabel\'s bond typing)')
    p.add_argument('--aromatic', action='store_true',
                   help='perceive aromatic rings of every sample and of its true molecule from the geometry on the GPU (a rule '
                        'of this project, not RDKit\'s) and write aromatic_rings_n, ring_filter and '
                        'valence_validity_geometric to metrics.json')
    p.add_argument('--diversity', action='store_true',
                   help='fingerprint every sample and every true molecule on the GPU (this project\'s circular fingerprint, '
                        'not RDKit\'s Morgan) and write internal_diversity, internal_diversity_linker, similarity_to_true and '
                        'similarity_to_true_linker to metrics.json')
    p.add_argument('--diversity_reference', default=None, metavar='PREFIX',
                   help='with --diversity: another data set under --data (typically the training set); every sample\'s '
                        'greatest similarity to it is written as nearest_reference_similarity / nearest_reference_identical')
    p.add_argument('--pharmacophore', action='store_true',
                   help='perceive the pharmacophore features of every sample and of its true molecule on the GPU and write their '
                        'feature-map score to metrics.json (feature_similarity, feature_similarity_linker; with --shape also '
                        'sc_similarity and sc_similarity_7/8/9 - this project\'s features after RDKit\'s BaseFeatures.fdef, not '
                        'SC-RDKit\'s numbers)')
    p.add_argument('--interactions', action='store_true',
                   help='pocket data sets: score the contacts of the sampled linkers (and of the true ones) with the pocket '
                        'atoms on the GPU - the intermolecular terms of Trott & Olson under this project\'s heavy-atom typing, '
                        'not AutoDock Vina\'s numbers - and write the scores to metrics.json')
    p.add_argument('--hydrogens', action='store_true',
                   help='add explicit hydrogens with 3D positions to the .sdf files on the GPU (needs --output_format sdf or '
                        'both; a rule of this project, not RDKit\'s AddHs and not OpenBabel\'s).  --bond_orders geometric is '
                        'recommended: the distance table\'s arbitrary orders inside aromatic rings give arbitrary hydrogen '
                        'counts there')
    add_selection_arguments(p)
    add_relax_argument(p)
    add_smiles_argument(p)
    add_stereo_argument(p)
    add_filters_argument(p)
    p.add_argument('--pose_checks', action='store_true',
                   help='check the internal geometry of every sample and of its true molecule on the GPU - bond lengths, bond '
                        'angles, clashes between atoms four or more bonds apart, always on the geometric bond orders (a rule of '
                        'this project after the idea of PoseBusters\' intramolecular checks, NOT PoseBusters\' numbers) - and '
                        'write pose_valid, its parts, their _linker variants and the true_ values to metrics.json')
    a = p.parse_args(argv)
    if a.keep_frames is not None:
        print(sample_trajectories(a.checkpoint, a.samples, a.prefix, a.keep_frames, a.device, a.data, a.n_steps))
    else:
        print(sample(a.checkpoint, a.samples, a.prefix, a.n_samples, a.device, a.data, a.n_steps, a.linker_size_model,
                     a.output_format, a.metrics, **({'geometry': True} if a.geometry else {}),
                     **({'clashes': True} if a.clashes else {}), **({'shape': True} if a.shape else {}),
                     **({'rings': True} if a.rings else {}),
                     **({'bond_orders': a.bond_orders} if a.bond_orders != 'distance' else {}),
                     **({'aromatic': True} if a.aromatic else {}), **({'diversity': True} if a.diversity else {}),
                     **({'diversity_reference': a.diversity_reference} if a.diversity_reference else {}),
                     **({'pharmacophore': True} if a.pharmacophore else {}),
                     **({'interactions': True} if a.interactions else {}),
                     **({'hydrogens': True} if a.hydrogens else {}),
                     **({'pose_checks': True} if a.pose_checks else {}),
                     **({'relax': a.relax} if a.relax is not None else {}), **({'smiles': True} if a.smiles else {}), **({'stereo': True} if a.stereo else {}),
                     **({'filters': a.filters} if a.filters is not None else {}),
                     **selection_arguments(a)))


if __name__ == '__main__':
    main()
