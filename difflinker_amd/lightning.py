"""``DDPM`` — the wrapper the reference's CLI scripts talk to (``src/lightning.py::DDPM``).

Hyper-parameter wiring (lightning.py:39-112), ``load_from_checkpoint`` for Lightning-format checkpoints
(``{'hyper_parameters', 'state_dict'}``), ``sample_chain`` (:405-463), and the evaluation of held-out data: ``forward``
(:148-199) with ``training=False``, ``validation_step`` / ``test_step`` (:228-268) and ``aggregate_metric`` (:478-480).
Training: ``training_step`` (:201-226) with a differentiable ``loss`` (``EDM.training_forward``, HIP backward of the
fully-connected denoiser), the random rotation of ``data_augmentation``, and ``configure_optimizers`` (:465-466);
``python -m difflinker_amd.train`` is the training loop.  Sample quality: ``sample_and_analyze`` (:322-403) with the
RDKit-free scores of ``metrics.py``, ``validation_epoch_end`` / ``test_epoch_end`` (:276-304) and
``compute_best_validation_metrics`` (:468-476).  RDKit metrics, animations, WandB and PL Trainer hooks are out of scope.
Subclasses ``pytorch_lightning.LightningModule`` when that package is importable (it is not in the
build image), else ``torch.nn.Module`` with the same surface the callers use
(generate.py:101-175, sample.py:84-164).
"""
import torch
import torch.nn as nn

from . import metrics as mol_metrics
from . import utils
from .datasets import MOADDataset, create_templates_for_linker_generation
from .edm import EDM, InpaintingEDM
from .egnn import Dynamics, DynamicsWithPockets

try:  # pragma: no cover
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:
    _Base = nn.Module


def get_activation(activation):
    """lightning.py:27-31."""
    if activation == 'silu':
        return nn.SiLU()
    raise Exception('activation fn not supported yet. Add it here.')


class DDPM(_Base):
    train_dataset = None
    val_dataset = None
    test_dataset = None
    starting_epoch = None
    FRAMES = 100

    def __init__(
        self,
        in_node_nf, n_dims, context_node_nf, hidden_nf, activation, tanh, n_layers, attention, norm_constant,
        inv_sublayers, sin_embedding, normalization_factor, aggregation_method,
        diffusion_steps, diffusion_noise_schedule, diffusion_noise_precision, diffusion_loss_type,
        normalize_factors, include_charges, model,
        data_path, train_data_prefix, val_data_prefix, batch_size, lr, torch_device, test_epochs, n_stability_samples,
        normalization=None, log_iterations=None, samples_dir=None, data_augmentation=False,
        center_of_mass='fragments', inpainting=False, anchors_context=True, graph_type=None,
    ):
        super().__init__()
        self.hparams_dict = {k: v for k, v in locals().items() if k not in ('self', '__class__')}
        if hasattr(self, 'save_hyperparameters') and _Base is not nn.Module:  # pragma: no cover
            self.save_hyperparameters()
        self.data_path = data_path
        self.train_data_prefix = train_data_prefix
        self.val_data_prefix = val_data_prefix
        self.batch_size = batch_size
        self.lr = lr
        self.torch_device = torch_device
        self.include_charges = include_charges
        self.test_epochs = test_epochs
        self.n_stability_samples = n_stability_samples
        self.log_iterations = log_iterations
        self.samples_dir = samples_dir
        self.data_augmentation = data_augmentation
        self.center_of_mass = center_of_mass
        self.inpainting = inpainting
        self.loss_type = diffusion_loss_type
        self.n_dims = n_dims
        self.num_classes = in_node_nf - include_charges
        self.anchors_context = anchors_context
        self.is_geom = ('geom' in self.train_data_prefix) or ('MOAD' in self.train_data_prefix)
        self.pockets = '.' in train_data_prefix              # MOAD prefixes look like 'MOAD_train.full'

        if graph_type is None:
            graph_type = '4A' if self.pockets else 'FC'
        if type(activation) is str:
            activation = get_activation(activation)
        dynamics_class = DynamicsWithPockets if self.pockets else Dynamics
        dynamics = dynamics_class(
            in_node_nf=in_node_nf, n_dims=n_dims, context_node_nf=context_node_nf, device=torch_device,
            hidden_nf=hidden_nf, activation=activation, n_layers=n_layers, attention=attention, tanh=tanh,
            norm_constant=norm_constant, inv_sublayers=inv_sublayers, sin_embedding=sin_embedding,
            normalization_factor=normalization_factor, aggregation_method=aggregation_method, model=model,
            normalization=normalization, centering=inpainting, graph_type=graph_type,
        )
        edm_class = InpaintingEDM if inpainting else EDM           # lightning.py:102
        self.edm = edm_class(
            dynamics=dynamics, in_node_nf=in_node_nf, n_dims=n_dims, timesteps=diffusion_steps,
            noise_schedule=diffusion_noise_schedule, noise_precision=diffusion_noise_precision,
            loss_type=diffusion_loss_type, norm_values=normalize_factors,
        )
        from .const import LINKER_SIZE_DIST
        from .linker_size import DistributionNodes
        self.linker_size_sampler = DistributionNodes(LINKER_SIZE_DIST)          # lightning.py:113
        self.metrics = {}                                                       # lightning.py:43: name -> value per epoch
        self.geometry_metrics = False           # sample_and_analyze adds metrics.compute_geometry's RMSD keys (train --geometry)
        self.clash_metrics = False              # pocket models: it adds metrics.compute_clashes' keys as well (train --clashes)
        self.interaction_metrics = False        # pocket models: metrics.compute_interactions' keys (train --interactions)
        self.shape_metrics = False              # it adds metrics.compute_shapes' keys: every sample against its true molecule (train --shape)
        self.pharmacophore_metrics = False      # it adds metrics.compute_pharmacophores' keys: feature-map score of every sample against its true molecule, sc_similarity with shape_metrics (train --pharmacophore)
        self.aromatic_metrics = False           # it adds metrics.compute_aromatic's keys: aromatic rings of the linker, ring filter, valence rule on geometric orders (train --aromatic)
        self.diversity_metrics = False          # it adds metrics.compute_diversity's keys: internal diversity of each input's samples, similarity to the true molecule (train --diversity)
        self.ring_metrics = False               # it adds metrics.compute_rings' keys: ring count of the linker, small rings, macrocycles (train --rings)
        self.pose_metrics = False               # it adds metrics.compute_pose_checks' keys: bond lengths, bond angles and internal clashes of every sample and of its true molecule (train --pose_checks)
        if _Base is nn.Module:
            self.current_epoch = 0              # Lightning's Trainer keeps this; here the training loop sets it

    # ---- checkpoints ----------------------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=True, **overrides):
        """Read a Lightning checkpoint written by the reference's ``ModelCheckpoint``
        (train_difflinker.py:96-101): ``hyper_parameters`` -> constructor, ``state_dict`` ->
        ``load_state_dict(strict)``."""
        if _Base is not nn.Module:  # pragma: no cover
            return super().load_from_checkpoint(checkpoint_path, map_location=map_location, strict=strict, **overrides)
        ckpt = torch.load(checkpoint_path, map_location=map_location or 'cpu', weights_only=False)
        hparams = dict(ckpt['hyper_parameters'])
        hparams.update(overrides)
        model = cls(**hparams)
        model.load_state_dict(ckpt['state_dict'], strict=strict)
        return model

    def checkpoint_dict(self):
        """The ``{'hyper_parameters', 'state_dict'}`` pair ``load_from_checkpoint`` reads."""
        return {'hyper_parameters': dict(self.hparams_dict), 'state_dict': self.state_dict()}

    def setup(self, stage=None):
        """Load the preprocessed dataset(s) (lightning.py:115-137); ``stage='val'`` is what the sampling scripts use."""
        from .datasets import MOADDataset, ZincDataset
        dataset_type = MOADDataset if '.' in self.train_data_prefix else ZincDataset
        if stage == 'fit':
            self.is_geom = ('geom' in self.train_data_prefix) or ('MOAD' in self.train_data_prefix)
            self.train_dataset = dataset_type(data_path=self.data_path, prefix=self.train_data_prefix, device=self.torch_device)
            self.val_dataset = dataset_type(data_path=self.data_path, prefix=self.val_data_prefix, device=self.torch_device)
        elif stage == 'val':
            self.is_geom = ('geom' in self.val_data_prefix) or ('MOAD' in self.val_data_prefix)
            self.val_dataset = dataset_type(data_path=self.data_path, prefix=self.val_data_prefix, device=self.torch_device)
        else:
            raise NotImplementedError

    def train_dataloader(self, collate_fn=None):
        from .datasets import collate, get_dataloader
        return get_dataloader(self.train_dataset, self.batch_size, collate_fn=collate_fn or collate, shuffle=True)

    def val_dataloader(self, collate_fn=None):
        from .datasets import collate, get_dataloader
        return get_dataloader(self.val_dataset, self.batch_size, collate_fn=collate_fn or collate)

    def test_dataloader(self, collate_fn=None):
        from .datasets import collate, get_dataloader
        return get_dataloader(self.test_dataset, self.batch_size, collate_fn=collate_fn or collate)

    # ---- evaluation of held-out data -------------------------------------------------------------------------
    def _context_and_com_mask(self, data, node_mask, fragment_mask, anchors):
        """Context and centre-of-mass mask (lightning.py:157-183).  Pocket data is recognised by ``self.pockets`` (a MOAD
        prefix), not by ``isinstance(self.train_dataset, MOADDataset)``: after ``setup('val')`` the train dataset is None,
        and the reference would then build the context of a pocket model without its pocket channels."""
        if self.anchors_context:
            context = torch.cat([anchors, fragment_mask], dim=-1)
        else:
            context = fragment_mask
        if self.pockets:
            fragment_only_mask = data['fragment_only_mask']
            pocket_only_mask = fragment_mask - fragment_only_mask
            if self.anchors_context:
                context = torch.cat([anchors, fragment_only_mask, pocket_only_mask], dim=-1)
            else:
                context = torch.cat([fragment_only_mask, pocket_only_mask], dim=-1)
        if self.inpainting:
            center_of_mass_mask = node_mask
        elif self.pockets and self.center_of_mass == 'fragments':
            center_of_mass_mask = data['fragment_only_mask']
        elif self.center_of_mass == 'fragments':
            center_of_mass_mask = fragment_mask
        elif self.center_of_mass == 'anchors':
            center_of_mass_mask = anchors
        else:
            raise NotImplementedError(self.center_of_mass)
        return context, center_of_mass_mask

    def forward(self, data, training=False, mol_offset=0):
        """``DDPM.forward`` (lightning.py:148-199) for evaluation: context, fragment centre of mass removed (and asserted
        zero), then ``self.edm.forward`` - the reference's 7-tuple.  ``training=True`` (data augmentation, a loss to
        back-propagate) is out of scope and raises; call it under ``torch.no_grad()`` (``validation_step`` does).
        Deviation: pocket context keyed on ``self.pockets`` (see ``_context_and_com_mask``), as in ``sample_chain``.
        ``mol_offset`` (not in the reference signature): global index of the batch's first molecule, for
        ``noise_source='philox'`` (``EDM.forward``)."""
        if training:
            raise NotImplementedError('DDPM.forward(training=True) is the training step: out of scope (no backward); '
                                      'evaluate with training=False, validation_step or test_step')
        x = data['positions']
        h = data['one_hot']
        node_mask = data['atom_mask']
        edge_mask = data['edge_mask']
        anchors = data['anchors']
        fragment_mask = data['fragment_mask']
        linker_mask = data['linker_mask']
        context, center_of_mass_mask = self._context_and_com_mask(data, node_mask, fragment_mask, anchors)
        x = utils.remove_partial_mean_with_mask(x, node_mask, center_of_mass_mask)
        utils.assert_partial_mean_zero_with_mask(x, node_mask, center_of_mass_mask)
        return self.edm.forward(x=x, h=h, node_mask=node_mask, fragment_mask=fragment_mask, linker_mask=linker_mask,
                                edge_mask=edge_mask, context=context, mol_offset=mol_offset)

    def _training_forward(self, data):
        """``forward(data, training=True)`` (lightning.py:148-199): context, fragment centre of mass removed, the random
        rotation when ``data_augmentation`` is on, then ``self.edm.training_forward`` (losses with a gradient)."""
        x = data['positions']
        node_mask = data['atom_mask']
        fragment_mask = data['fragment_mask']
        context, center_of_mass_mask = self._context_and_com_mask(data, node_mask, fragment_mask, data['anchors'])
        x = utils.remove_partial_mean_with_mask(x, node_mask, center_of_mass_mask)
        utils.assert_partial_mean_zero_with_mask(x, node_mask, center_of_mass_mask)
        if self.data_augmentation:
            x = utils.random_rotation(x)
        return self.edm.training_forward(x=x, h=data['one_hot'], node_mask=node_mask, fragment_mask=fragment_mask,
                                         linker_mask=data['linker_mask'], edge_mask=data['edge_mask'], context=context)

    def training_step(self, data, *args):
        """lightning.py:201-226: the 9 metrics of one batch; ``loss`` (``l2_loss`` or ``vlb_loss``) back-propagates to the
        denoiser's parameters."""
        delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = self._training_forward(data)
        vlb_loss = kl_prior + loss_term_t + loss_term_0 - delta_log_px
        if self.loss_type == 'l2':
            loss = l2_loss
        elif self.loss_type == 'vlb':
            loss = vlb_loss
        else:
            raise NotImplementedError(self.loss_type)
        return {'loss': loss, 'delta_log_px': delta_log_px, 'kl_prior': kl_prior, 'loss_term_t': loss_term_t,
                'loss_term_0': loss_term_0, 'l2_loss': l2_loss, 'vlb_loss': vlb_loss, 'noise_t': noise_t, 'noise_0': noise_0}

    def configure_optimizers(self):
        """lightning.py:465-466."""
        return torch.optim.AdamW(self.edm.parameters(), lr=self.lr, amsgrad=True, weight_decay=1e-12)

    def _metrics(self, data, mol_offset=0):
        with torch.no_grad():
            delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = self.forward(data, training=False,
                                                                                                      mol_offset=mol_offset)
        vlb_loss = kl_prior + loss_term_t + loss_term_0 - delta_log_px
        if self.loss_type == 'l2':
            loss = l2_loss
        elif self.loss_type == 'vlb':
            loss = vlb_loss
        else:
            raise NotImplementedError(self.loss_type)
        return {
            'loss': loss,
            'delta_log_px': delta_log_px,
            'kl_prior': kl_prior,
            'loss_term_t': loss_term_t,
            'loss_term_0': loss_term_0,
            'l2_loss': l2_loss,
            'vlb_loss': vlb_loss,
            'noise_t': noise_t,
            'noise_0': noise_0,
        }

    def validation_step(self, data, *args):
        """lightning.py:228-247: the 9 metrics of one batch (``loss`` = ``l2_loss`` or ``vlb_loss`` by ``loss_type``)."""
        return self._metrics(data)

    def test_step(self, data, *args):
        """lightning.py:249-268 (the same metrics as ``validation_step``)."""
        return self._metrics(data)

    @staticmethod
    def aggregate_metric(step_outputs, metric):
        """lightning.py:478-480: the mean of one metric over the step outputs."""
        return torch.tensor([float(out[metric]) for out in step_outputs]).mean()

    # ---- sample quality -------------------------------------------------------------------------------
    def _epoch_end(self, step_outputs, split, dataloader):
        now = {}
        for metric in (step_outputs[0].keys() if step_outputs else ()):
            now[f'{metric}/{split}'] = float(self.aggregate_metric(step_outputs, metric))
        if (self.current_epoch + 1) % self.test_epochs == 0:
            for name, value in self.sample_and_analyze(dataloader()).items():
                now[f'{name}/{split}'] = value
        for name, value in now.items():
            self.metrics.setdefault(name, []).append(value)
        return now

    def validation_epoch_end(self, validation_step_outputs):
        """lightning.py:276-292: the means of the step metrics go to ``self.metrics['<name>/val']``; every ``test_epochs``
        epochs the validation set is sampled and scored (``sample_and_analyze``) and those scores are stored the same way,
        followed by the metrics of the best epoch so far.  ``self.log`` does not exist here: returns what the reference
        logs, as a dict of floats."""
        now = self._epoch_end(validation_step_outputs, 'val', self.val_dataloader)
        if 'validity_and_connectivity/val' in now:
            best_metrics, best_epoch = self.compute_best_validation_metrics()
            now['best_epoch'] = int(best_epoch)
            now.update({f'best_{name}': value for name, value in best_metrics.items()})
        return now

    def test_epoch_end(self, test_step_outputs):
        """lightning.py:294-304: as ``validation_epoch_end`` on the test set, without the best-epoch lookup."""
        return self._epoch_end(test_step_outputs, 'test', self.test_dataloader)

    def compute_best_validation_metrics(self):
        """lightning.py:468-476: the position of the largest ``validity_and_connectivity/val`` and every ``*/val`` metric at
        that position.  As in the reference the position counts scored epochs, so with ``test_epochs > 1`` the step metrics
        it picks belong to an earlier epoch; a list too short for the position is left out."""
        scores = self.metrics['validity_and_connectivity/val']
        best_epoch = max(range(len(scores)), key=lambda k: (scores[k], -k))        # np.argmax: the first of equal maxima
        best_metrics = {name: values[best_epoch] for name, values in self.metrics.items()
                        if name.endswith('/val') and len(values) > best_epoch}
        return best_metrics, best_epoch

    def sample_and_analyze(self, dataloader):
        """lightning.py:322-403 with the scores of ``metrics.py`` in place of RDKit's: per batch ``n_stability_samples``
        chains; a ``FoundNaNException`` is printed in the reference's three formats and that sample is skipped; pocket
        models score the molecules without their pocket atoms; the true molecules and the final frames go through
        ``metrics.analyze`` and the result is ``metrics.compute_metrics`` over all of them (which drops the predictions whose
        true molecule is not valid and connected).  With ``self.geometry_metrics`` the symmetry-aware RMSD of the recovered
        samples (``metrics.compute_geometry``) is added: ``rmsd`` (``None`` when nothing recovered), ``rmsd_molecules``,
        ``rmsd_truncated``.  With ``self.clash_metrics`` a pocket model also gets the ``metrics.compute_clashes`` keys: the
        samples' linker atoms against the pocket atoms, and the data set's own linkers in the same pockets as ``true``.
        With ``self.interaction_metrics`` a pocket model likewise gets the ``metrics.compute_interactions`` keys: the contacts
        of the same rows under the intermolecular terms of Trott & Olson and this project's own typing (not AutoDock Vina's
        numbers), the linker typed within the whole ligand.
        With ``self.shape_metrics`` every sample's gridded van der Waals volume is compared with its true molecule's in the
        frame the two share (``metrics.compute_shapes``; pocket rows left out, once over all ligand rows and once over the
        linker rows).  With ``self.ring_metrics`` the rings of every sample and of its true molecule are perceived
        (``metrics.analyze_rings`` / ``compute_rings``; pocket rows dropped): the linker's ring count, small rings,
        macrocycles.  With ``self.pharmacophore_metrics`` the pharmacophore features of every sample are matched against its true
        molecule's (``metrics.analyze_pharmacophores`` / ``compute_pharmacophores``, this project's rule after RDKit's
        ``BaseFeatures.fdef``, not RDKit's numbers): ``feature_similarity(_linker)``, and ``sc_similarity`` when
        ``self.shape_metrics`` is set too.  With ``self.aromatic_metrics`` aromatic rings are perceived from the geometry and the ring bonds get
        Kekule orders (``metrics.analyze_aromatic`` / ``compute_aromatic``, a rule of this project's own, not RDKit's):
        ``aromatic_rings_n``, ``ring_filter``, ``valence_validity_geometric``.  With ``self.diversity_metrics`` every sample
        and every true molecule is fingerprinted (``metrics.analyze_fingerprints`` / ``compute_diversity``; this project's own
        circular fingerprint, not RDKit's Morgan; pocket rows dropped): ``internal_diversity`` and
        ``internal_diversity_linker`` among each input's samples, ``similarity_to_true`` and ``similarity_to_true_linker``.
        With ``self.pose_metrics`` the internal geometry of every sample and of its true molecule is checked
        (``metrics.analyze_pose_checks`` / ``compute_pose_checks``; a rule of this project's own after the idea of PoseBusters'
        intramolecular checks, NOT PoseBusters' numbers; pocket rows dropped, the linker rows marked): ``pose_valid``,
        ``bond_lengths_valid``, ``bond_angles_valid``, ``internal_clash_free``, their ``_linker`` variants, the per-molecule
        means and the ``true_`` values.
        No animation, no WandB."""
        pred, true, input_index = [], [], []
        pred_poses, true_poses = [], []
        pred_aromatic, true_aromatic = [], []
        pred_rings, true_rings = [], []
        pred_prints, true_prints, print_input = [], [], []
        shapes, linker_shapes = [], []
        pharm, linker_pharm = [], []
        pred_x, true_x, n_linker = [], [], []
        clashes = self.clash_metrics and self.pockets
        pred_clashes, true_clashes = [], []
        contacts = self.interaction_metrics and self.pockets
        pred_contacts, true_contacts = [], []
        first = 0
        for b, data in enumerate(dataloader):
            drop = data['pocket_mask'] if self.pockets else None                   # lightning.py:331-334
            n = len(data['positions'])
            true_batch = mol_metrics.to_host(
                mol_metrics.analyze(data['one_hot'], data['positions'], data['atom_mask'], self.is_geom, drop_mask=drop),
                data['one_hot'], data['atom_mask'], drop)
            if clashes:
                true_clash_batch = mol_metrics.clashes_to_host(mol_metrics.analyze_clashes(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['linker_mask'], drop, is_geom=self.is_geom))
            if contacts:
                true_contact_batch = mol_metrics.interactions_to_host(mol_metrics.analyze_interactions(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['linker_mask'], data['atom_mask'] - drop,
                    drop, is_geom=self.is_geom))
            if self.ring_metrics:
                true_ring_batch = mol_metrics.rings_to_host(*mol_metrics.analyze_rings(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['atom_mask'], self.is_geom,
                    data['linker_mask'], drop_mask=drop))
            if self.aromatic_metrics:
                true_aromatic_batch = mol_metrics.aromatic_to_host(mol_metrics.analyze_aromatic(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['atom_mask'], self.is_geom,
                    data['linker_mask'], drop_mask=drop))
            if self.pose_metrics:
                true_pose_batch = mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['atom_mask'], self.is_geom,
                    data['linker_mask'], drop_mask=drop))
            if self.diversity_metrics:                                             # one row per input, kept on the device
                true_prints.append(mol_metrics.analyze_fingerprints(
                    data['one_hot'][:, :, :self.num_classes], data['positions'], data['atom_mask'], self.is_geom,
                    data['linker_mask'], drop_mask=drop))
                sampled = len(print_input)
            if self.geometry_metrics:
                true_x_batch = list(mol_metrics.kept_positions(data['positions'], data['atom_mask'], drop)[0])
                n_linker_batch = data['linker_mask'].reshape(n, -1).sum(1).long().tolist()
            for sample_idx in range(self.n_stability_samples):
                try:
                    chain_batch, node_mask = self.sample_chain(data, keep_frames=1)
                except utils.FoundNaNException as e:
                    for idx in e.x_h_nan_idx:
                        print(f"FoundNaNException: [xh], e={self.current_epoch}, b={b}, i={idx}: {data['name'][idx]}")
                    for idx in e.only_x_nan_idx:
                        print(f"FoundNaNException: [x ], e={self.current_epoch}, b={b}, i={idx}: {data['name'][idx]}")
                    for idx in e.only_h_nan_idx:
                        print(f"FoundNaNException: [ h], e={self.current_epoch}, b={b}, i={idx}: {data['name'][idx]}")
                    continue
                x = chain_batch[0][:, :, :self.n_dims]
                one_hot = chain_batch[0][:, :, self.n_dims:self.n_dims + self.num_classes]
                out_drop = drop
                if drop is not None and drop.shape[1] < node_mask.shape[1]:        # a template wider than the input
                    out_drop = torch.nn.functional.pad(drop, (0, 0, 0, node_mask.shape[1] - drop.shape[1]))
                pred += mol_metrics.to_host(mol_metrics.analyze(one_hot, x, node_mask, self.is_geom, drop_mask=out_drop),
                                            one_hot, node_mask, out_drop)
                true += true_batch
                input_index += range(first, first + n)
                if clashes:                                                        # the template's linker rows
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_clashes += mol_metrics.clashes_to_host(mol_metrics.analyze_clashes(
                        one_hot, x, node_mask * (1 - frag), out_drop, is_geom=self.is_geom))
                    true_clashes += true_clash_batch
                if contacts:                                                       # the same rows; the ligand: all but the pocket
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_contacts += mol_metrics.interactions_to_host(mol_metrics.analyze_interactions(
                        one_hot, x, node_mask * (1 - frag), node_mask * (1 - out_drop), out_drop, is_geom=self.is_geom))
                    true_contacts += true_contact_batch
                if self.shape_metrics:
                    shapes += self._shape_records(data, one_hot, x, node_mask, drop, out_drop, linker=False)
                    linker_shapes += self._shape_records(data, one_hot, x, node_mask, drop, out_drop, linker=True)
                if self.pharmacophore_metrics:
                    whole, linker = self._pharmacophore_records(data, one_hot, x, node_mask, drop, out_drop)
                    pharm += whole
                    linker_pharm += linker
                if self.ring_metrics:                                              # the template's linker rows marked
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_rings += mol_metrics.rings_to_host(*mol_metrics.analyze_rings(
                        one_hot, x, node_mask, self.is_geom, node_mask * (1 - frag), drop_mask=out_drop))
                    true_rings += true_ring_batch
                if self.aromatic_metrics:                                          # the template's linker rows marked
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_aromatic += mol_metrics.aromatic_to_host(mol_metrics.analyze_aromatic(
                        one_hot, x, node_mask, self.is_geom, node_mask * (1 - frag), drop_mask=out_drop))
                    true_aromatic += true_aromatic_batch
                if self.pose_metrics:                                              # the template's linker rows marked
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_poses += mol_metrics.pose_checks_to_host(mol_metrics.analyze_pose_checks(
                        one_hot, x, node_mask, self.is_geom, node_mask * (1 - frag), drop_mask=out_drop))
                    true_poses += true_pose_batch
                if self.diversity_metrics:                                         # the template's linker rows the centres
                    frag = torch.nn.functional.pad(data['fragment_mask'], (0, 0, 0, node_mask.shape[1] - data['fragment_mask'].shape[1]))
                    pred_prints.append(mol_metrics.analyze_fingerprints(
                        one_hot, x, node_mask, self.is_geom, node_mask * (1 - frag), drop_mask=out_drop))
                    print_input += range(first, first + n)
                if self.geometry_metrics:
                    pred_x += list(mol_metrics.kept_positions(x, node_mask, out_drop)[0])
                    true_x += true_x_batch
                    n_linker += n_linker_batch
            if self.diversity_metrics and len(print_input) == sampled:             # every chain of the batch failed: its true
                true_prints.pop()                                                  # molecules would have no samples to go with
            first += n
        scores = mol_metrics.compute_metrics(pred, true, input_index)
        if self.geometry_metrics:
            scores.update(mol_metrics.compute_geometry(pred, true, pred_x, true_x, n_linker))
        if clashes:
            scores.update(mol_metrics.compute_clashes(pred_clashes, true_clashes))
        if contacts:
            scores.update(mol_metrics.compute_interactions(pred_contacts, true_contacts))
        if self.shape_metrics:
            scores.update(mol_metrics.compute_shapes(shapes, linker_shapes, pred))
        if self.pharmacophore_metrics:
            scores.update(mol_metrics.compute_pharmacophores(pharm, linker_pharm, shapes if self.shape_metrics else None))
        if self.ring_metrics:
            scores.update(mol_metrics.compute_rings(pred_rings, true_rings))
        if self.aromatic_metrics:
            scores.update(mol_metrics.compute_aromatic(pred_aromatic, true_aromatic))
        if self.pose_metrics:
            scores.update(mol_metrics.compute_pose_checks(pred_poses, true_poses))
        if self.diversity_metrics:
            records = []
            if pred_prints:
                whole, linker, true_whole, true_linker = (mol_metrics.cat_fingerprints([p[k] for p in parts])
                                                          for parts in (pred_prints, true_prints) for k in range(2))
                records = mol_metrics.diversity_records(whole, linker, print_input, true_whole, true_linker)
            scores.update(mol_metrics.compute_diversity(records, with_true=True, with_reference=False))
        return scores

    def _true_positions(self, data):
        """The data set's positions moved as ``sample_chain`` moves its input (centred on ``center_of_mass``), so that a sample
        and its true molecule share the fragments' coordinates."""
        if self.inpainting:                                                        # the conditions of ``sample_chain``
            com_mask = data['atom_mask']
        elif isinstance(self.val_dataset, MOADDataset) and self.center_of_mass == 'fragments':
            com_mask = data['fragment_only_mask']
        elif self.center_of_mass == 'fragments':
            com_mask = data['fragment_mask']
        elif self.center_of_mass == 'anchors':
            com_mask = data['anchors']
        else:
            raise NotImplementedError(self.center_of_mass)
        return utils.remove_partial_mean_with_mask(data['positions'], data['atom_mask'], com_mask)

    def _pharmacophore_records(self, data, one_hot, x, node_mask, drop, out_drop):
        """``metrics.pharmacophores_to_host`` of a sampled batch against the data set's molecules, in the frame of
        ``_shape_records``: the linker rows marked, the pocket rows dropped on both sides."""
        pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, node_mask.shape[1] - m.shape[1]))      # noqa: E731
        return mol_metrics.pharmacophores_to_host(mol_metrics.analyze_pharmacophores(
            one_hot, x, node_mask, node_mask * (1 - pad(data['fragment_mask'])), data['one_hot'][:, :, :self.num_classes],
            self._true_positions(data), data['atom_mask'], data['linker_mask'], is_geom=self.is_geom, drop_a=out_drop, drop_b=drop))

    def _shape_records(self, data, one_hot, x, node_mask, drop, out_drop, linker):
        """``metrics.ShapeRecord`` per molecule of a sampled batch against the data set's molecule.  ``sample_chain`` centres
        its input on ``center_of_mass`` and the data set's positions are not centred, so the true molecule is moved the same
        way first: the two then share the fragments' coordinates.  Pocket rows take part on neither side."""
        true_x = self._true_positions(data)
        pad = lambda m: torch.nn.functional.pad(m, (0, 0, 0, node_mask.shape[1] - m.shape[1]))      # noqa: E731
        if linker:
            mask, true_mask = node_mask * (1 - pad(data['fragment_mask'])), data['linker_mask']
        else:
            mask = node_mask if out_drop is None else node_mask * (1 - out_drop)
            true_mask = data['atom_mask'] if drop is None else data['atom_mask'] * (1 - drop)
        return mol_metrics.shapes_to_host(mol_metrics.analyze_shapes(
            one_hot, x, mask, data['one_hot'][:, :, :self.num_classes], true_x, true_mask, is_geom=self.is_geom))

    # ---- sampling -------------------------------------------------------------------------------------
    def sample_chain(self, data, sample_fn=None, keep_frames=None):
        """``DDPM.sample_chain`` (lightning.py:405-463): linker sizes -> zero templates -> context ->
        fragment-COM removal -> ``EDM.sample_chain``.  Returns ``(chain, node_mask)``."""
        if sample_fn is None:
            linker_sizes = data['linker_mask'].sum(1).view(-1).int()
        else:
            linker_sizes = sample_fn(data)
        # inpainting re-draws the fragments around the given atoms: no templates (lightning.py:411-414)
        template_data = data if self.inpainting else create_templates_for_linker_generation(data, linker_sizes)

        x = template_data['positions']
        node_mask = template_data['atom_mask']
        edge_mask = template_data['edge_mask']
        h = template_data['one_hot']
        anchors = template_data['anchors']
        fragment_mask = template_data['fragment_mask']
        linker_mask = template_data['linker_mask']

        if self.anchors_context:
            context = torch.cat([anchors, fragment_mask], dim=-1)
        else:
            context = fragment_mask
        if self.pockets:
            fragment_only_mask = template_data['fragment_only_mask']
            pocket_only_mask = fragment_mask - fragment_only_mask
            if self.anchors_context:
                context = torch.cat([anchors, fragment_only_mask, pocket_only_mask], dim=-1)
            else:
                context = torch.cat([fragment_only_mask, pocket_only_mask], dim=-1)

        if self.inpainting:
            center_of_mass_mask = node_mask
        elif isinstance(self.val_dataset, MOADDataset) and self.center_of_mass == 'fragments':     # lightning.py:443
            center_of_mass_mask = template_data['fragment_only_mask']
        elif self.center_of_mass == 'fragments':
            center_of_mass_mask = fragment_mask
        elif self.center_of_mass == 'anchors':
            center_of_mass_mask = anchors
        else:
            raise NotImplementedError(self.center_of_mass)
        x = utils.remove_partial_mean_with_mask(x, node_mask, center_of_mass_mask)

        chain = self.edm.sample_chain(
            x=x, h=h, node_mask=node_mask, edge_mask=edge_mask, fragment_mask=fragment_mask,
            linker_mask=linker_mask, context=context, keep_frames=keep_frames,
        )
        return chain, node_mask
