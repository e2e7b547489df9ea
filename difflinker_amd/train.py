"""Train or fine-tune DiffLinker on the GPU: a plain loop in place of the reference's ``train_difflinker.py`` (which drives
PyTorch Lightning's ``Trainer``; Lightning is not needed here).

    python -m difflinker_amd.train --config configs/zinc_difflinker.yml --data DIR --checkpoints CKPT_DIR
                                   [--max_steps K | --n_epochs E] [--val_every V] [--resume CKPT]

The YAML keys are the reference's (``train_difflinker.py``: nf, n_layers, inv_sublayers, lr, batch_size, ...); command-line
options given explicitly override them.  Each step: ``training_step`` on a shuffled batch (``setup('fit')``), ``backward``
(HIP), ``AdamW.step`` (``configure_optimizers``).  Every ``--val_every`` steps and at the end the mean ``validation_step``
metrics are printed, and ``CKPT_DIR/last.ckpt`` is written in Lightning's format (``hyper_parameters``, ``state_dict``,
plus ``optimizer_states``, ``global_step`` and ``epoch`` for ``--resume``); ``DDPM.load_from_checkpoint`` reads it.

``--sample_every_epochs E`` (off by default) adds the reference's end-of-epoch scoring: after every epoch that the loop
finishes, ``DDPM.validation_epoch_end`` aggregates the validation metrics and, every E-th epoch, samples
``n_stability_samples`` linkers per validation molecule and scores them (``metrics.py``: valence rule, connectivity,
uniqueness, novelty, recovery).  The result is printed as one JSON line, ``last.ckpt`` is written, and it is copied to
``best.ckpt`` whenever ``validity_and_connectivity/val`` improves.  An epoch cut short by ``--max_steps`` is not scored.
"""
import argparse
import json
import os
import shutil

import torch

from .const import GEOM_NUMBER_OF_ATOM_TYPES, NUMBER_OF_ATOM_TYPES
from .lightning import DDPM

DEFAULTS = dict(train_data_prefix='zinc_final_train', val_data_prefix='zinc_final_val', model='egnn_dynamics',
                activation='silu', diffusion_steps=500, diffusion_noise_schedule='polynomial_2', diffusion_noise_precision=1e-5,
                diffusion_loss_type='l2', n_epochs=200, batch_size=128, lr=2e-4, n_layers=6, inv_sublayers=1, nf=128,
                tanh=True, attention=True, norm_constant=1, sin_embedding=False, normalize_factors=[1, 4, 1],
                include_charges=True, normalization_factor=1, aggregation_method='sum', test_epochs=1,
                n_stability_samples=500, normalization=None, log_iterations=None, data_augmentation=False,
                center_of_mass='fragments', inpainting=False, remove_anchors_context=False, seed=0, graph_type=None)


def build_model(cfg, data, device):
    """``DDPM`` from the reference's config keys (train_difflinker.py: in_node_nf / context_node_nf as it derives them)."""
    is_geom = ('geom' in cfg['train_data_prefix']) or ('MOAD' in cfg['train_data_prefix'])
    in_node_nf = (GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES) + int(cfg['include_charges'])
    anchors_context = not cfg['remove_anchors_context']
    context_node_nf = (2 if anchors_context else 1) + int('.' in cfg['train_data_prefix'])
    return DDPM(
        data_path=data, train_data_prefix=cfg['train_data_prefix'], val_data_prefix=cfg['val_data_prefix'],
        in_node_nf=in_node_nf, n_dims=3, context_node_nf=context_node_nf, hidden_nf=cfg['nf'], activation=cfg['activation'],
        n_layers=cfg['n_layers'], attention=cfg['attention'], tanh=cfg['tanh'], norm_constant=cfg['norm_constant'],
        inv_sublayers=cfg['inv_sublayers'], sin_embedding=cfg['sin_embedding'],
        normalization_factor=cfg['normalization_factor'], aggregation_method=cfg['aggregation_method'],
        diffusion_steps=cfg['diffusion_steps'], diffusion_noise_schedule=cfg['diffusion_noise_schedule'],
        diffusion_noise_precision=cfg['diffusion_noise_precision'], diffusion_loss_type=cfg['diffusion_loss_type'],
        normalize_factors=cfg['normalize_factors'], include_charges=cfg['include_charges'], model=cfg['model'],
        batch_size=cfg['batch_size'], lr=cfg['lr'], torch_device=device, test_epochs=cfg['test_epochs'],
        n_stability_samples=cfg['n_stability_samples'], normalization=cfg['normalization'],
        log_iterations=cfg['log_iterations'], data_augmentation=cfg['data_augmentation'],
        center_of_mass=cfg['center_of_mass'], inpainting=cfg['inpainting'], anchors_context=anchors_context,
        graph_type=cfg['graph_type'])


def validate(model):
    metrics = [model.validation_step(data) for data in model.val_dataloader()]
    return {k: float(DDPM.aggregate_metric(metrics, k)) for k in metrics[0]} if metrics else {}


BEST_KEY = 'validity_and_connectivity/val'


def save(model, opt, path, step, epoch, **extra):
    ckpt = model.checkpoint_dict()
    ckpt.update(optimizer_states=[opt.state_dict()], global_step=step, epoch=epoch, **extra)
    tmp = path + '.tmp'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def main(argv=None):
    p = argparse.ArgumentParser(description='DiffLinker training on MI355X (HIP forward and backward)')
    p.add_argument('--config', type=argparse.FileType('r'), default=None)
    p.add_argument('--data', default='datasets')
    p.add_argument('--checkpoints', default='checkpoints')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--max_steps', type=int, default=None, help='stop after this many optimiser steps')
    p.add_argument('--n_epochs', type=int, default=None)
    p.add_argument('--batch_size', type=int, default=None)
    p.add_argument('--lr', type=float, default=None)
    p.add_argument('--val_every', type=int, default=0, help='validate and checkpoint every V steps (0: at the end only)')
    p.add_argument('--no_validation', action='store_true')
    p.add_argument('--resume', default=None, help='checkpoint of this loop to continue from')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--sample_every_epochs', type=int, default=0,
                   help='score the validation set at the end of every epoch and sample it every E-th epoch; keeps best.ckpt '
                        '(0: off)')
    p.add_argument('--geometry', action='store_true',
                   help='with --sample_every_epochs: add the symmetry-aware RMSD of the recovered samples to the epoch scores')
    p.add_argument('--clashes', action='store_true',
                   help='with --sample_every_epochs, pocket models: add the steric clashes of the sampled linkers with the '
                        'pocket atoms to the epoch scores')
    p.add_argument('--shape', action='store_true',
                   help='with --sample_every_epochs: add the gridded shape overlap of every sample with its true molecule to '
                        'the epoch scores')
    p.add_argument('--rings', action='store_true',
                   help='with --sample_every_epochs: add the ring scores of the samples (ring count of the linker, small rings, '
                        'macrocycles) to the epoch scores')
    p.add_argument('--aromatic', action='store_true',
                   help='with --sample_every_epochs: perceive aromatic rings from the geometry (a rule of this project, not '
                        'RDKit\'s or OpenBabel\'s) and add aromatic_rings_n, ring_filter and valence_validity_geometric to the '
                        'epoch scores')
    p.add_argument('--diversity', action='store_true',
                   help='with --sample_every_epochs: add internal_diversity(_linker) and similarity_to_true(_linker) of the '
                        'samples to the epoch scores (Tanimoto on this project\'s circular fingerprint, not RDKit\'s Morgan)')
    p.add_argument('--pharmacophore', action='store_true',
                   help='with --sample_every_epochs: add the feature-map score of every sample\'s pharmacophore features '
                        'against its true molecule\'s to the epoch scores (feature_similarity(_linker); with --shape also '
                        'sc_similarity; this project\'s features after RDKit\'s BaseFeatures.fdef, not RDKit\'s numbers)')
    p.add_argument('--interactions', action='store_true',
                   help='with --sample_every_epochs, pocket models: add the contact scores of the sampled linkers with the '
                        'pocket atoms to the epoch scores (the intermolecular terms of Trott & Olson under this project\'s '
                        'heavy-atom typing, not AutoDock Vina\'s numbers)')
    p.add_argument('--pose_checks', action='store_true',
                   help='with --sample_every_epochs: check the internal geometry of every sample and of its true molecule - bond '
                        'lengths, bond angles, clashes between atoms four or more bonds apart, on the geometric bond orders (a '
                        'rule of this project after the idea of PoseBusters\' intramolecular checks, NOT PoseBusters\' numbers) - '
                        'and add pose_valid, its parts and their _linker variants to the epoch scores')
    a = p.parse_args(argv)
    cfg = dict(DEFAULTS)
    if a.config is not None:
        import yaml
        cfg.update({k: v for k, v in (yaml.safe_load(a.config) or {}).items() if k in DEFAULTS})
    for k in ('n_epochs', 'batch_size', 'lr', 'seed'):
        if getattr(a, k) is not None:
            cfg[k] = getattr(a, k)
    torch.manual_seed(int(cfg['seed']))
    device = torch.device(a.device)
    start_step = start_epoch = 0
    if a.resume:
        ckpt = torch.load(a.resume, map_location='cpu', weights_only=False)
        model = DDPM(**ckpt['hyper_parameters'])
        model.load_state_dict(ckpt['state_dict'])
        model.data_path = a.data
        start_step, start_epoch = int(ckpt.get('global_step', 0)), int(ckpt.get('epoch', 0))
    else:
        ckpt = None
        model = build_model(cfg, a.data, str(device))
    model = model.to(device)
    model.torch_device = device
    model.setup('fit')
    opt = model.configure_optimizers()
    if ckpt is not None and ckpt.get('optimizer_states'):
        opt.load_state_dict(ckpt['optimizer_states'][0])
    os.makedirs(a.checkpoints, exist_ok=True)
    path = os.path.join(a.checkpoints, 'last.ckpt')
    best_path = os.path.join(a.checkpoints, 'best.ckpt')
    best = float(ckpt.get('best_validity_and_connectivity', float('-inf'))) if ckpt is not None else float('-inf')
    if a.sample_every_epochs:
        model.test_epochs = a.sample_every_epochs
    model.geometry_metrics = bool(a.geometry)
    model.clash_metrics = bool(a.clashes)
    model.interaction_metrics = bool(a.interactions)
    model.shape_metrics = bool(a.shape)
    model.ring_metrics = bool(a.rings)
    model.aromatic_metrics = bool(a.aromatic)
    model.diversity_metrics = bool(a.diversity)
    model.pharmacophore_metrics = bool(a.pharmacophore)
    model.pose_metrics = bool(a.pose_checks)
    kept = lambda: {'best_validity_and_connectivity': best} if a.sample_every_epochs else {}   # noqa: E731
    step, epoch = start_step, start_epoch
    n_epochs = int(cfg['n_epochs'])
    done = False
    while not done and epoch < n_epochs:
        model.train()
        for data in model.train_dataloader():
            data = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in data.items()}
            out = model.training_step(data, step)
            opt.zero_grad(set_to_none=True)
            out['loss'].backward()
            opt.step()
            step += 1
            print(json.dumps({'step': step, 'epoch': epoch, 'loss': float(out['loss'])}), flush=True)
            if a.val_every and step % a.val_every == 0:
                if not a.no_validation:
                    print(json.dumps({'step': step, 'val': validate(model)}), flush=True)
                save(model, opt, path, step, epoch, **kept())
            if a.max_steps is not None and step >= a.max_steps:
                done = True
                break
        else:
            if a.sample_every_epochs:
                model.eval()
                model.current_epoch = epoch
                scores = model.validation_epoch_end([model.validation_step(data) for data in model.val_dataloader()])
                print(json.dumps({'step': step, 'epoch': epoch, 'val_epoch': scores}), flush=True)
                improved = BEST_KEY in scores and scores[BEST_KEY] > best
                if improved:
                    best = scores[BEST_KEY]
                save(model, opt, path, step, epoch + 1, **kept())
                if improved:
                    shutil.copyfile(path, best_path + '.tmp')
                    os.replace(best_path + '.tmp', best_path)
            epoch += 1
    if not a.no_validation:
        print(json.dumps({'step': step, 'val': validate(model)}), flush=True)
    save(model, opt, path, step, epoch, **kept())
    print(json.dumps({'checkpoint': path, 'step': step}), flush=True)
    return path


if __name__ == '__main__':
    main()
