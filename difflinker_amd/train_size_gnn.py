"""Train the linker-size predictor on the GPU: a plain loop in place of the reference's ``train_size_gnn.py`` (which drives
PyTorch Lightning's ``Trainer``; Lightning is not needed here).

    python -m difflinker_amd.train_size_gnn --data DIR --train_data_prefix zinc_final_train --val_data_prefix zinc_final_val
                                            --checkpoints CKPT_DIR [--n_layers 3] [--normalization batch_norm]
                                            [--batch_size 64] [--lr 1e-3] [--loss_weights]
                                            [--max_steps K | --n_epochs E] [--val_every V] [--resume CKPT] [--seed S]

As in ``train_size_gnn.py:45-60``: a prefix containing ``geom`` selects the GEOM atom types and size tables, any other the
ZINC ones.  ``--loss_weights`` uses the balanced class weights ``N_train / (C * n_c)`` counted on the training set.  Each
step: ``training_step`` in ``.train()`` mode on a shuffled batch, ``backward`` (HIP), ``AdamW.step``
(``configure_optimizers``).  Validation runs in ``.eval()`` mode and prints the mean ``loss/val`` and ``accuracy/val``
(``validation_epoch_end``).  ``CKPT_DIR/last.ckpt`` is written in Lightning's format (``hyper_parameters``, ``state_dict``,
plus ``optimizer_states``, ``global_step`` and ``epoch`` for ``--resume``); ``SizeClassifier.load_from_checkpoint`` and
``generate --linker_size CKPT`` read it.  Only ``--task classification`` and ``--hidden_nf 128`` are supported.
"""
import argparse
import json
import os

import torch

from . import const
from .linker_size import SizeClassifier, balanced_loss_weights


def class_counts(model, dataset):
    """Number of training molecules per class (true linker size -> class as ``get_true_labels`` maps it)."""
    counts = [0] * len(model.linker_id2size)
    for item in dataset:
        counts[int(model.get_true_labels(item['linker_mask'].reshape(1, -1))[0])] += 1
    return counts


def build_model(a, device):
    is_geom = 'geom' in a.train_data_prefix
    if is_geom:
        in_node_nf, id2size, size2id = const.GEOM_NUMBER_OF_ATOM_TYPES, const.GEOM_TRAIN_LINKER_ID2SIZE, const.GEOM_TRAIN_LINKER_SIZE2ID
    else:
        in_node_nf, id2size, size2id = const.NUMBER_OF_ATOM_TYPES, const.ZINC_TRAIN_LINKER_ID2SIZE, const.ZINC_TRAIN_LINKER_SIZE2ID
    return SizeClassifier(data_path=a.data, train_data_prefix=a.train_data_prefix, val_data_prefix=a.val_data_prefix,
                          in_node_nf=in_node_nf, hidden_nf=a.hidden_nf, out_node_nf=len(id2size), n_layers=a.n_layers,
                          batch_size=a.batch_size, lr=a.lr, normalization=a.normalization, torch_device=str(device),
                          linker_size2id=dict(size2id), linker_id2size=list(id2size))


def to_device(data, device):
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in data.items()}
    if 'edges' in out:
        out['edges'] = [e.to(device) for e in out['edges']]
    return out


def validate(model, device):
    """Mean ``loss`` over the validation batches and ``accuracy`` (validation_epoch_end), in eval mode."""
    was_training = model.training
    model.eval()
    losses, correct, total = [], 0, 0
    with torch.no_grad():
        for data in model.val_dataloader():
            data = to_device(data, device)
            output, loss = model.forward(data)
            losses.append({'loss': float(loss)})
            true = model.get_true_labels(data['linker_mask'])
            correct += int((output.argmax(dim=-1) == true).sum())
            total += len(true)
    model.train(was_training)
    if not losses:
        return {}
    return {'loss/val': float(SizeClassifier.aggregate_metric(losses, 'loss')), 'accuracy/val': correct / total}


def save(model, opt, path, step, epoch):
    ckpt = model.checkpoint_dict()
    ckpt.update(optimizer_states=[opt.state_dict()], global_step=step, epoch=epoch)
    tmp = path + '.tmp'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def parser():
    p = argparse.ArgumentParser(description='Linker-size predictor training on MI355X (HIP forward and backward)')
    p.add_argument('--data', default='datasets')
    p.add_argument('--train_data_prefix', default='zinc_final_train')
    p.add_argument('--val_data_prefix', default='zinc_final_val')
    p.add_argument('--hidden_nf', type=int, default=128)
    p.add_argument('--n_layers', type=int, default=3)
    p.add_argument('--normalization', default=None)
    p.add_argument('--batch_size', type=int, default=64)
    p.add_argument('--lr', type=float, default=1e-3)
    p.add_argument('--task', default='classification')
    p.add_argument('--loss_weights', action='store_true', default=False)
    p.add_argument('--checkpoints', default='checkpoints')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--max_steps', type=int, default=None, help='stop after this many optimiser steps')
    p.add_argument('--n_epochs', type=int, default=1000)
    p.add_argument('--val_every', type=int, default=0, help='validate and checkpoint every V steps (0: at the end only)')
    p.add_argument('--resume', default=None, help='checkpoint of this loop to continue from')
    p.add_argument('--seed', type=int, default=0)
    return p


def main(argv=None):
    a = parser().parse_args(argv)
    if a.task != 'classification':
        raise NotImplementedError(f'--task {a.task}: only the classifier (SizeClassifier) is trained here')
    torch.manual_seed(a.seed)
    device = torch.device(a.device)
    start_step = start_epoch = 0
    ckpt = None
    if a.resume:
        ckpt = torch.load(a.resume, map_location='cpu', weights_only=False)
        model = SizeClassifier(**ckpt['hyper_parameters'])
        model.load_state_dict(ckpt['state_dict'])
        model.data_path = a.data
        start_step, start_epoch = int(ckpt.get('global_step', 0)), int(ckpt.get('epoch', 0))
    else:
        model = build_model(a, device)
    model = model.to(device)
    model.torch_device = str(device)
    model.setup('fit')
    if a.loss_weights and ckpt is None:
        model.loss_weights = balanced_loss_weights(class_counts(model, model.train_dataset))
        model.hparams_dict['loss_weights'] = model.loss_weights
    opt = model.configure_optimizers()
    if ckpt is not None and ckpt.get('optimizer_states'):
        opt.load_state_dict(ckpt['optimizer_states'][0])
    os.makedirs(a.checkpoints, exist_ok=True)
    path = os.path.join(a.checkpoints, 'last.ckpt')
    step, epoch = start_step, start_epoch
    done = False
    while not done and epoch < a.n_epochs:
        model.train()
        for data in model.train_dataloader():
            out = model.training_step(to_device(data, device), step)
            opt.zero_grad(set_to_none=True)
            out['loss'].backward()
            opt.step()
            step += 1
            print(json.dumps({'step': step, 'epoch': epoch, 'loss': float(out['loss'])}), flush=True)
            if a.val_every and step % a.val_every == 0:
                print(json.dumps({'step': step, 'val': validate(model, device)}), flush=True)
                save(model, opt, path, step, epoch)
            if a.max_steps is not None and step >= a.max_steps:
                done = True
                break
        else:
            epoch += 1
    print(json.dumps({'step': step, 'val': validate(model, device)}), flush=True)
    save(model, opt, path, step, epoch)
    print(json.dumps({'checkpoint': path, 'step': step}), flush=True)
    return path


if __name__ == '__main__':
    main()
