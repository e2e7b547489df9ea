"""Score a checkpoint on held-out data: the diffusion loss and the VLB terms of every batch (``DDPM.validation_step``,
reference ``src/lightning.py:228-247``) averaged over the batches the way ``DDPM.aggregate_metric`` (:478-480) does.

    python -m difflinker_amd.evaluate --checkpoint m.ckpt --data DIR --prefix geom_test [--batch_size 64]
                                      [--noise_source philox --seed S] [--device cuda]

prints one JSON object ``{metric: mean}``.  The data set is loaded through ``setup('val')`` with ``val_data_prefix``
overridden, as the reference's ``sample.py`` does.  One ``t`` and one noise draw per molecule, as in the reference:
``noise_source='torch'`` (default) draws them with ``torch.randint`` / ``torch.randn`` after ``torch.manual_seed(seed)``;
``'philox'`` draws them in the kernels from ``seed`` and the molecule's index in the data set, independent of the batch size.
"""
import argparse
import json

import torch

from .lightning import DDPM

METRICS = ('loss', 'delta_log_px', 'kl_prior', 'loss_term_t', 'loss_term_0', 'l2_loss', 'vlb_loss', 'noise_t', 'noise_0')


def evaluate(model, dataloader):
    """Per-metric means over the batches of ``dataloader`` of ``model.validation_step`` (``DDPM.aggregate_metric``).  With
    ``noise_source='philox'`` every batch draws from the same ``noise_seed`` at its molecules' running index in the data set,
    so the result does not depend on the batch size; ``noise_seed`` then advances by one."""
    edm = model.edm
    philox = edm.noise_source == 'philox'
    seed = int(edm.noise_seed)
    outputs = []
    offset = 0
    for data in dataloader:
        if philox:
            edm.noise_seed = seed
            outputs.append(model._metrics(data, mol_offset=offset))
        else:
            outputs.append(model.validation_step(data))
        offset += int(data['positions'].shape[0])
    if philox:
        edm.noise_seed = seed + 1
    return {m: float(DDPM.aggregate_metric(outputs, m)) for m in METRICS}


def main(argv=None):
    p = argparse.ArgumentParser(description='DiffLinker: diffusion loss and VLB of held-out data on MI355X')
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--data', required=True, help='directory of the preprocessed data set')
    p.add_argument('--prefix', required=True, help='data set prefix, e.g. geom_test or MOAD_test.full')
    p.add_argument('--batch_size', type=int, default=64)
    p.add_argument('--noise_source', choices=('torch', 'philox'), default='torch')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--device', default='cuda')
    a = p.parse_args(argv)
    device = torch.device(a.device)
    model = DDPM.load_from_checkpoint(a.checkpoint, map_location=device)
    model.val_data_prefix = a.prefix
    model.data_path = a.data
    model.batch_size = a.batch_size
    model = model.eval().to(device)
    model.torch_device = device
    model.setup(stage='val')
    model.edm.noise_source = a.noise_source
    if a.noise_source == 'philox':
        model.edm.noise_seed = a.seed
    else:
        torch.manual_seed(a.seed)
    result = evaluate(model, model.val_dataloader())
    print(json.dumps(result))
    return result


if __name__ == '__main__':
    main()
