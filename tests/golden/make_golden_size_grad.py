"""Generate ``size_grad.npz`` from the UNMODIFIED reference: the linker-size predictor in TRAINING mode (BatchNorm over all
B*N rows) and the gradient of its cross-entropy loss with respect to every ``SizeGNN`` parameter, as ``loss.backward()``
gives it on the CPU.

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_size_grad.py

``SizeClassifier`` needs pytorch_lightning, which this image lacks, so its ten lines of ``forward`` are restated around the
reference ``SizeGNN`` and ``coord2diff``, as ``make_golden.py::size_gnn`` does.  Per case: the inputs, the train-mode logits,
the loss, ``running_mean`` / ``running_var`` of every BatchNorm after the forward, and one gradient per parameter
(``<tag>.grad.<key>``, whole up to ``KEEP`` entries, else ``KEEP`` entries at the flat indices ``<tag>.idx.<key>``).  The
weights are not stored: ``helpers.seeded_size_state_dict`` regenerates them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save                                  # noqa: E402  (sets sys.path: repository, tests/, reference)
from make_golden_grad import sample                           # noqa: E402

from src.linker_size import SizeGNN                           # noqa: E402
from src.egnn import coord2diff                               # noqa: E402

from helpers import seeded_size_state_dict                    # noqa: E402
from size_train_ref import size_batch, true_labels            # noqa: E402

IN_NF, OUT_NF = 8, 10
# (tag, n_layers, normalization, sizes, linkers, loss weights, weight seed)
CASES = [
    ('bn2', 2, 'batch_norm', [14, 9, 12, 5, 11], [4, 3, 5, 0, 2], True, 601),
    ('plain3', 3, None, [10, 16, 7], [3, 5, 2], False, 602),
    ('bn1_full', 1, 'batch_norm', [9, 9, 9], [0, 0, 0], False, 603),
]


def loss_weights():
    return torch.linspace(0.5, 2.0, OUT_NF)


def size_grad():
    out = {}
    for tag, L, norm, sizes, linkers, weighted, wseed in CASES:
        data = size_batch(sizes, linkers, IN_NF, seed=wseed)
        gnn = SizeGNN(in_node_nf=IN_NF, hidden_nf=128, out_node_nf=OUT_NF, n_layers=L, normalization=norm)
        gnn.load_state_dict(seeded_size_state_dict(IN_NF, 128, OUT_NF, L, seed=wseed, batch_norm=norm is not None),
                            strict=True)
        gnn.train()
        h, x = data['one_hot'], data['positions']
        fragment_mask, edge_mask, edges = data['fragment_mask'], data['edge_mask'], data['edges']
        x = x * fragment_mask
        h = h * fragment_mask
        bs, n_nodes = x.shape[0], x.shape[1]
        fm = fragment_mask.view(bs * n_nodes, 1)
        distances, _ = coord2diff(x.view(bs * n_nodes, -1), edges)
        distance_edge_mask = (edge_mask.bool() & (distances < 6)).long()
        output = gnn.forward(h.view(bs * n_nodes, -1), edges, distances, fm, distance_edge_mask)
        output = output.view(bs, n_nodes, -1).mean(1)
        weight = loss_weights() if weighted else None
        loss = torch.nn.functional.cross_entropy(output, true_labels(data['linker_mask']), weight=weight)
        gnn.zero_grad()
        loss.backward()
        print(tag, 'B', bs, 'N', n_nodes, 'loss', float(loss))
        out.update({f'{tag}.one_hot': data['one_hot'], f'{tag}.positions': data['positions'],
                    f'{tag}.fragment_mask': data['fragment_mask'], f'{tag}.linker_mask': data['linker_mask'],
                    f'{tag}.edge_mask': data['edge_mask'], f'{tag}.logits': output.detach(),
                    f'{tag}.loss': np.float32(float(loss)),
                    f'{tag}.params': np.array([L, int(norm is not None), int(weighted), wseed])})
        for k, v in gnn.state_dict().items():
            if k.endswith('running_mean') or k.endswith('running_var'):
                out[f'{tag}.stat.{k}'] = v
        for k, p in gnn.named_parameters():
            idx, vals = sample(k, p.grad.detach().numpy().copy())
            out[f'{tag}.grad.{k}'] = vals
            if idx is not None:
                out[f'{tag}.idx.{k}'] = idx
    save('size_grad', in_nf=IN_NF, out_nf=OUT_NF, loss_weights=loss_weights(), **out)


if __name__ == '__main__':
    size_grad()
