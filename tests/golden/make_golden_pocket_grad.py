"""Generate ``pocket_grad.npz`` from the UNMODIFIED reference: the gradient of ``EDM.forward``'s ``l2_loss`` (one case) and
``vlb_loss`` (the other) with respect to every parameter of ``DynamicsWithPockets``, as ``loss.backward()`` gives it on the CPU.

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pocket_grad.py

Two ragged batches of three complexes (12 fragment, 3..8 linker, 40..70 pocket atoms), 2 layers: ``FC-10A-4A`` with the l2
loss and ``FC-4A`` with the VLB.  Every case stores its inputs, the draws of the reference's forward (replayed as
``make_golden_loss.py`` does), its 7 outputs and one gradient per ``state_dict`` key, sampled to at most 512 entries per
tensor as ``make_golden_grad.py`` does.  The weights are not stored: they are regenerated from the seeds by
``trained_like_state_dict(seeded_state_dict(...))``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, save                        # noqa: E402,F401  (sets sys.path: repository, tests/, reference)
from make_golden_grad import sample                       # noqa: E402
from make_golden_loss import NORM_VALUES, draws, loss_inputs, pick_seed    # noqa: E402

from src.egnn import DynamicsWithPockets                  # noqa: E402
from src.edm import EDM                                   # noqa: E402

from difflinker_amd import synthetic                      # noqa: E402
from difflinker_amd.datasets import collate               # noqa: E402
from helpers import seeded_state_dict, trained_like_state_dict   # noqa: E402

GRAPHS = {'FC-4A': 1, 'FC-10A-4A': 2}
# (tag, graph type, pocket atoms per complex, nf, ctx, n_layers, T, weight seed, data seed, loss)
CASES = [
    ('fc10_l2', 'FC-10A-4A', (70, 40, 55), 9, 2, 2, 10, 91, 95, 'l2'),
    ('fc4_vlb', 'FC-4A', (40, 62, 51), 9, 2, 2, 10, 92, 96, 'vlb'),
]


def ragged_pocket_batch(pockets, nf, seed):
    mols = []
    for k, n_pocket in enumerate(pockets):
        mols += synthetic.pocket_molecules(1, n_frag=12, n_pocket=n_pocket, linker=(3, 8), nf=nf, seed=seed + k)
    return collate(mols)


def pocket_grad():
    out = {}
    for tag, graph_type, pockets, nf, ctx, L, T, wseed, dseed, loss in CASES:
        inp = loss_inputs(ragged_pocket_batch(pockets, nf, dseed), pockets=True)
        B, N = inp['x'].shape[:2]
        dyn = DynamicsWithPockets(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, device='cpu', n_layers=L,
                                  attention=False, tanh=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
                                  normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
                                  normalization='batch_norm', centering=False, graph_type=graph_type)
        sd = trained_like_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, wseed, coord_gain=0.02), wseed)
        dyn.load_state_dict(sd, strict=True)
        edm = EDM(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=T, noise_schedule='polynomial_2', noise_precision=1e-5,
                  loss_type=loss, norm_values=NORM_VALUES)
        seed = pick_seed('fc', B, T)
        t_int, noise_x, noise_h = draws(seed, B, N, nf, T)
        torch.manual_seed(seed)
        res = edm.forward(x=inp['x'], h=inp['h'], node_mask=inp['node_mask'], fragment_mask=inp['fragment_mask'],
                          linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'], context=inp['context'])
        delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = res
        target = l2_loss if loss == 'l2' else kl_prior + loss_term_t + loss_term_0 - delta_log_px
        dyn.zero_grad()
        target.backward()
        grads = {k: p.grad.detach().numpy().copy() for k, p in dyn.named_parameters()}
        print(tag, 'N', N, 'seed', seed, 't', t_int.flatten().tolist(), 'loss', float(target))
        out.update({f'{tag}.{k}': v for k, v in inp.items()})
        out.update({f'{tag}.t_int': t_int, f'{tag}.noise_x': noise_x, f'{tag}.noise_h': noise_h,
                    f'{tag}.outputs': np.array([float(v) for v in res], dtype=np.float32),
                    f'{tag}.params': np.array([nf, ctx, L, T, wseed, GRAPHS[graph_type], int(loss == 'vlb')])})
        for k, v in grads.items():
            idx, vals = sample(k, v)
            out[f'{tag}.grad.{k}'] = vals
            if idx is not None:
                out[f'{tag}.idx.{k}'] = idx
    save('pocket_grad', norm_values=np.array(NORM_VALUES, dtype=np.float32), **out)


if __name__ == '__main__':
    pocket_grad()
