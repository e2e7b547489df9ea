"""Generate ``edm_grad.npz`` from the UNMODIFIED reference: the gradient of ``EDM.forward``'s ``l2_loss`` (and, for one
case, of ``vlb_loss``) with respect to every ``Dynamics`` parameter, as ``loss.backward()`` gives it on the CPU.

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad.py

Every case stores its inputs, the draws of the reference's forward (replayed as ``make_golden_loss.py`` does), its 7
outputs and one gradient per ``state_dict`` key (``<tag>.grad.<key>``): whole for tensors of at most ``KEEP`` entries, else
``KEEP`` entries at fixed positions (``<tag>.idx.<key>``, flat indices) to keep the file small.  The weights are not stored: they are regenerated
from the seeds by ``trained_like_state_dict(seeded_state_dict(...))``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, ragged_fc_batch, save      # noqa: E402,F401  (sets sys.path: repository, tests/, reference)
from make_golden_loss import NORM_VALUES, draws, loss_inputs, pick_seed    # noqa: E402

from src.egnn import Dynamics                             # noqa: E402
from src.edm import EDM, InpaintingEDM                    # noqa: E402

from helpers import seeded_state_dict, trained_like_state_dict   # noqa: E402

# (tag, EDM class, nf, ctx, n_layers, T, weight seed, loss)
CASES = [
    ('fc', EDM, 9, 1, 2, 10, 81, 'l2'),
    ('t0', EDM, 9, 1, 1, 10, 82, 'l2'),
    ('inpaint', InpaintingEDM, 8, 1, 2, 10, 83, 'l2'),
    ('ragged_vlb', EDM, 8, 1, 1, 10, 84, 'vlb'),
]


KEEP = 512


def sample(key, g):
    flat = g.reshape(-1)
    if flat.size <= KEEP:
        return None, flat
    idx = np.sort(np.random.default_rng(len(key) * 7919 + flat.size)
                  .choice(flat.size, KEEP, replace=False)).astype(np.int32)
    return idx, flat[idx]


def batch_of(tag, nf):
    if tag == 'fc':
        return ragged_fc_batch([14, 9, 12, 5, 11, 8], [4, 3, 5, 2, 4, 3], nf, seed=91)
    if tag == 't0':
        return ragged_fc_batch([10, 7, 12], [3, 2, 4], nf, seed=92)
    if tag == 'inpaint':
        return ragged_fc_batch([12, 7, 10, 9], [4, 2, 3, 3], nf, seed=93)
    return ragged_fc_batch([21, 6, 15, 9, 30], [6, 2, 4, 3, 8], nf, seed=94)


def edm_grad():
    out = {}
    for tag, edm_cls, nf, ctx, L, T, wseed, loss in CASES:
        inpainting = edm_cls is InpaintingEDM
        inp = loss_inputs(batch_of(tag, nf), inpainting=inpainting)
        B, N = inp['x'].shape[:2]
        dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, device='cpu', n_layers=L,
                       attention=False, tanh=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
                       normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
                       normalization='batch_norm', centering=inpainting, graph_type='FC')
        sd = trained_like_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, wseed, coord_gain=0.02), wseed)
        dyn.load_state_dict(sd, strict=True)
        edm = edm_cls(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=T, noise_schedule='polynomial_2',
                      noise_precision=1e-5, loss_type=loss, norm_values=NORM_VALUES)
        seed = pick_seed('t0' if tag == 't0' else 'fc', B, T)
        t_int, noise_x, noise_h = draws(seed, B, N, nf, T)
        torch.manual_seed(seed)
        res = edm.forward(x=inp['x'], h=inp['h'], node_mask=inp['node_mask'], fragment_mask=inp['fragment_mask'],
                          linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'], context=inp['context'])
        delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = res
        target = l2_loss if loss == 'l2' else kl_prior + loss_term_t + loss_term_0 - delta_log_px
        dyn.zero_grad()
        target.backward()
        grads = {k: p.grad.detach().numpy().copy() for k, p in dyn.named_parameters()}
        print(tag, 'seed', seed, 't', t_int.flatten().tolist(), 'loss', float(target))
        out.update({f'{tag}.{k}': v for k, v in inp.items()})
        out.update({f'{tag}.t_int': t_int, f'{tag}.noise_x': noise_x, f'{tag}.noise_h': noise_h,
                    f'{tag}.outputs': np.array([float(v) for v in res], dtype=np.float32),
                    f'{tag}.params': np.array([nf, ctx, L, T, wseed, int(inpainting), int(loss == 'vlb')])})
        for k, v in grads.items():
            idx, vals = sample(k, v)
            out[f'{tag}.grad.{k}'] = vals
            if idx is not None:
                out[f'{tag}.idx.{k}'] = idx
    save('edm_grad', norm_values=np.array(NORM_VALUES, dtype=np.float32), **out)


if __name__ == '__main__':
    edm_grad()
