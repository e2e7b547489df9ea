"""Training on the GPU: the HIP backward of the fully-connected denoiser (csrc/egnn_backward.hip) against fp64 autograd of
the oracle, the loss gradient (``EDM.training_forward``) against an fp64 restatement of the reference's l2 loss, bitwise
determinism, the values of ``training_forward`` against ``EDM.forward``, re-packing after ``optimizer.step()``, a short
overfit and the ``python -m difflinker_amd.train`` loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_cases as TC
from helpers import ragged_fc_molecules, rel_l2, seeded_state_dict, trained_like_state_dict
from oracle import egnn_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured (MI355X) over the cases of tests/train_cases.py: at most 2.5e-7 over all ('wrap_257'), 7.1e-7 per tensor ('sub4_trained');
# fp32 eager autograd of the oracle: 5.6e-7 / 2.7e-6; the reference fixtures below: 5.5e-7 / 1.7e-6.  (With every sum of the kernel
# one fp32 chain the same cases gave 1.4e-6 / 4.6e-6, both 'wrap_257'.)
BAR_ALL, BAR_TENSOR = 2e-6, 1e-5
FP32_CLASS = TC.FP32_CLASS              # and within 2x the error of fp32 eager autograd against the same fp64 gradient
assert (BAR_ALL, BAR_TENSOR) == (TC.BAR_ALL, TC.BAR_TENSOR)


def batch(sizes, linkers, nf, ctx, seed):
    from difflinker_amd.datasets import collate
    mols = ragged_fc_molecules(sizes, linkers, nf, seed)
    b = collate(mols)
    g = torch.Generator().manual_seed(seed + 1)
    B, N = b['positions'].shape[:2]
    context = torch.cat([b['fragment_mask']] + [torch.rand(B, N, 1, generator=g) for _ in range(ctx - 1)], -1) * b['atom_mask']
    return b, context


def make_dyn(nf, ctx, L, S, wseed, trained=False, centering=False):
    from difflinker_amd import Dynamics
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, inv_sublayers=S,
                   norm_constant=1e-6, normalization_factor=100, centering=centering)
    sd = seeded_state_dict(nf + ctx + 1, 128, L, wseed, coord_gain=0.02, inv_sublayers=S)
    if trained:
        sd = trained_like_state_dict(sd, wseed)
    dyn.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return dyn.to(DEV)


def oracle_grads(dyn, t, z, nm, lm, em, ctx, G):
    cfg = egnn_oracle.EGNNConfig(in_node_nf=dyn.in_node_nf, context_node_nf=dyn.context_node_nf, n_layers=dyn.n_layers,
                                 inv_sublayers=dyn.inv_sublayers, norm_constant=dyn.norm_constant,
                                 normalization_factor=dyn.normalization_factor, centering=dyn.centering)
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in dyn.state_dict().items()}
    d = lambda v: None if v is None else v.detach().cpu().double()          # noqa: E731
    out = egnn_oracle.dynamics_forward(p, cfg, d(t), d(z), d(nm), d(lm), d(em), d(ctx))
    (out * d(G)).sum().backward()
    return {k: v.grad for k, v in p.items()}


def hip_grads(dyn, t, z, nm, lm, em, ctx, G):
    g = lambda v: None if v is None else v.to(DEV)                            # noqa: E731
    grads = dyn.parameter_grad(g(t), g(z), g(nm), g(lm), g(em), g(ctx), g(G))
    return {k: v.cpu() for k, v in zip([n for n, _ in dyn.named_parameters()], grads)}


def compare(hip, ref):
    keys = list(ref)
    a = torch.cat([hip[k].double().reshape(-1) for k in keys])
    b = torch.cat([ref[k].reshape(-1) for k in keys])
    worst = max(rel_l2(hip[k], ref[k]) for k in keys if ref[k].norm() > 0)
    return rel_l2(a, b), worst


# sizes, linkers, nf, ctx, L, S, per-molecule t, centering, trained-like of the four first cases (tests/train_cases.py holds the table)
CASES = {k: tuple(TC.spec(k)[f] for f in ('sizes', 'linkers', 'nf', 'ctx', 'L', 'S', 'per_mol_t', 'centering', 'trained'))
         for k in TC.EXISTING}


@pytest.mark.parametrize('case', list(TC.CASES))
def test_parameter_grad_matches_fp64_oracle(case):
    """Every case of tests/train_cases.py against fp64 autograd of the oracle: under the bars, within ``FP32_CLASS`` times the
    error of fp32 eager autograd of the same oracle, every output finite, and exactly zero where the fp64 gradient is (the
    kernel multiplies by ``lm = 0`` or a zero ``coord_diff`` there: nothing to round)."""
    inp = TC.build(case)
    if case in TC.REFUSED:                               # outside the kernels' scope: refused by name, before any launch
        with pytest.raises(NotImplementedError, match=TC.REFUSED[case]):
            TC.hip_grads(TC.make_dyn(inp, DEV), DEV, *inp.args())
        return
    ref, f32 = TC.reference(case)
    hip = TC.hip_grads(TC.make_dyn(inp, DEV), DEV, *inp.args())
    assert set(hip) == set(ref)
    for k, v in hip.items():
        assert bool(torch.isfinite(v).all()), k
    for k in TC.zero_tensors(ref):
        assert not bool(hip[k].any()), f'{k}: the fp64 gradient is exactly zero'
    total, worst = compare(hip, ref)
    total32, worst32 = compare(f32, ref)
    print(f'{case}: rel-L2 all {total:.2e}, worst tensor {worst:.2e}; fp32 eager autograd {total32:.2e}, {worst32:.2e}')
    assert total <= BAR_ALL and worst <= BAR_TENSOR, (total, worst)
    assert total <= FP32_CLASS * total32 and worst <= FP32_CLASS * worst32, (total, total32, worst, worst32)


def test_edge_mask_values_are_used_as_given():
    """collate's int8 mask is 0 / -1 / -2; a 0/1 mask gives another gradient, the backward follows the forward's factor."""
    b, context = batch([9, 13], [3, 4], 8, 1, seed=2)
    assert set(torch.unique(b['edge_mask']).tolist()) == {0, -1, -2}
    B, N = b['positions'].shape[:2]
    z = torch.cat([b['positions'], b['one_hot']], -1)
    G = torch.randn(B, N, 11, generator=torch.Generator().manual_seed(1))
    t = torch.full((B, 1), 0.5)
    dyn = make_dyn(8, 1, 1, 2, wseed=5)
    args = [t, z, b['atom_mask'], b['linker_mask'], b['edge_mask'], context, G]
    hip = hip_grads(dyn, *args)
    total, _ = compare(hip, oracle_grads(dyn, *args))
    assert total <= BAR_ALL
    args[4] = (b['edge_mask'] != 0).to(torch.int8)
    other = hip_grads(dyn, *args)
    assert compare(other, hip)[0] > 1e-3


def test_parameter_grad_bitwise_repeatable():
    b, context = batch([14, 30, 8, 21], [4, 9, 2, 6], 8, 2, seed=4)
    B, N = b['positions'].shape[:2]
    z = torch.cat([b['positions'], b['one_hot']], -1)
    G = torch.randn(B, N, 11, generator=torch.Generator().manual_seed(9))
    dyn = make_dyn(8, 2, 2, 2, wseed=8)
    args = (torch.rand(B, 1), z, b['atom_mask'], b['linker_mask'], b['edge_mask'], context, G)
    a, c = hip_grads(dyn, *args), hip_grads(dyn, *args)
    assert all(torch.equal(a[k], c[k]) for k in a)


def make_edm(nf, ctx, L, S, wseed, inpainting=False, loss_type='l2'):
    from difflinker_amd import EDM, InpaintingEDM
    dyn = make_dyn(nf, ctx, L, S, wseed, centering=inpainting)
    edm = (InpaintingEDM if inpainting else EDM)(dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
                                                 noise_precision=1e-5, loss_type=loss_type, norm_values=[1, 4, 10])
    return edm.to(DEV)


def edm_inputs(sizes, linkers, nf, seed):
    b, _ = batch(sizes, linkers, nf, 1, seed)
    g = {k: b[k].to(DEV) for k in ('positions', 'one_hot', 'atom_mask', 'fragment_mask', 'linker_mask', 'edge_mask')}
    return g, g['fragment_mask']


def edm_args(g, ctx):
    return (g['positions'], g['one_hot'], g['atom_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], ctx)


@pytest.mark.parametrize('inpainting', [False, True])
def test_training_forward_values_equal_forward(inpainting):
    edm = make_edm(8, 1, 2, 2, 21, inpainting=inpainting)
    g, ctx = edm_inputs([10, 17, 6], [3, 5, 2], 8, seed=1)
    B, N = g['positions'].shape[:2]
    t_int = torch.tensor([0, 250, 500], device=DEV)
    noise = (torch.randn(B, N, 3, device=DEV), torch.randn(B, N, 8, device=DEV))
    with torch.no_grad():
        want = edm(*edm_args(g, ctx), t_int=t_int, noise=noise)
    got = edm.training_forward(*edm_args(g, ctx), t_int=t_int, noise=noise)
    for a, c in zip(got, want):
        assert type(a) is type(c)
        if torch.is_tensor(a):
            assert torch.equal(a.detach(), c)
    for k in (2, 3, 4, 5, 6):
        assert got[k].requires_grad
    edm.noise_source = 'philox'
    edm.noise_seed = 77
    with torch.no_grad():
        want = edm(*edm_args(g, ctx))
    edm.noise_seed = 77
    got = edm.training_forward(*edm_args(g, ctx))
    for a, c in zip(got, want):
        assert torch.equal(torch.as_tensor(a).detach().cpu(), torch.as_tensor(c).cpu())


def fp64_l2_grads(edm, g, ctx, t_int, noise):
    """Gradient of the reference's l2 loss (edm.py:41-88: z_t, one denoiser call, the masked squared error over
    (3 + nf) n_linker, batch mean) restated in fp64 on the oracle, for an EDM of one context channel and 2 sublayers."""
    nf = edm.in_node_nf
    B = g['positions'].shape[0]
    d = lambda v: v.detach().cpu().double()                                   # noqa: E731
    x, h, nm, fm, lm = d(g['positions']), d(g['one_hot']) / 4, d(g['atom_mask']), d(g['fragment_mask']), d(g['linker_mask'])
    xh = torch.cat([x, h], -1)
    table = edm.gamma.gamma.detach().cpu().double()
    t = t_int.cpu().double() / edm.T
    gam = table[torch.round(t * 500).long()].view(B, 1, 1)
    alpha, sigma = torch.sqrt(torch.sigmoid(-gam)), torch.sqrt(torch.sigmoid(gam))
    eps = torch.cat([d(noise[0]), d(noise[1])], -1) * lm
    z = xh * fm + (alpha * xh + sigma * eps) * lm
    dyn = edm.dynamics
    cfg = egnn_oracle.EGNNConfig(in_node_nf=nf, context_node_nf=1, n_layers=dyn.n_layers, inv_sublayers=2, norm_constant=1e-6,
                                 normalization_factor=100)
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in dyn.state_dict().items()}
    eps_hat = egnn_oracle.dynamics_forward(p, cfg, t.view(B, 1), z, nm, lm, d(g['edge_mask']), d(ctx)) * lm
    err = ((eps - eps_hat) ** 2).sum((1, 2))
    l2 = (err / ((3 + nf) * lm.sum((1, 2)))).mean()
    l2.backward()
    return {k: v.grad for k, v in p.items()}


def test_l2_loss_gradient_matches_fp64():
    """d l2_loss / d theta of ``EDM.training_forward`` against the reference's l2 loss (edm.py:41-88) restated in fp64."""
    nf = 8
    edm = make_edm(nf, 1, 1, 2, 33)
    g, ctx = edm_inputs([11, 16, 9, 13], [4, 5, 3, 4], nf, seed=6)
    B, N = g['positions'].shape[:2]
    t_int = torch.tensor([0, 120, 260, 499], device=DEV)
    gen = torch.Generator().manual_seed(2)
    noise = (torch.randn(B, N, 3, generator=gen).to(DEV), torch.randn(B, N, nf, generator=gen).to(DEV))
    edm.dynamics.zero_grad()
    out = edm.training_forward(*edm_args(g, ctx), t_int=t_int, noise=noise)
    out[4].backward()
    hip = {k: p.grad.cpu() for k, p in edm.dynamics.named_parameters()}
    ref = fp64_l2_grads(edm, g, ctx, t_int, noise)
    total, worst = compare(hip, ref)
    print(f'l2 loss gradient: rel-L2 all {total:.2e}, worst tensor {worst:.2e}')
    assert total <= BAR_ALL and worst <= BAR_TENSOR


def test_forward_after_optimizer_step_uses_new_weights():
    from difflinker_amd import Dynamics
    edm = make_edm(8, 1, 1, 2, 12)
    g, ctx = edm_inputs([10, 14], [3, 4], 8, seed=3)
    B, N = g['positions'].shape[:2]
    opt = torch.optim.AdamW(edm.parameters(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    z = torch.cat([g['positions'], g['one_hot']], -1)
    t = torch.full((B, 1), 0.3, device=DEV)
    fwd = lambda dyn: dyn.forward(t, z, g['atom_mask'], g['linker_mask'], g['edge_mask'], ctx)   # noqa: E731
    with torch.no_grad():
        before = fwd(edm.dynamics)
    out = edm.training_forward(*edm_args(g, ctx), t_int=torch.tensor([100, 300], device=DEV),
                               noise=(torch.randn(B, N, 3, device=DEV), torch.randn(B, N, 8, device=DEV)))
    opt.zero_grad()
    out[4].backward()
    opt.step()
    with torch.no_grad():
        after = fwd(edm.dynamics)
    fresh = Dynamics(n_dims=3, in_node_nf=8, context_node_nf=1, hidden_nf=128, n_layers=1, inv_sublayers=2,
                     norm_constant=1e-6, normalization_factor=100)
    fresh.load_state_dict(edm.dynamics.state_dict())
    with torch.no_grad():
        want = fwd(fresh.to(DEV))
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_adamw_step_matches_oracle_gradient_and_overfits():
    from difflinker_amd import utils
    nf = 8
    edm = make_edm(nf, 1, 1, 2, 17)
    g, ctx = edm_inputs([12, 9, 15], [4, 3, 5], nf, seed=8)
    B, N = g['positions'].shape[:2]
    g['positions'] = utils.remove_partial_mean_with_mask(g['positions'], g['atom_mask'], g['fragment_mask'])
    t_int = torch.tensor([40, 200, 350], device=DEV)
    gen = torch.Generator().manual_seed(4)
    noise = (torch.randn(B, N, 3, generator=gen).to(DEV), torch.randn(B, N, nf, generator=gen).to(DEV))
    # one step against AdamW on the fp64 oracle's gradient (the same first-step update)
    params = dict(edm.dynamics.named_parameters())
    start = {k: v.detach().clone() for k, v in params.items()}
    opt = torch.optim.AdamW(edm.parameters(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    out = edm.training_forward(*edm_args(g, ctx), t_int=t_int, noise=noise)
    opt.zero_grad()
    out[4].backward()
    grads = {k: v.grad.detach().clone() for k, v in params.items()}
    ref = fp64_l2_grads(edm, g, ctx, t_int, noise)           # at the weights before the step
    opt.step()
    shadow = {k: torch.nn.Parameter(v.detach().cpu().double()) for k, v in start.items()}
    sopt = torch.optim.AdamW(shadow.values(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    for k, v in shadow.items():
        v.grad = ref[k]
    sopt.step()
    step = torch.cat([(params[k].detach().cpu().double() - start[k].cpu().double()).reshape(-1) for k in params])
    want = torch.cat([(shadow[k].detach() - start[k].cpu().double()).reshape(-1) for k in params])
    err = rel_l2(step, want)
    print(f'AdamW step vs fp64-oracle gradient: rel-L2 {err:.2e}')
    assert err <= BAR_TENSOR
    assert rel_l2(torch.cat([grads[k].cpu().reshape(-1) for k in params]), torch.cat([ref[k].reshape(-1) for k in params])) <= BAR_ALL
    losses = [float(out[4].detach())]
    for _ in range(49):
        out = edm.training_forward(*edm_args(g, ctx), t_int=t_int, noise=noise)
        opt.zero_grad()
        out[4].backward()
        opt.step()
        losses.append(float(out[4].detach()))
    print('overfit l2:', losses[0], '->', losses[-1])
    assert losses[-1] < 0.5 * losses[0], losses


def _toy_dataset(n_mols, nf, seed):
    g = torch.Generator().manual_seed(seed)
    data = []
    for k in range(n_mols):
        n_frag, n_link = 6 + k % 4, 3
        n = n_frag + n_link
        link = torch.zeros(n)
        link[n_frag:] = 1
        data.append({'uuid': k, 'name': f'mol{k}', 'positions': 2.0 * torch.randn((n, 3), generator=g),
                     'one_hot': torch.nn.functional.one_hot(torch.randint(0, nf, (n,), generator=g), nf).float(),
                     'charges': torch.zeros(n), 'anchors': torch.zeros(n), 'fragment_mask': 1 - link, 'linker_mask': link,
                     'num_atoms': n})
    return data


def test_train_cli_writes_loadable_checkpoint(tmp_path):
    from difflinker_amd import DDPM
    from difflinker_amd.const import NUMBER_OF_ATOM_TYPES
    torch.save(_toy_dataset(6, NUMBER_OF_ATOM_TYPES, 0), os.path.join(tmp_path, 'zinc_final_train.pt'))
    torch.save(_toy_dataset(3, NUMBER_OF_ATOM_TYPES, 1), os.path.join(tmp_path, 'zinc_final_val.pt'))
    cfg = os.path.join(tmp_path, 'cfg.yml')
    with open(cfg, 'w') as f:
        f.write('nf: 128\nn_layers: 1\ninv_sublayers: 1\ntanh: False\nattention: False\nnorm_constant: 0.000001\n'
                'normalization_factor: 100\ninclude_charges: False\nbatch_size: 3\nlr: 0.0002\nnormalize_factors: [1, 4, 10]\n'
                'train_data_prefix: zinc_final_train\nval_data_prefix: zinc_final_val\n')
    ck = os.path.join(tmp_path, 'ck')
    run = lambda *extra: subprocess.run([sys.executable, '-m', 'difflinker_amd.train', '--config', cfg, '--data',   # noqa: E731
                                         str(tmp_path), '--checkpoints', ck, *extra], cwd=ROOT, capture_output=True,
                                        text=True, timeout=600)
    proc = run('--max_steps', '3')
    assert proc.returncode == 0, proc.stderr[-3000:]
    path = os.path.join(ck, 'last.ckpt')
    assert json.loads(proc.stdout.strip().splitlines()[-1])['step'] == 3
    proc = run('--max_steps', '4', '--resume', path)
    assert proc.returncode == 0, proc.stderr[-3000:]
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert ckpt['global_step'] == 4 and ckpt['optimizer_states']
    model = DDPM.load_from_checkpoint(path, map_location='cpu', torch_device='cuda:0').to(DEV).eval()
    model.data_path = str(tmp_path)
    model.setup('val')
    data = next(iter(model.val_dataloader()))
    model.edm.T = 5
    chain, nm = model.sample_chain(data, keep_frames=1)
    assert torch.isfinite(chain).all()


GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'edm_grad.npz'))


@pytest.mark.parametrize('tag', ['fc', 't0', 'inpaint', 'ragged_vlb'])
def test_loss_gradient_matches_reference_fixture(tag):
    """``loss.backward()`` of the unmodified reference (tests/golden/make_golden_grad.py) on the same inputs and draws."""
    from difflinker_amd import Dynamics, EDM, InpaintingEDM
    nf, ctx, L, T, wseed, inpainting, vlb = (int(v) for v in GOLDEN[f'{tag}.params'])
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, norm_constant=1e-6,
                   normalization_factor=100, normalization='batch_norm', centering=bool(inpainting))
    sd = trained_like_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, wseed, coord_gain=0.02), wseed)
    dyn.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    edm = (InpaintingEDM if inpainting else EDM)(dyn, in_node_nf=nf, n_dims=3, timesteps=T, noise_schedule='polynomial_2',
                                                 noise_precision=1e-5, loss_type='vlb' if vlb else 'l2',
                                                 norm_values=[1, 4, 10]).to(DEV)
    g = {k: torch.from_numpy(GOLDEN[f'{tag}.{k}']).to(DEV) for k in ('x', 'h', 'node_mask', 'fragment_mask', 'linker_mask',
                                                                     'edge_mask', 'context', 't_int', 'noise_x', 'noise_h')}
    res = edm.training_forward(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'],
                               g['context'], t_int=g['t_int'], noise=(g['noise_x'], g['noise_h']))
    loss = res[1] + res[2] + res[3] - res[0] if vlb else res[4]
    dyn.zero_grad()
    loss.backward()
    hip, ref = {}, {}
    for k, p in dyn.named_parameters():
        want = torch.from_numpy(GOLDEN[f'{tag}.grad.{k}']).double()
        got = p.grad.detach().cpu().reshape(-1)
        if f'{tag}.idx.{k}' in GOLDEN:
            got = got[torch.from_numpy(GOLDEN[f'{tag}.idx.{k}']).long()]
        hip[k], ref[k] = got, want
    total, worst = compare(hip, ref)
    print(f'{tag}: reference fixture rel-L2 all {total:.2e}, worst tensor {worst:.2e}')
    assert total <= BAR_ALL and worst <= BAR_TENSOR, (total, worst)
