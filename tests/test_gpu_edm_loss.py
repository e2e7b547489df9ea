"""``EDM.forward`` / ``InpaintingEDM.forward`` on the GPU: the loss and VLB terms of held-out data (src/edm.py:41-124,
:467-548) - golden parity with the unmodified reference, per-molecule rows against an fp64 restatement, the two noise
sources, determinism, and the DDPM / command-line layers."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ragged_fc_molecules, seeded_state_dict, trained_like_state_dict
from oracle import egnn_oracle, philox_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'edm_loss.npz'))
NAMES = ('delta_log_px', 'kl_prior', 'loss_term_t', 'loss_term_0', 'l2_loss', 'noise_t', 'noise_0')
DEV = torch.device('cuda:0')


def make_edm(nf, ctx, L, T, wseed, pockets=False, inpainting=False, timesteps=None):
    from difflinker_amd import Dynamics, DynamicsWithPockets, EDM, InpaintingEDM
    cls = DynamicsWithPockets if pockets else Dynamics
    dyn = cls(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, norm_constant=1e-6,
              normalization='batch_norm', centering=inpainting, graph_type='FC-10A-4A' if pockets else 'FC')
    sd = trained_like_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, wseed, coord_gain=0.02), wseed)
    dyn.load_state_dict(sd, strict=True)
    edm = (InpaintingEDM if inpainting else EDM)(dyn, in_node_nf=nf, n_dims=3, timesteps=timesteps or T,
                                                 noise_schedule='polynomial_2', noise_precision=1e-5, loss_type='l2',
                                                 norm_values=[1, 4, 10])
    edm.T = T
    return edm.to(DEV).eval(), sd


def golden_case(tag):
    nf, ctx, L, T, wseed, pockets, inpainting = (int(v) for v in GOLDEN[f'{tag}.params'])
    edm, _ = make_edm(nf, ctx, L, T, wseed, bool(pockets), bool(inpainting))
    g = {k: torch.from_numpy(GOLDEN[f'{tag}.{k}']) for k in ('x', 'h', 'node_mask', 'fragment_mask', 'linker_mask',
                                                           'edge_mask', 'context', 't_int', 'noise_x', 'noise_h')}
    return edm, {k: v.to(DEV) for k, v in g.items()}


def call(edm, g, **kw):
    with torch.no_grad():
        return edm(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'], **kw)


def bits(v):
    return torch.as_tensor(v, dtype=torch.float32).reshape(1).cpu().view(torch.int32)


def same_outputs(a, b):
    return all(type(x) is type(y) and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('tag', ['fc', 't0', 'inpaint', 'pocket'])
def test_golden_parity_with_the_reference(tag):
    """The 7 outputs of the reference's forward (CPU fp32) from the same t_int and noise: relative 1e-4 per term, NaN
    where the reference has NaN (no molecule with t > 0), the float 0. where it has 0. (no molecule with t = 0)."""
    edm, g = golden_case(tag)
    got = call(edm, g, t_int=g['t_int'], noise=(g['noise_x'], g['noise_h']))
    ref = GOLDEN[f'{tag}.outputs']
    has_t0 = bool(GOLDEN[f'{tag}.has_t0'])
    errs = {}
    for k, name in enumerate(NAMES):
        if name in ('loss_term_0', 'noise_0') and not has_t0:
            assert isinstance(got[k], float) and got[k] == 0., (name, got[k])
            continue
        v = float(got[k])
        if math.isnan(ref[k]):
            assert math.isnan(v), (name, v)
            continue
        errs[name] = abs(v - float(ref[k])) / max(abs(float(ref[k])), 1e-30) if ref[k] != 0 else abs(v)
    print(f'[edm loss golden {tag}] ' + ' '.join(f'{k} {e:.1e}' for k, e in errs.items()))
    for name, e in errs.items():
        assert e <= 1e-4, (name, e)


def restate_rows(edm, sd, cfg, x, h, nm, fm, lm, em, ctx, t_int, nx, nh, inpainting=False):
    """fp64 restatement of edm.py:41-124, 244-326 per molecule around the oracle's Dynamics.forward: the rows of
    dl_edm_loss_epilogue."""
    d64 = torch.float64
    T, ts = edm.T, edm.gamma.timesteps
    table = edm.gamma.gamma.detach().cpu().to(d64)
    p = {k: v.to(d64) for k, v in sd.items()}
    xh = torch.cat([x.to(d64), h.to(d64) / 4.0], 2)
    nm, fm, lm, ctx = nm.to(d64), fm.to(d64), lm.to(d64), ctx.to(d64)
    mask = nm if inpainting else lm
    t = t_int.to(d64).reshape(-1, 1) / T

    def lookup(tt):
        return table[torch.round(tt * ts).long().reshape(-1)]
    gt, gs = lookup(t), lookup(t - 1.0 / T)
    alpha, sigma = torch.sigmoid(-gt).sqrt().view(-1, 1, 1), torch.sigmoid(gt).sqrt().view(-1, 1, 1)
    ex = nx.to(d64) * mask
    if inpainting:
        ex = ex - ex.sum(1, keepdim=True) / mask.sum(1, keepdim=True) * mask
    eps = torch.cat([ex, nh.to(d64) * mask], 2)
    z = alpha * xh + sigma * eps
    if not inpainting:
        z = xh * fm + z * lm
    eps_hat = egnn_oracle.dynamics_forward(p, cfg, t, z, nm, None if inpainting else lm, em, ctx)
    if not inpainting:
        eps_hat = eps_hat * lm
    err = ((eps - eps_hat) ** 2).sum((1, 2))
    n = mask.sum((1, 2))
    d = (n - 1) * 3 if inpainting else n * 3
    gT, g0 = table[ts], table[0]
    aT, sT = torch.sigmoid(-gT).sqrt(), torch.sigmoid(gT).sqrt()
    mu = aT * xh
    kl_h = (torch.log(1 / sT) + 0.5 * (sT ** 2 + mu[..., 3:] ** 2) - 0.5).sum((1, 2))
    kl_x = d * torch.log(1 / sT) + 0.5 * (d * sT ** 2 + (mu[..., :3] ** 2).sum((1, 2))) - 0.5 * d
    log_px = -0.5 * ((eps - eps_hat)[..., :3] ** 2).sum((1, 2))
    sigma0 = torch.sigmoid(gt).sqrt().view(-1, 1, 1) * 4.0
    cen = z[..., 3:] * 4.0 - 1.0
    cdf = lambda v: 0.5 * (1 + torch.erf(v / math.sqrt(2)))       # noqa: E731
    lp = torch.log(cdf((cen + 0.5) / sigma0) - cdf((cen - 0.5) / sigma0) + 1e-10)
    lp = lp - torch.logsumexp(lp, dim=2, keepdim=True)
    log_ph = (lp * (xh[..., 3:] * 4.0) * mask).sum((1, 2))
    log_const = d * (-0.5 * g0 - 0.5 * np.log(2 * np.pi))
    snr = torch.exp(-(gs - gt)) - 1
    return torch.stack([err, eps_hat.pow(2).sum((1, 2)).sqrt(), kl_x + kl_h, log_px, log_ph, log_const, snr, n], 1)


@pytest.mark.parametrize('inpainting', [False, True])
def test_rows_against_fp64_restatement(inpainting):
    """Per-molecule epilogue rows against fp64, at sizes on one compute unit (<= 55 atoms), on teams (60..80) and on the
    HBM-resident kernels (~120), t from 0 to T on the 500-entry table."""
    from difflinker_amd.datasets import collate
    nf, ctx, L, T = 9, 1, 2, 500
    sizes, linkers = [40, 52, 64, 78, 118, 20, 33], [8, 10, 12, 14, 20, 5, 7]
    data = collate(ragged_fc_molecules(sizes, linkers, nf, seed=91))
    B, N = data['positions'].shape[:2]
    edm, sd = make_edm(nf, ctx, L, T, 92, inpainting=inpainting)
    cfg = egnn_oracle.EGNNConfig(in_node_nf=nf, context_node_nf=ctx, n_layers=L, centering=inpainting)
    nm, fm, lm = data['atom_mask'].float(), data['fragment_mask'], data['linker_mask']
    x = data['positions'] - (data['positions'] * fm).sum(1, keepdim=True) / fm.sum(1, keepdim=True) * nm
    h, em, ctx_t = data['one_hot'], data['edge_mask'], fm
    g = torch.Generator().manual_seed(93)
    t_int = torch.tensor([0, 1, 250, 500, 37, 499, 3], dtype=torch.int64)
    nx, nh = torch.randn((B, N, 3), generator=g), torch.randn((B, N, nf), generator=g)
    on = lambda v: v.to(DEV)                                        # noqa: E731
    with torch.no_grad():
        rows, t_dev = edm._loss_rows(on(x), on(h), on(data['atom_mask']), on(fm), on(lm), on(em), on(ctx_t), on(t_int),
                                     (on(nx), on(nh)), 0)
    rows = rows.cpu().double()
    assert torch.equal(t_dev.cpu().long(), t_int)
    ref = restate_rows(edm, sd, cfg, x, h, nm, fm, lm, em, ctx_t, t_int, nx, nh, inpainting=inpainting)
    rel = (rows - ref).abs() / ref.abs().clamp_min(1.0)
    err_t = ((rows[:, 0] - ref[:, 0]).abs() / ref[:, 0].abs()).max().item()
    print(f'[edm loss fp64 inpainting={inpainting}] error_t max rel {err_t:.2e}; per column max '
          + ' '.join(f'{v:.1e}' for v in rel.max(0).values.tolist()))
    assert rel.max().item() <= 1e-4
    assert err_t <= 2e-6


def test_torch_noise_is_the_reference_call_sequence():
    edm, g = golden_case('fc')
    torch.manual_seed(1234)
    a = call(edm, g)
    torch.manual_seed(1234)
    B, N = g['x'].shape[:2]
    t_int = torch.randint(0, edm.T + 1, size=(B, 1), device=DEV)
    nx, nh = torch.randn((B, N, 3), device=DEV), torch.randn((B, N, edm.in_node_nf), device=DEV)
    b = call(edm, g, t_int=t_int, noise=(nx, nh))
    assert same_outputs(a, b)


def _philox_rows(edm, g, seed, lo, hi):
    edm.noise_source, edm.noise_seed = 'philox', seed
    em = g['edge_mask'].reshape(g['x'].shape[0], -1)[lo:hi].reshape(-1, 1)
    with torch.no_grad():
        rows, t_int = edm._loss_rows(g['x'][lo:hi], g['h'][lo:hi], g['node_mask'][lo:hi], g['fragment_mask'][lo:hi],
                                     g['linker_mask'][lo:hi], em, g['context'][lo:hi], None, None, lo)
    assert edm.noise_seed == seed + 1
    return rows.cpu(), t_int.cpu()


def test_philox_draws_do_not_depend_on_the_batch_split_and_follow_the_keying():
    edm, g = golden_case('fc')
    seed = 0x0123456789ABCDEF
    edm.team_batch = 8                                  # a shard pins the team size of the whole batch
    whole, t_whole = _philox_rows(edm, g, seed, 0, 8)
    first, t_first = _philox_rows(edm, g, seed, 0, 4)
    second, t_second = _philox_rows(edm, g, seed, 4, 8)
    assert torch.equal(whole, torch.cat([first, second])) and torch.equal(t_whole, torch.cat([t_first, t_second]))
    # the documented keying: t_int = mulhi(r[0], T + 1) of counter (mol, 0, 0x80000001, 0); eps = philox_normal(seed, mol,
    # atom, 0x80000000, component)
    T, B, N, nf = edm.T, 8, g['x'].shape[1], edm.in_node_nf
    counter = np.stack([np.arange(B), np.zeros(B), np.full(B, 0x80000001), np.zeros(B)], 1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    r0 = philox_oracle.philox4x32_10(counter, key)[:, 0].astype(np.uint64)
    t_ref = torch.from_numpy(((r0 * np.uint64(T + 1)) >> np.uint64(32)).astype(np.int32))
    assert torch.equal(t_whole, t_ref)
    nx, nh = philox_oracle.normal_bank(seed, B, N, nf, 1, draw0=0x80000000)
    edm.noise_source = 'torch'
    with torch.no_grad():
        explicit, _ = edm._loss_rows(g['x'][:8], g['h'][:8], g['node_mask'][:8], g['fragment_mask'][:8],
                                     g['linker_mask'][:8], g['edge_mask'].reshape(10, -1)[:8].reshape(-1, 1),
                                     g['context'][:8], t_ref.to(DEV), (nx[0].to(DEV), nh[0].to(DEV)), 0)
    rel = ((explicit.cpu() - whole).abs() / whole.abs().clamp_min(1.0)).max().item()
    print(f'[edm loss philox] rows from the restated draws: max rel {rel:.1e}')
    assert rel <= 1e-5
    # no counter of the loss is one of a chain of the same seed: chains use draw words 0 .. T + 1 (EDM) and 0 .. 2T + 2
    # (inpainting), the loss 0x80000000 and 0x80000001
    chain_draws = set(range(0, 2 * T + 3))
    assert not ({0x80000000, 0x80000001} & chain_draws)
    bank_x, _ = edm.philox_noise_bank(B, N, DEV, seed=seed)
    for k in range(T + 2):
        assert not torch.allclose(bank_x[k].cpu(), nx[0], atol=1e-3)


def test_reproducible_bit_for_bit():
    edm, g = golden_case('fc')
    edm.noise_source = 'philox'
    edm.noise_seed = 77
    a = call(edm, g)
    edm.noise_seed = 77
    b = call(edm, g)
    assert same_outputs(a, b)
    edm.noise_source = 'torch'
    torch.manual_seed(5)
    c = call(edm, g)
    torch.manual_seed(5)
    d = call(edm, g)
    assert same_outputs(c, d)


def _toy_dataset(n_mols, nf, pockets=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = []
    for k in range(n_mols):
        n_frag, n_link, n_pock = 6 + k, 3, (5 if pockets else 0)
        n = n_frag + n_pock + n_link
        frag_only = torch.zeros(n)
        frag_only[:n_frag] = 1
        pock = torch.zeros(n)
        pock[n_frag:n_frag + n_pock] = 1
        link = torch.zeros(n)
        link[n_frag + n_pock:] = 1
        item = {'uuid': k, 'name': f'mol{k}', 'positions': 2.0 * torch.randn((n, 3), generator=g),
                'one_hot': torch.nn.functional.one_hot(torch.randint(0, nf, (n,), generator=g), nf).float(),
                'charges': torch.zeros(n), 'anchors': torch.zeros(n), 'fragment_mask': frag_only + pock,
                'linker_mask': link, 'num_atoms': n}
        if pockets:
            item['fragment_only_mask'] = frag_only
            item['pocket_mask'] = pock
        data.append(item)
    return data


@pytest.mark.parametrize('pockets', [False, True])
def test_ddpm_validation_and_test_step_and_cli(tmp_path, pockets):
    from difflinker_amd import DDPM, utils
    from difflinker_amd.evaluate import evaluate
    nf = 9 if pockets else 8
    prefix = 'MOAD_test.full' if pockets else 'zinc_final_test'
    torch.save(_toy_dataset(5, nf, pockets=pockets), os.path.join(tmp_path, ('MOAD_test_full' if pockets else prefix) + '.pt'))
    hp = dict(in_node_nf=nf, n_dims=3, context_node_nf=2 if pockets else 1, hidden_nf=128, activation='silu', tanh=False,
              n_layers=2, attention=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
              normalization_factor=100, aggregation_method='sum', diffusion_steps=500,
              diffusion_noise_schedule='polynomial_2', diffusion_noise_precision=1e-5, diffusion_loss_type='vlb',
              normalize_factors=[1, 4, 10], include_charges=False, model='egnn_dynamics', data_path=str(tmp_path),
              train_data_prefix='MOAD_train.full' if pockets else 'zinc_final_train', val_data_prefix=prefix,
              batch_size=2, lr=2e-4, torch_device='cuda:0', test_epochs=20, n_stability_samples=10,
              normalization='batch_norm', anchors_context=False, graph_type='FC-10A-4A' if pockets else None)
    m = DDPM(**hp)
    m.edm.dynamics.load_state_dict(seeded_state_dict(nf + hp['context_node_nf'] + 1, 128, 2, 95, coord_gain=0.02), strict=True)
    m = m.to(DEV).eval()
    m.setup('val')
    batch = next(iter(m.val_dataloader()))
    for step in (m.validation_step, m.test_step):
        torch.manual_seed(11)
        out = step(batch)
        assert set(out) == {'loss', 'delta_log_px', 'kl_prior', 'loss_term_t', 'loss_term_0', 'l2_loss', 'vlb_loss',
                            'noise_t', 'noise_0'}
        # by hand: context, centre of mass, EDM.forward, the reference's composition (lightning.py:228-247)
        fm, nm = batch['fragment_mask'], batch['atom_mask']
        if pockets:
            ctx = torch.cat([batch['fragment_only_mask'], fm - batch['fragment_only_mask']], -1)
            com = batch['fragment_only_mask']
        else:
            ctx, com = fm, fm
        x = utils.remove_partial_mean_with_mask(batch['positions'], nm, com)
        torch.manual_seed(11)
        with torch.no_grad():
            res = m.edm(x, batch['one_hot'], nm, fm, batch['linker_mask'], batch['edge_mask'], ctx)
        vlb = res[1] + res[2] + res[3] - res[0]
        want = dict(zip(NAMES, res), vlb_loss=vlb, loss=vlb)
        for k, v in want.items():
            assert torch.equal(bits(out[k]), bits(v)), k
    # the command line on the same files, philox draws keyed by the molecule's index in the data set
    ckpt = os.path.join(tmp_path, 'm.ckpt')
    torch.save(m.checkpoint_dict(), ckpt)
    m.edm.noise_source, m.edm.noise_seed = 'philox', 5
    want = evaluate(m, m.val_dataloader())
    assert set(want) >= {'loss', 'vlb_loss', 'l2_loss'} and math.isfinite(want['l2_loss'])
    proc = subprocess.run([sys.executable, '-m', 'difflinker_amd.evaluate', '--checkpoint', ckpt, '--data', str(tmp_path),
                           '--prefix', prefix, '--batch_size', '2', '--noise_source', 'philox', '--seed', '5',
                           '--device', 'cuda:0'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert set(got) == set(want)
    for k in want:
        assert (math.isnan(got[k]) and math.isnan(want[k])) or got[k] == want[k], (k, got[k], want[k])
