"""The C ABI on its own (include/difflinker_hip.h through raw ctypes; PyTorch only provides the device buffers): a host
that is not the Python drop-in gets the same numbers and the documented status codes."""
import ctypes

import pytest
import torch

from helpers import seeded_state_dict, rel_l2
from oracle import egnn_oracle
from oracle.egnn_oracle import EGNNConfig
from test_gpu_parity import ragged_inputs, FWD_TOLS

FWD_TOL = FWD_TOLS['f16x3']          # DLConfig(..., precision = 1) below: the default arithmetic

pytestmark = pytest.mark.gpu


def test_forward_through_raw_ctypes_matches_oracle_and_reports_errors():
    from difflinker_amd import _lib
    from difflinker_amd.egnn import egnn_tensor_order
    lib = _lib.load()
    nf, ctx, L = 9, 1, 2
    sd = seeded_state_dict(nf + ctx + 1, 128, L, seed=123)
    host = [sd['dynamics.' + k].contiguous() for k in egnn_tensor_order(L)]
    cfg = _lib.DLConfig(3, nf, ctx, 128, L, 2, 1, 1e-6, 100.0, 1)
    assert lib.dl_model_num_tensors(ctypes.byref(cfg)) == len(host)
    ptrs = (ctypes.c_void_p * len(host))(*[t.data_ptr() for t in host])
    model = ctypes.c_void_p()
    assert lib.dl_model_create(ctypes.byref(cfg), ptrs, len(host), ctypes.byref(model)) == 0
    try:
        inp, z, t = ragged_inputs([20, 55, 9], [4, 7, 2], nf, seed=5)
        B, N = z.shape[:2]
        d = torch.device('cuda:0')
        xh, tt = z.to(d).contiguous(), t.to(d).contiguous()
        nm = inp['node_mask'].reshape(B, N).to(torch.int8).to(d).contiguous()
        lm = inp['linker_mask'].reshape(B, N).float().to(d).contiguous()
        em = inp['edge_mask'].reshape(B, N, N).to(torch.int8).to(d).contiguous()
        cx = inp['context'].reshape(B, N, ctx).float().to(d).contiguous()
        out = torch.full((B, N, 3 + nf), float('nan'), device=d)
        flags = torch.full((B,), -1, dtype=torch.int32, device=d)
        p = lambda x: ctypes.c_void_p(x.data_ptr())          # noqa: E731
        need = lib.dl_workspace_bytes(B, 1)                  # ABI v6: the caller owns the scratch, the callee allocates nothing
        ws = torch.empty(need, dtype=torch.uint8, device=d)
        st = lib.dl_egnn_forward_fc(model, B, N, p(xh), p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags), p(ws), need, None)
        assert st == 0
        torch.cuda.synchronize()
        ref = egnn_oracle.dynamics_forward({k: v for k, v in sd.items()}, EGNNConfig(in_node_nf=nf, context_node_nf=ctx, n_layers=L),
                                           t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'])
        # the suite's forward bar for the default arithmetic (tests/test_gpu_parity.FWD_TOLS['f16x3']; VERDICT round 5: 2e-5 here)
        assert rel_l2(out.cpu()[..., 3:], ref[..., 3:]) <= FWD_TOL and flags.cpu().tolist() == [0, 0, 0]
        # the coordinates the sampler consumes, x + vel, at the same bar; the raw velocity - a difference of fp32 coordinates,
        # a few ulp(|x|) of absolute error on both sides - at the north-star bar (as tests/test_gpu_parity.report does)
        assert rel_l2(z[..., :3] + out.cpu()[..., :3], z[..., :3] + ref[..., :3]) <= FWD_TOL
        assert rel_l2(out.cpu()[..., :3], ref[..., :3]) <= 1e-4
        assert float(out.cpu()[..., :3].abs().max()) > 0
        # status codes: null pointer, negative batch, a molecule with more atoms than dl_max_atoms() (flag bit 2)
        assert lib.dl_egnn_forward_fc(model, B, N, None, p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags), p(ws), need, None) == -1
        assert lib.dl_egnn_forward_fc(model, -1, N, p(xh), p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags), p(ws), need, None) == -1
        assert lib.dl_egnn_forward_fc(model, 0, N, p(xh), p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags), p(ws), need, None) == 0
        big, zb, tb = ragged_inputs([56], [3], nf, seed=6)
        xb = zb.to(d).contiguous()
        nmb = big['node_mask'].reshape(1, 56).to(torch.int8).to(d).contiguous()
        lmb = big['linker_mask'].reshape(1, 56).float().to(d).contiguous()
        emb = big['edge_mask'].reshape(1, 56, 56).to(torch.int8).to(d).contiguous()
        cxb = big['context'].reshape(1, 56, ctx).float().to(d).contiguous()
        outb = torch.empty((1, 56, 3 + nf), device=d)
        fb = torch.zeros((1,), dtype=torch.int32, device=d)
        assert lib.dl_egnn_forward_fc(model, 1, 56, p(xb), p(tb.to(d)), 0, p(nmb), p(lmb), p(emb), p(cxb), p(outb), p(fb), p(ws), need, None) == 0
        torch.cuda.synchronize()
        assert int(fb.cpu()[0]) & 4 and float(outb.abs().max()) == 0.0
    finally:
        lib.dl_model_destroy(model)
    bad = _lib.DLConfig(3, nf, ctx, 64, L, 2, 1, 1e-6, 100.0, 1)              # hidden_nf != 128
    assert lib.dl_model_create(ctypes.byref(bad), ptrs, len(host), ctypes.byref(model)) == -2
    assert lib.dl_error_string(-3).decode().startswith('molecule exceeds')


def test_team_entry_points_through_raw_ctypes():
    """ABI v6: dl_egnn_forward_fc_team / dl_team_max / dl_workspace_bytes without the Python drop-in: same numbers as
    the one-workgroup entry point to fp32 rounding, documented refusals (team size, workspace size and alignment)."""
    from difflinker_amd import _lib
    from difflinker_amd.egnn import egnn_tensor_order
    lib = _lib.load()
    nf, ctx, L = 9, 1, 2
    sd = seeded_state_dict(nf + ctx + 1, 128, L, seed=124)
    host = [sd['dynamics.' + k].contiguous() for k in egnn_tensor_order(L)]
    cfg = _lib.DLConfig(3, nf, ctx, 128, L, 2, 1, 1e-6, 100.0, 1)
    ptrs = (ctypes.c_void_p * len(host))(*[t.data_ptr() for t in host])
    model = ctypes.c_void_p()
    assert lib.dl_model_create(ctypes.byref(cfg), ptrs, len(host), ctypes.byref(model)) == 0
    try:
        inp, z, t = ragged_inputs([20, 55, 9, 31, 2], [4, 7, 2, 5, 1], nf, seed=7)
        B, N = z.shape[:2]
        d = torch.device('cuda:0')
        xh, tt = z.to(d).contiguous(), t.to(d).contiguous()
        nm = inp['node_mask'].reshape(B, N).to(torch.int8).to(d).contiguous()
        lm = inp['linker_mask'].reshape(B, N).float().to(d).contiguous()
        em = inp['edge_mask'].reshape(B, N, N).to(torch.int8).to(d).contiguous()
        cx = inp['context'].reshape(B, N, ctx).float().to(d).contiguous()
        p = lambda x: ctypes.c_void_p(x.data_ptr())          # noqa: E731
        assert lib.dl_team_max(B) == 8
        need = max(lib.dl_workspace_bytes(B, team) for team in (1, 2, 4, 8))
        ws = torch.empty(need + 16, dtype=torch.uint8, device=d)
        outs = {}
        for team in (1, 2, 4, 8):
            out = torch.full((B, N, 3 + nf), float('nan'), device=d)
            flags = torch.full((B,), -1, dtype=torch.int32, device=d)
            st = lib.dl_egnn_forward_fc_team(model, B, N, p(xh), p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags),
                                             team, p(ws), lib.dl_workspace_bytes(B, team), None)
            torch.cuda.synchronize()
            assert st == 0 and flags.cpu().tolist() == [0] * B
            outs[team] = out.cpu()
        ref = egnn_oracle.dynamics_forward({k: v for k, v in sd.items()}, EGNNConfig(in_node_nf=nf, context_node_nf=ctx, n_layers=L),
                                           t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'])
        for team in (1, 2, 4, 8):
            assert rel_l2(outs[team][..., 3:], ref[..., 3:]) <= FWD_TOL
        out = torch.empty((B, N, 3 + nf), device=d)
        flags = torch.zeros((B,), dtype=torch.int32, device=d)
        args = (model, B, N, p(xh), p(tt), 0, p(nm), p(lm), p(em), p(cx), p(out), p(flags))
        need4, need1 = lib.dl_workspace_bytes(B, 4), lib.dl_workspace_bytes(B, 1)
        assert lib.dl_egnn_forward_fc_team(*args, 3, p(ws), need, None) == -1                 # team must be 1, 2, 4 or 8
        assert lib.dl_egnn_forward_fc_team(*args, 4, p(ws), need4 - 1, None) == -1            # workspace too small
        assert lib.dl_egnn_forward_fc_team(*args, 4, None, need4, None) == -1                 # no workspace
        assert lib.dl_egnn_forward_fc_team(*args, 4, ctypes.c_void_p(ws.data_ptr() + 4), need4, None) == -1   # not 16-byte aligned
        assert lib.dl_egnn_forward_fc_team(*args, 1, None, 0, None) == -1                     # ABI v6: team 1 needs its scratch too
        assert lib.dl_egnn_forward_fc(*args, p(ws), need1 - 1, None) == -1
        assert lib.dl_egnn_forward_fc(*args, p(ws), need1, None) == 0                         # the callee allocates nothing
        torch.cuda.synchronize()
        assert flags.cpu().tolist() == [0] * B and rel_l2(out.cpu()[..., 3:], ref[..., 3:]) <= FWD_TOL
    finally:
        lib.dl_model_destroy(model)


def test_join_entry_point_through_raw_ctypes_runs_a_valid_plan_and_refuses_every_bad_one():
    """``dl_join_workspace_bytes`` / ``dl_sample_chain_fc_join`` without ``EDM._sample_chain_fused``: a valid plan of one team
    (molecule 0 switches at call 2, molecule 2 helps) returns DL_OK and the numbers of the one-launch chain - bit for bit off the
    team, to fp32 rounding on it; every documented refusal answers its status code BEFORE anything is launched or cleared (the
    chain and the flags keep their sentinels)."""
    from difflinker_amd import _lib, Dynamics, EDM
    from oracle import edm_oracle
    lib = _lib.load()
    d = torch.device('cuda:0')
    # the workspace query: nothing for no teams, linear in the teams (one exchange block, arrival and join words per team)
    assert lib.dl_join_workspace_bytes(0) == 0 and lib.dl_join_workspace_bytes(-1) == 0 and lib.dl_join_workspace_bytes(-2 ** 31) == 0
    per_team = lib.dl_join_workspace_bytes(1)
    assert per_team > 0 and per_team % 16 == 0
    assert [lib.dl_join_workspace_bytes(k) for k in (2, 3, 7, 128)] == [k * per_team for k in (2, 3, 7, 128)]

    nf, ctx, L, T, keep = 8, 1, 1, 4, 2
    sizes, linkers = [30, 28, 10, 9], [5, 4, 3, 2]

    def model(**flags):
        dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, n_layers=L, norm_constant=1e-6, **flags)
        dyn.load_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, seed=125, edge_feat_nf=24 if flags else 2), strict=True)
        dyn.team = 1
        return dyn.to(d)
    dyn = model()
    edm = EDM(dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2', noise_precision=1e-5, loss_type='l2',
              norm_values=[1, 4, 10]).to(d)
    edm.T = T
    inp, _, _ = ragged_inputs(sizes, linkers, nf, seed=126)
    B, N = inp['x'].shape[:2]
    bank = edm_oracle.NoiseBank.generate(T, B, N, 3, nf, seed=127)
    g = {k: v.to(d) for k, v in inp.items()}
    edm.split_chain = False
    one = edm.sample_chain(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'],
                           keep_frames=keep, noise_bank=bank.stacked()).cpu()
    assert edm.last_route == 'one'

    coefs, (inv_alpha0, sigma0, sigma_x) = edm.step_coefficients(B)
    f32 = lambda t_, shape: t_.reshape(shape).to(torch.float32).to(d).contiguous()          # noqa: E731
    bufs = dict(x=f32(inp['x'], (B, N, 3)), h=f32(inp['h'], (B, N, nf)),
                node_mask=inp['node_mask'].reshape(B, N).to(torch.int8).to(d).contiguous(),
                fragment_mask=f32(inp['fragment_mask'], (B, N)), linker_mask=f32(inp['linker_mask'], (B, N)),
                edge_mask=inp['edge_mask'].reshape(B, N, N).to(torch.int8).to(d).contiguous(), context=f32(inp['context'], (B, N, ctx)),
                noise_x=bank.stacked()[0].to(d).contiguous(), noise_h=bank.stacked()[1].to(d).contiguous(),
                coefs=coefs.to(d).contiguous(), order=torch.arange(B, dtype=torch.int32, device=d),
                q_end=torch.tensor([2, T + 1, T + 1, T + 1], dtype=torch.int32, device=d),
                z_state=torch.empty((B, N, 3 + nf), device=d),
                chain=torch.full((keep, B, N, 3 + nf), float('nan'), device=d),
                nan_flags=torch.full((B,), -7, dtype=torch.int32, device=d), nan_step=torch.full((B,), -7, dtype=torch.int32, device=d))
    need = lib.dl_workspace_bytes(B, 1)
    bufs['workspace'] = torch.empty(need, dtype=torch.uint8, device=d)
    maps = torch.tensor([0, -1, 0, -1] + [0], dtype=torch.int32, device=d)            # team_of [B], then team_mol [teams]
    jneed = lib.dl_join_workspace_bytes(1)
    jws = torch.empty(jneed + 16, dtype=torch.uint8, device=d)
    spare = torch.zeros(B, dtype=torch.int32, device=d)                                # something to point q_begin / skip_flags at
    assert jws.data_ptr() % 16 == 0

    def chain_args(**over):
        a = _lib.DLChainArgs(B=B, N=N, T=T, keep_frames=keep, noise_seed=0, mol_offset=0, team=1, inv_alpha0=inv_alpha0, sigma0=sigma0,
                             sigma_x=sigma_x, norm_x=1.0, norm_h=4.0, bias_h=0.0, workspace_bytes=need, mol_index=None,
                             order_first=0, order_count=0, q_begin=None, skip_flags=None,
                             **{k: v.data_ptr() for k, v in bufs.items()})
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def join_args(**over):
        j = _lib.DLJoinArgs(teams=1, team_of=maps.data_ptr(), team_mol=maps.data_ptr() + 4 * B, workspace=jws.data_ptr(),
                            workspace_bytes=jneed, wait_ticks=None)
        for k, v in over.items():
            setattr(j, k, v)
        return j

    def call(handle, a, j):
        with torch.cuda.device(d):
            st = lib.dl_sample_chain_fc_join(handle, ctypes.byref(a), ctypes.byref(j), ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
        torch.cuda.synchronize()
        return st
    handle = dyn.hip_model(d)
    cus = torch.cuda.get_device_properties(d).multi_processor_count
    BAD_ARG, UNSUPPORTED = -1, -2
    refused = [
        ('teams = 0', chain_args(), join_args(teams=0), BAD_ARG),
        ('teams < 0', chain_args(), join_args(teams=-1), BAD_ARG),
        ('2 * teams > B', chain_args(), join_args(teams=3, workspace_bytes=lib.dl_join_workspace_bytes(3)), BAD_ARG),
        ('B above the compute units', chain_args(B=cus + 1), join_args(), BAD_ARG),
        ('q_begin set', chain_args(q_begin=spare.data_ptr()), join_args(), BAD_ARG),
        ('skip_flags set', chain_args(skip_flags=spare.data_ptr()), join_args(), BAD_ARG),
        ('no q_end', chain_args(q_end=None), join_args(), BAD_ARG),
        ('no z_state', chain_args(z_state=None), join_args(), BAD_ARG),
        ('order_first != 0', chain_args(order_first=1), join_args(), BAD_ARG),
        ('order_count != 0', chain_args(order_count=B), join_args(), BAD_ARG),
        ('join workspace one byte short', chain_args(), join_args(workspace_bytes=jneed - 1), BAD_ARG),
        ('no join workspace', chain_args(), join_args(workspace=None), BAD_ARG),
        ('join workspace not 16-byte aligned', chain_args(), join_args(workspace=jws.data_ptr() + 4), BAD_ARG),
        ('noise_x without noise_h', chain_args(noise_h=None), join_args(), BAD_ARG),
        ('noise_h without noise_x', chain_args(noise_x=None), join_args(), BAD_ARG),
        ('no team_of', chain_args(), join_args(team_of=None), BAD_ARG),
        ('a team of several compute units per molecule', chain_args(team=2), join_args(), BAD_ARG),
    ]
    for what, a, j, want in refused:
        assert call(handle, a, j) == want, what
    sin = model(sin_embedding=True)
    assert call(sin.hip_model(d), chain_args(), join_args()) == UNSUPPORTED, 'a sin_embedding model'
    # nothing ran and nothing was cleared: the sentinels are still there
    assert bool(torch.isnan(bufs['chain']).all()) and bufs['nan_flags'].cpu().tolist() == [-7] * B and bufs['nan_step'].cpu().tolist() == [-7] * B

    # the same arguments, unaltered: the chain (the caller clears the flags: the entry point does not)
    bufs['nan_flags'].zero_()
    bufs['nan_step'].fill_(-1)
    bufs['chain'].zero_()                                                              # (the kernel writes the rows of real atoms)
    assert call(handle, chain_args(), join_args()) == 0
    got = bufs['chain'].cpu()
    assert bufs['nan_flags'].cpu().tolist() == [0] * B and bufs['nan_step'].cpu().tolist() == [-1] * B
    assert torch.equal(got[:, 1:], one[:, 1:]), 'molecules 1..3 never run on a team (the helper samples its own chain alone)'
    lm = inp['linker_mask'][:1]
    err = rel_l2(got[0, :1, :, :3] * lm, one[0, :1, :, :3] * lm)
    print(f'raw join launch, the team molecule against one launch: linker-x rel-L2 {err:.3e}')
    assert err <= 1e-5 and torch.equal(got[0, :1, :, 3:], one[0, :1, :, 3:])
