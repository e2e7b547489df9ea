"""The hand-over of a ragged batch inside ONE launch (EDM.split_chain -> dl_sample_chain_fc_join): each of split_plan's team
molecules moves to a team of two as soon as a molecule that finished its own chain joins it (edm.join_plan)."""
import pytest
import torch

import test_gpu_parity as P
from helpers import rel_l2
from oracle import edm_oracle

pytestmark = pytest.mark.gpu

NF, T = 8, 24
SIZES, LINKERS = [50, 48, 50, 47, 20, 22, 18, 25, 21, 19, 23, 20], [8, 7, 9, 6, 4, 5, 3, 6, 4, 4, 5, 4]


def _edm(dyn, nf, T):
    from difflinker_amd import EDM
    edm = EDM(dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(P.dev())
    edm.T = T
    return edm


def _case(L, seed):
    dyn, sd, cfg = P.make_dynamics(NF, 1, L, seed=seed)
    dyn.team = 1
    inp, _, _ = P.ragged_inputs(SIZES, LINKERS, NF, seed=seed + 1)
    B, N = inp['x'].shape[:2]
    edm = _edm(dyn, NF, T)
    bank = edm_oracle.NoiseBank.generate(T, B, N, 3, NF, seed=seed + 2)
    g = {k: v.to(P.dev()) for k, v in inp.items()}
    return dyn, sd, cfg, inp, edm, bank, g


def _run(edm, g, split, noise, keep=6):
    edm.split_chain = split
    out = edm.sample_chain(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'],
                           keep_frames=keep, noise_bank=noise)
    torch.cuda.synchronize()
    return out.cpu()


def _plan(L):
    from difflinker_amd import edm as edm_mod
    cus = torch.cuda.get_device_properties(P.dev()).multi_processor_count
    plan = edm_mod.join_plan(SIZES, LINKERS, T + 1, cus, L, 2)
    assert plan is not None
    return plan


def _against_one_launch(got, one, inp, owners):
    untouched = sorted(set(range(len(SIZES))) - set(owners))
    assert torch.equal(got[:, untouched], one[:, untouched]), 'molecules that never run on a team: the bits of the one-launch chain'
    lm = inp['linker_mask'][owners]
    err = rel_l2(got[0, owners, :, :3] * lm, one[0, owners, :, :3] * lm)
    assert err <= 1e-5 and torch.equal(got[0, owners, :, 3:], one[0, owners, :, 3:]), err
    return err


def test_join_launch_samples_the_oracles_chain_repeatably():
    """One launch, teams formed inside it: the oracle's chain in every kept frame, bitwise repeatable, molecules off the teams
    bit-identical to the one-launch chain, team molecules within fp32 rounding of it."""
    L = 2
    dyn, sd, cfg, inp, edm, bank, g = _case(L, 211)
    q_end, owners, helpers = _plan(L)
    orc = edm_oracle.EDMOracle(edm_oracle.make_dynamics_oracle(sd, cfg), in_node_nf=NF, timesteps=500)
    orc.T = T
    want = orc.sample_chain(inp['x'], inp['h'], inp['node_mask'], inp['fragment_mask'], inp['linker_mask'], inp['edge_mask'],
                            inp['context'], bank, keep_frames=6)
    got = _run(edm, g, True, bank.stacked())
    assert edm.last_split_event is None, 'one launch per chain'
    P.check_chain(f'join chain ({len(owners)} teams), T=24, 6 frames', got, want, inp)
    assert torch.equal(got, _run(edm, g, True, bank.stacked())), 'bitwise repeatable'
    err = _against_one_launch(got, _run(edm, g, False, bank.stacked()), inp, owners)
    print(f'join vs one launch, team molecules: linker-x rel-L2 {err:.3e}')


@pytest.mark.parametrize('who_waits', ['owner', 'helper'])
def test_join_launch_with_forced_switch_calls(monkeypatch, who_waits):
    """Forced plans: every owner switches after its first call (it waits for a helper that still has its whole chain to run),
    or at its last call (the helper waits for it).  Either way the numbers of the default plan's checks hold."""
    from difflinker_amd import edm as edm_mod
    L = 1
    dyn, sd, cfg, inp, edm, bank, g = _case(L, 221)
    q_end, owners, helpers = _plan(L)
    forced = list(q_end)
    for o in owners:
        forced[o] = 1 if who_waits == 'owner' else T
    monkeypatch.setattr(edm_mod, 'join_plan', lambda *a_, **k_: (forced, owners, helpers))
    got = _run(edm, g, True, bank.stacked(), keep=3)
    assert torch.equal(got, _run(edm, g, True, bank.stacked(), keep=3)), 'bitwise repeatable'
    err = _against_one_launch(got, _run(edm, g, False, bank.stacked(), keep=3), inp, owners)
    print(f'{who_waits} waits: team molecules vs one launch, linker-x rel-L2 {err:.3e}')


def test_join_launch_reports_nans_like_one_launch():
    """A NaN planted in an owner before its switch call, in an owner's team phase, and in a helper's own molecule (the helper
    still joins its team): the exception carries what the one-launch chain reports."""
    from difflinker_amd.utils import FoundNaNException
    L = 1
    dyn, sd, cfg, inp, edm, bank, g = _case(L, 231)
    q_end, owners, helpers = _plan(L)
    o, hp = owners[0], helpers[0]
    assert 3 < q_end[o] < T - 3
    for draw, mol in ((2, o), (q_end[o] + 2, o), (3, hp)):
        nx, nh = (t_.clone() for t_ in bank.stacked())
        nx[draw, mol, SIZES[mol] - 1, 0] = float('nan')            # a linker atom: z after step draw - 1 holds a NaN -> call `draw`
        seen = {}
        for split in (False, True):
            with pytest.raises(FoundNaNException) as ei:
                _run(edm, g, split, (nx, nh), keep=1)
            e = ei.value
            seen[split] = (e.x_h_nan_idx, e.only_x_nan_idx, e.only_h_nan_idx, e.first_step)
        print(f'NaN in draw {draw} of molecule {mol} (owner {o} switches at {q_end[o]}, helper {hp}): '
              f'one launch {seen[False]}, join {seen[True]}')
        assert seen[True] == seen[False] and (seen[True][0] | seen[True][1] | seen[True][2]) == {mol} and seen[True][3] == draw


def test_join_launch_team_fault_ends_in_the_one_compute_unit_rerun():
    """dl_debug_team_fault: the helpers give up at their first exchange, every team molecule is flagged void (bit 3), and the
    drop-in re-runs the chain with one compute unit per molecule: the one-launch chain's bits, no exception."""
    from difflinker_amd import _lib
    L = 1
    with _lib.test_hooks() as lib:
        dyn, sd, cfg, inp, edm, bank, g = _case(L, 241)
        one = _run(edm, g, False, bank.stacked(), keep=2)
        lib.dl_debug_team_fault(1)
        with pytest.warns(RuntimeWarning, match='did not assemble'):
            got = _run(edm, g, True, bank.stacked(), keep=2)
    assert torch.equal(got, one)
