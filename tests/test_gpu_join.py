"""The hand-over of a ragged batch inside ONE launch (EDM.split_chain -> dl_sample_chain_fc_join): each of split_plan's team
molecules moves to a team of two as soon as a molecule that finished its own chain joins it (edm.join_plan).

Every test asserts the route it means to test (``EDM.last_route``: 'join' here, 'one' for the chain it is compared with).  The
kernel has five instantiations - ``sample_chain_fc_kernel_join<PREC, ATT>``: <0,false>, <0,true>, <1,false>, <1,true>, <2,false> -
each of which inlines two chains and the meeting protocol; ``test_join_variant_*`` launch every one of them against the float64
oracle and against the one-launch chain of the same model."""
import pytest
import torch

import test_gpu_parity as P
from helpers import rel_l2, seeded_state_dict
from oracle import edm_oracle
from oracle.egnn_oracle import EGNNConfig

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


def _run(edm, g, split, noise, keep=6, route=None):
    """One chain by the join launch (``split``) or by one launch; the route is asserted, also when the chain raises."""
    edm.split_chain = split
    edm.last_route = None
    try:
        out = edm.sample_chain(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'],
                               keep_frames=keep, noise_bank=noise)
        torch.cuda.synchronize()
    finally:
        assert edm.last_route == (route or ('join' if split else 'one')), edm.last_route
    return out.cpu()


def _plan(L, sublayers=2):
    from difflinker_amd import edm as edm_mod
    cus = torch.cuda.get_device_properties(P.dev()).multi_processor_count
    plan = edm_mod.join_plan(SIZES, LINKERS, T + 1, cus, L, sublayers)
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
            got = _run(edm, g, True, bank.stacked(), keep=2, route='one')      # the join launch gave up (the warning); the re-run is the last chain
    assert torch.equal(got, one)


# ---- every instantiation of the join kernel, the optional hyper-parameters, another shape ----------------------------------
ATTENTION = dict(attention=True)
ALL_FLAGS = dict(attention=True, tanh=True, aggregation_method='mean')
VARIANTS = [('fp32', False), ('fp32', True), ('f16x3', False), ('f16x3', True), ('f16x2', False)]     # <0,f> <0,t> <1,f> <1,t> <2,f>


def _model(precision, seed, L, flags=None, nf=NF, ctx=1, hidden_nf=128, inv_sublayers=2, coord_gain=0.02):
    """A denoiser with seeded weights on one compute unit per molecule, its state_dict and the oracle's configuration."""
    from difflinker_amd import Dynamics
    flags = dict(flags or {})
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=hidden_nf, n_layers=L, inv_sublayers=inv_sublayers,
                   norm_constant=1e-6, normalization='batch_norm', **flags)
    dyn.precision = precision
    dyn.team = 1
    sd = seeded_state_dict(nf + ctx + 1, hidden_nf, L, seed, coord_gain=coord_gain, inv_sublayers=inv_sublayers,
                           attention=bool(flags.get('attention')))
    dyn.load_state_dict(sd, strict=True)
    cfg = EGNNConfig(in_node_nf=nf, context_node_nf=ctx, hidden_nf=hidden_nf, n_layers=L, inv_sublayers=inv_sublayers, **flags)
    return dyn.to(P.dev()), sd, cfg


def _inputs(dyn, nf, ctx, seed):
    inp, _, _ = P.ragged_inputs(SIZES, LINKERS, nf, seed=seed, ctx=ctx)
    B, N = inp['x'].shape[:2]
    bank = edm_oracle.NoiseBank.generate(T, B, N, 3, nf, seed=seed + 1)
    return inp, _edm(dyn, nf, T), bank, {k: v.to(P.dev()) for k, v in inp.items()}


def _oracle64(sd, cfg, nf, inp, bank, keep):
    """The oracle's chain in float64: the fp32 weights, inputs and draws, every operation of the network and the sampler in
    double - a reference whose own rounding (1e-16) is far below anything the kernels are held to."""
    orc = edm_oracle.EDMOracle(edm_oracle.make_dynamics_oracle({k: v.double() for k, v in sd.items()}, cfg), in_node_nf=nf,
                               timesteps=500, dtype=torch.float64)
    orc.T = T
    d = {k: v.double() for k, v in inp.items()}
    return orc.sample_chain(d['x'], d['h'], d['node_mask'], d['fragment_mask'], d['linker_mask'], d['edge_mask'], d['context'],
                            edm_oracle.NoiseBank([t_.double() for t_ in bank.draws]), keep_frames=keep)


def _join_case(tag, dyn, sd, cfg, owners, nf=NF, ctx=1, seed=0, keep=6):
    """The checks of one join-route case: route by name (in _run), the float64 oracle's chain in every kept frame (for the join
    launch and, as the yardstick of what this arithmetic does on these inputs, for one launch), bitwise repeatable, molecules
    off the teams bit-identical to one launch, team molecules within the 1e-5 of _against_one_launch.  Every molecule counts:
    the chains are finite and the atom types unambiguous, or the case needs another seed."""
    inp, edm, bank, g = _inputs(dyn, nf, ctx, seed)
    want = _oracle64(sd, cfg, nf, inp, bank, keep)
    assert torch.isfinite(want).all()
    got = _run(edm, g, True, bank.stacked(), keep)
    assert edm.last_split_event is None, 'one launch per chain'
    assert torch.isfinite(got).all()
    one = _run(edm, g, False, bank.stacked(), keep)
    P.check_chain(f'{tag}: one launch vs float64 oracle', one, want, inp)
    P.check_chain(f'{tag}: join ({len(owners)} teams) vs float64 oracle', got, want, inp)
    assert torch.equal(got, _run(edm, g, True, bank.stacked(), keep)), 'bitwise repeatable'
    err = _against_one_launch(got, one, inp, owners)
    print(f'[{tag}] join vs one launch, team molecules: linker-x rel-L2 {err:.3e}')
    return got


@pytest.mark.parametrize('precision,attention', VARIANTS, ids=[f'{p_}{"-attention" if a_ else ""}' for p_, a_ in VARIANTS])
def test_join_variant_against_the_float64_oracle_and_one_launch(precision, attention):
    """Route 'join', kernel ``sample_chain_fc_kernel_join<PREC, ATT>`` with PREC = 0 / 1 / 2 for 'fp32' / 'f16x3' / 'f16x2' and ATT =
    edge attention: the 12-molecule batch, T = 24, two blocks.  Bars: ``P.check_chain`` (CHAIN_TOL = 1e-4 on the final linker
    coordinates and the other frames, exact atom types, fragments fixed) - the chain bar of tests/test_gpu_parity.py for fp32 and
    f16x3 and of tests/test_gpu_f16x2.py for f16x2; route to route the 1e-5 of ``_against_one_launch``.
    Measured figures of every case: profiles/join/README.md."""
    L = 2
    dyn, sd, cfg = _model(precision, 301 + 10 * VARIANTS.index((precision, attention)), L, ATTENTION if attention else None)
    _, owners, _ = _plan(L)
    _join_case(f'join<{precision}, attention {attention}>', dyn, sd, cfg, owners, seed=302)


def test_join_launch_of_f16x2_with_attention_is_the_f16x3_kernel():
    """'f16x2' with attention has no kernel of its own: the dispatch of dl_sample_chain_fc_join (and of every other entry point)
    takes ``<1,true>``, the kernel of 'f16x3' with attention, on the same packed weights - the same bits, on either route."""
    L = 1
    chains = {}
    for precision in ('f16x2', 'f16x3'):
        dyn, sd, cfg = _model(precision, 351, L, ATTENTION)
        inp, edm, bank, g = _inputs(dyn, NF, 1, 352)
        chains[precision] = (_run(edm, g, True, bank.stacked(), 3), _run(edm, g, False, bank.stacked(), 3))
    assert torch.isfinite(chains['f16x3'][0]).all()
    assert torch.equal(chains['f16x2'][0], chains['f16x3'][0]), 'join launch'
    assert torch.equal(chains['f16x2'][1], chains['f16x3'][1]), 'one launch'
    assert not torch.equal(chains['f16x3'][0], chains['f16x3'][1]), 'the team molecules are summed in the team order'


def test_join_launch_with_attention_tanh_and_mean_aggregation():
    """Route 'join', kernel ``<1,true>`` with all three optional hyper-parameters on (the model of
    tests/test_gpu_flags.py::test_flags_chain_vs_oracle, whose T = 10 never reaches the hand-over): same checks, same bars."""
    L = 2
    dyn, sd, cfg = _model('f16x3', 361, L, ALL_FLAGS, coord_gain=0.2)
    _, owners, _ = _plan(L)
    _join_case('join, attention + tanh + mean', dyn, sd, cfg, owners, seed=362)


def test_join_launch_off_the_released_shape(monkeypatch):
    """Route 'join' with three GCLs per block, two context channels, a 64-wide network and nine atom types: ``join_plan`` is given
    the sublayers and places the switch calls differently (call 9 instead of 10 for the 50-atom molecules); same checks."""
    from difflinker_amd import edm as edm_mod
    L, nf, ctx = 2, 9, 2
    dyn, sd, cfg = _model('f16x3', 371, L, None, nf=nf, ctx=ctx, hidden_nf=64, inv_sublayers=3)
    q_end, owners, _ = _plan(L, sublayers=3)
    assert q_end != _plan(L)[0], 'the plan follows the sublayers'
    seen = []
    plan_fn = edm_mod.join_plan
    monkeypatch.setattr(edm_mod, 'join_plan', lambda *a_, **k_: seen.append(a_[5]) or plan_fn(*a_, **k_))
    _join_case('join, 3 GCLs per block, 2 context channels, hidden 64, nf 9', dyn, sd, cfg, owners, nf=nf, ctx=ctx, seed=372)
    assert seen and set(seen) == {3}, 'EDM hands the sublayers of the model to join_plan'


@pytest.mark.parametrize('who_waits', ['owner', 'helper'])
def test_join_attention_variant_with_forced_switch_calls(monkeypatch, who_waits):
    """The plans of test_join_launch_with_forced_switch_calls on the attention kernel ``<1,true>``: every owner switches after
    its first call (the team phase of that instantiation runs for nearly the whole chain) or at its last call (for one call);
    the checks of every other variant, the float64 oracle included."""
    from difflinker_amd import edm as edm_mod
    L = 1
    dyn, sd, cfg = _model('f16x3', 381, L, ATTENTION)
    q_end, owners, helpers = _plan(L)
    forced = list(q_end)
    for o in owners:
        forced[o] = 1 if who_waits == 'owner' else T
    monkeypatch.setattr(edm_mod, 'join_plan', lambda *a_, **k_: (forced, owners, helpers))
    _join_case(f'join<f16x3, attention>, {who_waits} waits', dyn, sd, cfg, owners, seed=382, keep=3)
