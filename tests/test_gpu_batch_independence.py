"""Batch independence of the radius-graph kernels (csrc/egnn_sparse.hip: ``DynamicsWithPockets`` and the HBM-resident
fully-connected kernels of ``Dynamics``): the output rows of a molecule are the same BITS when it is computed alone, inside a
batch, at another position of it, next to other neighbours, or as part of a shard - and so are its sampled chain and its loss
row.  Every comparison is ``torch.equal``; the inputs and the preconditions that make them able to fail (row tiles that would
straddle molecules, quad lists that would start inside a neighbour's edge tile) are tests/independence_cases.py, asserted on
the CPU by tests/test_batch_independence_host.py.  Out of scope: the padded width ``N`` (a shard keeps it).

Before the tiles were cut per molecule (one quad scan and one row tiling over all ``B * N`` atoms) these tests failed with
rel-L2 differences of 1e-8 .. 1e-7 between the layouts; the figures are in profiles/HISTORY.md."""
import pytest
import torch

import independence_cases as IC
import test_gpu_parity as P
from helpers import rel_l2, seeded_state_dict
from oracle import edm_oracle, egnn_oracle
from oracle.egnn_oracle import EGNNConfig

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16x3', 'fp32')
CHAIN_T, CHAIN_KEEP = 8, 2


def same_bits(tag, got, want):
    """Print how far two results are apart, return whether they are the same bits."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    differ = int((got != want).sum())
    print(f'[{tag}] {differ} of {got.numel()} values differ, rel-L2 {rel_l2(got, want) if differ else 0.0:.3e}')
    return differ == 0 and torch.equal(got, want)


def pocket_dyn(graph_type, precision, n_layers=2, seed=901, **flags):
    from difflinker_amd import DynamicsWithPockets
    dyn = DynamicsWithPockets(n_dims=3, in_node_nf=IC.NF, context_node_nf=2, hidden_nf=128, n_layers=n_layers, norm_constant=1e-6,
                              normalization='batch_norm', graph_type=graph_type, **flags)
    dyn.precision = precision
    sd = seeded_state_dict(IC.NF + 3, 128, n_layers, seed, coord_gain=0.02, attention=bool(flags.get('attention')))
    dyn.load_state_dict(sd, strict=True)
    cfg = EGNNConfig(in_node_nf=IC.NF, context_node_nf=2, n_layers=n_layers, graph_type=graph_type, **flags)
    return dyn.to(P.dev()), sd, cfg


def fc_dyn(precision, seed=905):
    from difflinker_amd import Dynamics
    dyn = Dynamics(n_dims=3, in_node_nf=IC.FC_NF, context_node_nf=1, hidden_nf=128, n_layers=1, norm_constant=1e-6,
                   normalization='batch_norm')
    dyn.precision = precision
    dyn.load_state_dict(seeded_state_dict(IC.FC_NF + 2, 128, 1, seed), strict=True)
    return dyn.to(P.dev())


def on_device(inp):
    return {k: v.to(P.dev()) for k, v in inp.items()}


def each_alone_against_the_batch(tag, dyn, inp, z, t, rows=None):
    whole = P.run_hip_forward(dyn, inp, z, t)
    assert torch.isfinite(whole).all()
    ok = []
    for b in (range(z.shape[0]) if rows is None else rows):
        one = P.run_hip_forward(dyn, IC.alone(inp, b), z[b:b + 1], t[b:b + 1])
        ok.append(same_bits(f'{tag}: molecule {b} alone against row {b} of the batch', one[0], whole[b]))
    return whole, ok


# ---- one forward on the radius graph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('graph_type', IC.GRAPHS)
@pytest.mark.parametrize('layout', list(IC.POCKET_LAYOUTS))
def test_a_molecule_alone_is_its_row_of_the_batch(layout, graph_type, precision):
    """Row ``b`` of the batch forward equals the forward of molecule ``b`` alone (its ``edge_mask`` re-based to zeros), for every
    ``b``; and the batch is the oracle's at the bar of tests/test_gpu_parity.py (the kernels did not agree on something wrong)."""
    inp, z, t, _ = IC.pocket_case(layout)
    dyn, sd, cfg = pocket_dyn(graph_type, precision)
    whole, ok = each_alone_against_the_batch(f'{layout} {graph_type} {precision}', dyn, inp, z, t)
    ref = egnn_oracle.dynamics_forward_pockets(sd, cfg, t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'])
    ev, eh = P.report(f'{layout} {graph_type} {precision} against the oracle', whole, ref, z)
    assert ev <= P.FWD_TOLS[precision] and eh <= P.FWD_TOLS[precision]
    assert all(ok)


def test_a_molecule_alone_is_its_row_of_the_batch_in_the_two_term_arithmetic():
    inp, z, t, _ = IC.pocket_case('n60')
    dyn, _, _ = pocket_dyn('FC-10A-4A', 'f16x2')
    _, ok = each_alone_against_the_batch('n60 FC-10A-4A f16x2', dyn, inp, z, t)
    assert all(ok)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('layout', list(IC.POCKET_LAYOUTS))
def test_the_batch_reversed_gives_the_outputs_reversed(layout, precision):
    inp, z, t, _ = IC.pocket_case(layout)
    dyn, _, _ = pocket_dyn('FC-10A-4A', precision)
    whole = P.run_hip_forward(dyn, inp, z, t)
    back = P.run_hip_forward(dyn, IC.reversed_batch(inp), z.flip(0), t.flip(0))
    assert same_bits(f'{layout} {precision}: the batch reversed', back.flip(0), whole)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('layout', list(IC.POCKET_LAYOUTS))
def test_a_row_does_not_depend_on_what_its_neighbours_hold(layout, precision):
    """The other three molecules replaced by molecules of another seed, coordinates and features 100 times larger (other fp16
    scales in a shared tile, other degrees in front): row ``b`` is unchanged."""
    inp, z, t, _ = IC.pocket_case(layout)
    cases, _ = IC.neighbours_case(layout)
    dyn, _, _ = pocket_dyn(IC.NEIGHBOUR_GRAPH, precision)
    whole = P.run_hip_forward(dyn, inp, z, t)
    ok = []
    for b, (im, zm, tm) in cases.items():
        out = P.run_hip_forward(dyn, im, zm, tm)
        assert torch.isfinite(out).all()
        ok.append(same_bits(f'{layout} {precision}: molecule {b} among neighbours 100 times larger', out[b], whole[b]))
    assert all(ok)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_molecule_alone_is_its_row_of_the_batch_with_attention_and_mean(precision):
    """The ``ATT`` instantiation of the edge kernel and the division by the degree (``aggregation_method='mean'``)."""
    inp, z, t, _ = IC.pocket_case('n60')
    dyn, _, _ = pocket_dyn('FC-10A-4A', precision, seed=902, attention=True, aggregation_method='mean')
    _, ok = each_alone_against_the_batch(f'n60 attention + mean {precision}', dyn, inp, z, t)
    assert all(ok)


def test_a_neighbour_beyond_the_f16_range_is_reported_alone_and_moves_no_other_row():
    """Molecule 1 with its atoms 3e10 times further apart: an f16x3 scale of ITS tiles leaves the fp16 range
    (tests/test_gpu_round5.py::test_pocket_coordinates_beyond_the_f16_range_are_reported) - its flag word says so, no other
    molecule's does, and the other rows are the bits of the untouched batch.  The batch-wide maxima behind the coordinate
    pass's widening test see molecule 1 too: they decide which tiles are computed, not what a tile holds."""
    from difflinker_amd.utils import FoundNaNException
    inp, z, t, _ = IC.pocket_case('n60')
    dyn, _, _ = pocket_dyn('FC-10A-4A', 'f16x3')
    whole = P.run_hip_forward(dyn, inp, z, t)
    zz = z.clone()
    zz[1, :, :3] *= 3e10
    g = on_device(inp)
    prep = dyn.prepare(g['node_mask'], g['linker_mask'], g['edge_mask'], g['context'])
    out, flags = dyn.launch(prep, t.to(P.dev()), zz.to(P.dev()))
    torch.cuda.synchronize()
    out, flags = out.cpu(), flags.cpu().tolist()
    print('nan_flags with molecule 1 beyond the f16 range:', flags)
    assert flags[1] & 16 and [flags[b] for b in (0, 2, 3)] == [0, 0, 0]
    ok = [same_bits(f'molecule {b} beside a neighbour beyond the f16 range', out[b], whole[b]) for b in (0, 2, 3)]
    assert all(ok)
    with pytest.raises(FoundNaNException) as ei:
        P.run_hip_forward(dyn, inp, zz, t)
    assert ei.value.f16_range_idx == {1}


# ---- the HBM-resident fully-connected kernels (graph type 3) --------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', ['big', 'mixed'])
def test_a_big_molecule_alone_is_its_row_of_the_batch(case, precision):
    """Molecules beyond the LDS-resident limit: all of a batch ('big'), or the two that ``Dynamics.prepare`` gathers out of a mixed
    batch into a sub-batch of their own ('mixed') - each against itself alone."""
    inp, z, t = IC.fc_case(case)
    dyn = fc_dyn(precision)
    big = IC.fc_big(inp).tolist()
    g = on_device(inp)
    prep = dyn.prepare(g['node_mask'], g['linker_mask'], g['edge_mask'], g['context'])
    if case == 'big':
        assert prep['large'] and prep.get('split') is None
    else:
        assert [(p['large'], p['idx'].tolist()) for p in prep['split'] if p['large']] == [(True, big)]
    _, ok = each_alone_against_the_batch(f'fully connected {case} {precision}', dyn, inp, z, t, rows=big)
    assert all(ok)


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def pocket_edm(dyn):
    """The EDM of BASELINE config C5 (``timesteps=1000``) with a short chain and the counter-based noise."""
    from difflinker_amd import EDM
    edm = EDM(dyn, in_node_nf=IC.NF, n_dims=3, timesteps=1000, noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(P.dev())
    edm.T = CHAIN_T
    edm.noise_source = 'philox'
    return edm


def noise_seed_with_a_misaligned_start(edm, inp, graph_type, first_molecules):
    """The first of 5, 105, ... for which the chain's first denoiser call - on ``z_T``, known once the draws are - meets the
    preconditions: no pair on a cut-off, and one of ``first_molecules`` with a number of quads in front of it that is no
    multiple of 4."""
    B, N = inp['x'].shape[:2]
    xn, hn = edm.normalize(inp['x'], inp['h'])
    for seed in range(5, 5 + 100 * 50, 100):
        nx, nh = edm.philox_noise_bank(B, N, P.dev(), seed=seed)
        z = torch.cat([xn, hn], 2) * inp['fragment_mask'] + torch.cat([nx[0], nh[0]], 2).cpu() * inp['linker_mask']
        if IC.near_a_cutoff(z, inp, graph_type):
            continue
        front = IC.quads_in_front(IC.pocket_degrees(z, inp, graph_type))
        if all(any(int(front[b]) % 4 for b in firsts) for firsts in first_molecules):
            print(f'noise seed {seed}: quads in front of the molecules at z_T {front.tolist()}')
            return seed
    raise AssertionError('no noise seed meets the preconditions')


def shard_chain(edm, g, rank, world, seed, **kw):
    """One rank's chain the way ``sample_chain_sharded`` runs it: the slice, the global molecule index, the whole batch's
    per-step scalars and team size."""
    from difflinker_amd.distributed import shard_sampler_inputs
    local, (lo, hi) = shard_sampler_inputs(g, rank, world)
    edm.noise_seed = seed
    edm.coef_batch = edm.team_batch = g['x'].shape[0]
    try:
        if 'noise_bank' not in kw:
            kw['mol_offset'] = lo
        return edm.sample_chain(keep_frames=CHAIN_KEEP, **local, **kw).cpu()
    finally:
        edm.coef_batch = edm.team_batch = None


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('batch', list(IC.SHARDINGS))
def test_pocket_chain_shards_sample_the_bits_of_the_whole_batch(batch, precision):
    """4 molecules as 2 x 2 and 4 x 1, 5 molecules as 2 + 2 + 1: ``shard_sampler_inputs`` re-bases the batch-id ``edge_mask``, the
    host loop keys the draws by ``mol_offset``; the frames of the shards, concatenated, are the unsharded chain's."""
    from difflinker_amd.distributed import sample_chain_sharded
    inp, _, _, _ = IC.pocket_case('n60', batch)
    dyn, _, _ = pocket_dyn('FC-10A-4A', precision)
    edm = pocket_edm(dyn)
    g = on_device(inp)
    seed = noise_seed_with_a_misaligned_start(edm, inp, 'FC-10A-4A', list(IC.shard_firsts(batch).values()))
    edm.noise_seed = seed
    whole = edm.sample_chain(keep_frames=CHAIN_KEEP, **g).cpu()
    assert torch.isfinite(whole).all() and whole.shape[:2] == (CHAIN_KEEP, batch)
    assert float((whole[0, :, :, :3] * inp['linker_mask']).abs().max()) > 0
    edm.noise_seed = seed
    ok = [same_bits(f'{batch} molecules {precision}: world size 1', sample_chain_sharded(edm, g, keep_frames=CHAIN_KEEP).cpu(), whole)]
    assert edm.noise_source == 'philox' and edm.coef_batch is None and edm.team_batch is None
    for world in IC.SHARDINGS[batch]:
        parts = [shard_chain(edm, g, rank, world, seed) for rank in range(world)]
        ok.append(same_bits(f'{batch} molecules {precision}: {world} shards', torch.cat(parts, dim=1), whole))
    assert all(ok)


def test_pocket_chain_shard_with_its_draws_as_an_explicit_bank():
    """The draws of one shard as an explicit bank (``philox_noise_bank`` with the shard's ``mol_offset``): the same bits as the
    in-kernel draws, and the oracle's chain for that bank."""
    batch, rank, world = 4, 1, 2
    inp, _, _, _ = IC.pocket_case('n60', batch)
    dyn, sd, cfg = pocket_dyn('FC-10A-4A', 'f16x3')
    edm = pocket_edm(dyn)
    g = on_device(inp)
    seed = noise_seed_with_a_misaligned_start(edm, inp, 'FC-10A-4A', [[IC.shard_bounds(batch, rank, world)[0]]])
    want = shard_chain(edm, g, rank, world, seed)
    lo, hi = IC.shard_bounds(batch, rank, world)
    N = inp['x'].shape[1]
    bank = edm.philox_noise_bank(hi - lo, N, P.dev(), mol_offset=lo, seed=seed)
    edm.noise_source = 'torch'
    got = shard_chain(edm, g, rank, world, seed, noise_bank=bank)
    assert same_bits('a shard of the pocket chain: explicit bank against in-kernel draws', got, want)
    from difflinker_amd.distributed import shard_sampler_inputs
    local, _ = shard_sampler_inputs(inp, rank, world)
    orc = edm_oracle.EDMOracle(edm_oracle.make_dynamics_oracle(sd, cfg), in_node_nf=IC.NF, timesteps=1000)
    orc.T = CHAIN_T
    draws = []
    for k in range(CHAIN_T + 2):
        draws += [bank[0][k].cpu(), bank[1][k].cpu()]
    ref = orc.sample_chain(local['x'], local['h'], local['node_mask'], local['fragment_mask'], local['linker_mask'],
                           local['edge_mask'], local['context'], edm_oracle.NoiseBank(draws), keep_frames=CHAIN_KEEP)
    P.check_chain('a shard of the pocket chain against the oracle', got, ref, local)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_fully_connected_chain_with_big_molecules_is_shard_independent(precision):
    """Sizes 30, 120, 45, 130: the whole batch gathers the two big molecules into one sub-batch of the HBM-resident kernels, each
    shard of two holds one of them."""
    from difflinker_amd import EDM
    inp, _, _ = IC.fc_case('chain')
    dyn = fc_dyn(precision)
    edm = EDM(dyn, in_node_nf=IC.FC_NF, n_dims=3, timesteps=500, noise_schedule='polynomial_2', noise_precision=1e-5,
              loss_type='l2', norm_values=[1, 4, 10]).to(P.dev())
    edm.T = 4
    edm.noise_source = 'philox'
    g = on_device(inp)
    edm.noise_seed = 7
    whole = edm.sample_chain(keep_frames=CHAIN_KEEP, **g).cpu()
    assert torch.isfinite(whole).all()
    parts = [shard_chain(edm, g, rank, 2, 7) for rank in range(2)]
    got = torch.cat(parts, dim=1)
    big = IC.fc_big(inp)
    ok = [same_bits(f'fully connected chain {precision}: the big molecules', got[:, big], whole[:, big]),
          same_bits(f'fully connected chain {precision}: every molecule', got, whole)]
    assert all(ok)


# ---- loss rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_pocket_loss_rows_of_the_halves_are_those_of_the_whole_batch(precision):
    from difflinker_amd.distributed import shard_sampler_inputs
    inp, _, _, _ = IC.pocket_case('n60')
    dyn, _, _ = pocket_dyn('FC-10A-4A', precision)
    edm = pocket_edm(dyn)
    edm.T = 1000
    g = on_device(inp)

    def rows(local, lo):
        edm.noise_seed = 13
        with torch.no_grad():
            r, t_int = edm._loss_rows(local['x'], local['h'], local['node_mask'], local['fragment_mask'], local['linker_mask'],
                                      local['edge_mask'], local['context'], None, None, lo)
        return r.cpu(), t_int.cpu()
    whole, t_whole = rows(g, 0)
    assert torch.isfinite(whole).all() and len(set(t_whole.tolist())) > 1
    parts = []
    for rank in range(2):
        local, (lo, hi) = shard_sampler_inputs(g, rank, 2)
        parts.append(rows(local, lo))
    assert torch.equal(torch.cat([p[1] for p in parts]), t_whole)
    assert same_bits(f'loss rows {precision}: two halves against the whole batch', torch.cat([p[0] for p in parts]), whole)
