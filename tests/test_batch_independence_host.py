"""The preconditions of tests/test_gpu_batch_independence.py, asserted without a GPU: every case it runs could go wrong - its
row tiles would straddle molecules, its quad lists would start inside a neighbour's edge tile - if the kernels cut their tiles
over the whole batch (tests/independence_cases.py)."""
import pytest
import torch

import independence_cases as IC
from test_gpu_pocket_train import assert_clear_of_cutoffs


@pytest.mark.parametrize('batch', [None, 5])
@pytest.mark.parametrize('layout', list(IC.POCKET_LAYOUTS))
def test_pocket_cases_meet_their_preconditions(layout, batch):
    inp, z, t, seed = IC.pocket_case(layout, batch)
    B, N = z.shape[:2]
    assert B == (batch or 4) and inp['edge_mask'].numel() == B * N
    assert (N % 32 != 0) if layout == 'n60' else (N == 64)                                   # (a), or its deliberate absence
    assert (N + 31) // 32 == 2, 'two row tiles per molecule'
    for graph in IC.GRAPHS:
        if graph != '4A':
            assert_clear_of_cutoffs(z, inp, graph)
        assert IC.near_a_cutoff(z, inp, graph) == 0
        front = IC.quads_in_front(IC.pocket_degrees(z, inp, graph))
        print(f'{layout}, batch {B}, seed {seed}, N = {N}, {graph}: quads in front of the molecules {front.tolist()}')
        assert bool((front[1:] % 4 != 0).any())                                               # (b)
        for world, firsts in IC.shard_firsts(B).items():                                      # (c)
            assert any(int(front[b]) % 4 for b in firsts), (world, firsts, front.tolist())
    assert IC.pocket_problems(layout, inp, z) == []


def test_the_oracle_degrees_are_the_radius_graph_degrees():
    """``pocket_degrees`` against a direct count on one molecule: ligand atoms see every other ligand atom."""
    inp, z, t, _ = IC.pocket_case('n60')
    deg = IC.pocket_degrees(z, inp, 'FC-10A-4A')
    real = inp['node_mask'][..., 0] != 0
    lig = real & (inp['context'][..., -1] == 0)
    assert bool((deg[~real] == 0).all())
    assert bool((deg[lig] >= (lig.sum(1, keepdim=True) - 1).expand_as(deg)[lig]).all())
    d4 = IC.pocket_degrees(z, inp, '4A')
    x = (z[..., :3] * inp['node_mask']).double()
    want = ((torch.cdist(x, x) <= 4.0) & real[:, :, None] & real[:, None, :]).sum(-1) - real.long()
    assert torch.equal(d4, want)


@pytest.mark.parametrize('layout', list(IC.POCKET_LAYOUTS))
def test_neighbour_cases_meet_their_preconditions(layout):
    cases, seed = IC.neighbours_case(layout)
    inp, z, t, _ = IC.pocket_case(layout)
    for graph in (IC.NEIGHBOUR_GRAPH,):
        fronts = []
        for b, (im, zm, tm) in cases.items():
            assert zm.shape == z.shape and torch.equal(zm[b], z[b]) and torch.equal(tm[b], t[b])
            assert all(torch.equal(im[k][b], inp[k][b]) for k in im if k != 'edge_mask')
            assert torch.equal(im['edge_mask'], inp['edge_mask'])
            others = [k for k in range(z.shape[0]) if k != b]
            assert float(zm[others].abs().max()) > 50.0 * float(z.abs().max()), 'the neighbours are of another magnitude'
            assert IC.near_a_cutoff(zm, im, graph) == 0
            fronts.append(int(IC.quads_in_front(IC.pocket_degrees(zm, im, graph))[b]))
        print(f'{layout}, seed {seed}, {graph}: quads in front of the kept molecule {fronts}')
        assert any(f % 4 for f in fronts[1:])


def test_fully_connected_cases_meet_their_preconditions():
    for name, (sizes, linkers, _) in IC.FC_CASES.items():
        inp, z, t = IC.fc_case(name)
        B, N = z.shape[:2]
        assert N == max(sizes) and N % 32 != 0                                                # (a)
        big = IC.fc_big(inp)
        assert big.tolist() == [k for k, n in enumerate(sizes) if n > IC.FC_BIG_LIMIT] and big.numel() >= 2
        deg = IC.fc_degrees(inp)
        assert deg.sum(1).tolist() == [n * n for n in sizes], 'every pair of a molecule, the diagonal included'
        front = IC.fc_big_front(inp)
        print(f'{name}: sizes {sizes}, big {big.tolist()}, quads in front of the big ones {front.tolist()}')
        if name != 'chain':
            assert bool((front[1:] % 4 != 0).any())                                           # (b)
    # the chain's big molecules (120 atoms = 1800 quads, then 130) meet on a tile boundary: that case rests on (a) alone - the row
    # tile that would hold the last 8 rows of molecule 1 and the first 24 of molecule 3
    assert IC.fc_big_front(IC.fc_case('chain')[0]).tolist() == [0, 1800]


def test_alone_and_reversed_are_what_they_say():
    inp, z, t, _ = IC.pocket_case('n60')
    B, N = z.shape[:2]
    one = IC.alone(inp, 2)
    assert one['x'].shape[0] == 1 and torch.equal(one['edge_mask'], torch.zeros(N, dtype=inp['edge_mask'].dtype))
    assert torch.equal(one['context'][0], inp['context'][2])
    rev = IC.reversed_batch(inp)
    assert torch.equal(rev['linker_mask'][0], inp['linker_mask'][B - 1]) and torch.equal(rev['edge_mask'], inp['edge_mask'])
    fc, _, _ = IC.fc_case('mixed')
    one = IC.alone(fc, 2)
    n = fc['x'].shape[1]
    assert torch.equal(one['edge_mask'].view(n, n), fc['edge_mask'].view(3, n, n)[2])
    assert torch.equal(IC.reversed_batch(fc)['edge_mask'].view(3, n, n)[0], fc['edge_mask'].view(3, n, n)[2])
