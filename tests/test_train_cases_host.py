"""The preconditions of the fully-connected backward's GPU tests, on the CPU: for every case of tests/train_cases.py the fp32 eager
gradient of the oracle sits well under the bars the kernel is held to (so the reference leaves room), the cases built to bind do
bind on the oracle, and the tensors whose gradient is exactly zero are the ones each case names."""
import dataclasses

import pytest
import torch

import train_cases as TC
from helpers import rel_l2


def flat(grads):
    return torch.cat([grads[k].double().reshape(-1) for k in grads])


@pytest.mark.parametrize('case', list(TC.CASES))
def test_fp32_eager_leaves_room_under_the_bars(case):
    ref, f32 = TC.reference(case)
    total, worst = TC.compare(f32, ref)
    print(f'{case}: fp32 eager autograd against fp64: rel-L2 all {total:.2e}, worst tensor {worst:.2e}')
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert total <= TC.BAR_ALL / 2 and worst <= TC.BAR_TENSOR / 2, (total, worst)


@pytest.mark.parametrize('case', list(TC.CASES))
def test_exactly_zero_tensors_are_the_ones_the_case_names(case):
    ref, _ = TC.reference(case)
    want = []
    if case in TC.ZERO_COORD_MLP:
        want = sorted(k for k in ref if k.endswith(TC.COORD_MLP))
        assert len(want) == len(TC.COORD_MLP) * TC.build(case).cfg.n_layers
    assert TC.zero_tensors(ref) == want


def test_check_trainable_takes_every_case_but_the_too_wide_one():
    """``context_node_nf = 0`` and ``condition_time = False`` are in the backward's scope; 16 atom types are not (no kernel of the
    project takes a state row beyond 3 + 13), and the refusal names the reason."""
    from difflinker_amd import egnn
    for case in TC.CASES:
        dyn = TC.make_dyn(TC.build(case), 'cpu')
        if case in TC.REFUSED:
            with pytest.raises(NotImplementedError, match=TC.REFUSED[case]):
                egnn.check_trainable(dyn)
        else:
            egnn.check_trainable(dyn)


def test_asymmetric_mask_binds():
    inp = TC.build('asymmetric_mask')
    B, N = inp.z.shape[:2]
    em = inp.em.reshape(B, N, N)
    assert not torch.equal(em, em.transpose(1, 2))
    assert bool(torch.diagonal(em, dim1=1, dim2=2).ne(0).any())                     # live on the diagonal
    padded = (inp.nm[:, :, 0] == 0)
    assert bool(em[padded[:, :, None] | padded[:, None, :]].ne(0).any())           # and on padded pairs
    assert set(torch.unique(em).tolist()) == set(TC.MASK_VALUES)
    ref, _ = TC.reference('asymmetric_mask')
    other = TC.oracle_grads(dataclasses.replace(inp, em=TC.transposed_mask(inp)))
    diff = rel_l2(flat(other), flat(ref))
    worst = max(rel_l2(other[k], ref[k]) for k in ref)
    print(f'asymmetric mask against its transpose: rel-L2 all {diff:.2e}, worst tensor {worst:.2e}')
    assert diff > 1e-3


def test_norm_constant_binds():
    inp = TC.build('nc1_norm1')
    assert inp.cfg.norm_constant == 1.0 and inp.cfg.normalization_factor == 1.0
    ref, _ = TC.reference('nc1_norm1')
    other = TC.oracle_grads(dataclasses.replace(inp, cfg=dataclasses.replace(inp.cfg, norm_constant=1e-6)))
    diff = rel_l2(flat(other), flat(ref))
    print(f'norm_constant 1 against 1e-6: rel-L2 all {diff:.2e}')
    assert diff > 1e-4
    assert TC.build('nc0').cfg.norm_constant == 0.0


@pytest.mark.parametrize('case', ['coincident', 'coincident_nc0'])
def test_coincident_atoms_have_zero_distance(case):
    inp = TC.build(case)
    x = (inp.z[0, :, :3] * inp.nm[0]).double()
    assert inp.nm[0, 0, 0] == 1 and inp.nm[0, 1, 0] == 1 and inp.lm[0, 0, 0] == 0 and inp.lm[0, 1, 0] == 0
    assert float(((x[0] - x[1]) ** 2).sum()) == 0.0
    assert inp.em.reshape(-1, inp.N, inp.N)[0, 0, 1] != 0 and inp.em.reshape(-1, inp.N, inp.N)[0, 1, 0] != 0
    assert inp.cfg.norm_constant == (0.0 if case.endswith('nc0') else 1e-6)


def test_sizes_reach_the_mechanisms():
    assert TC.build('wrap_257').N > 256
    for case, edge in (('tile_32', 32), ('tile_64', 64), ('tile_32_trained_centering', 32)):
        sizes = TC.build(case).sizes
        assert min(sizes) < edge < max(sizes) and edge % 32 == 0, (case, sizes)
    assert 64 in TC.build('tile_64').sizes and 32 in TC.build('tile_32').sizes
    assert TC.build('tiny').sizes == (1, 2, 3) and TC.build('one_atom_alone').N == 1
    inp = TC.build('no_linker_molecule')
    assert float(inp.lm[1].sum()) == 0 and float(inp.lm[0].sum()) > 0 and float(inp.lm[2].sum()) > 0
    assert float(TC.build('no_linker_anywhere').lm.sum()) == 0
    assert TC.build('no_context').context is None and TC.build('no_context').cfg.fin == 9
    assert TC.build('no_time').cfg.fin == 9 and TC.build('wide_input').cfg.fin == 20 and TC.build('wide_input_13').cfg.fin == 17
    assert TC.build('many_small').z.shape[0] == 300


def test_existing_cases_are_unchanged():
    """The four cases the backward was held to before the table: the inputs ``tests/test_gpu_train.py`` used to build itself."""
    from difflinker_amd.datasets import collate
    from helpers import ragged_fc_molecules, seeded_state_dict
    inp = TC.build('ragged')
    b = collate(ragged_fc_molecules([12, 20, 7], [4, 6, 2], 8, 7))
    gen = torch.Generator().manual_seed(3)
    z = torch.cat([b['positions'], b['one_hot'] / 4], -1) + 0.5 * torch.randn(3, 20, 11, generator=gen) * b['linker_mask']
    t = torch.rand(3, 1, generator=gen)
    G = torch.randn(3, 20, 11, generator=gen)
    assert torch.equal(inp.z, z) and torch.equal(inp.t, t) and torch.equal(inp.G, G) and torch.equal(inp.em, b['edge_mask'])
    sd = seeded_state_dict(8 + 2 + 1, 128, 2, 44, coord_gain=0.02, inv_sublayers=2)
    assert all(torch.equal(inp.sd[k], sd[k]) for k in sd)
    assert inp.context.shape == (3, 20, 2) and torch.equal(inp.context[..., :1], b['fragment_mask'])
