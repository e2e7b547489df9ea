"""Properties of the fully-connected HIP backward (csrc/egnn_backward.hip) beyond parity with the oracle (that is
tests/test_gpu_train.py, over the cases of tests/train_cases.py): a batch's gradient is the sum of its molecules', padding changes
no bit, ``grad_out`` on rows the masks exclude is never read into a result, the width limit answers before any launch, and a
workspace that grew and was kept gives the bits of a fresh one."""
import pytest
import torch

import train_cases as TC
from helpers import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SUM_BAR = 1e-6          # a batch against the sum of its molecules: the bar of tests/test_gpu_pocket_train.py


def run(dyn, args):
    return TC.hip_grads(dyn, DEV, *args)


def flat(grads, keys):
    return torch.cat([grads[k].double().reshape(-1) for k in keys])


def assert_same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs by at most {float((a[k] - b[k]).abs().max()):.2e}'


@pytest.mark.parametrize('case', ['tile_32', 'asymmetric_mask'])
def test_batch_gradient_is_the_sum_of_its_molecules(case):
    """Each molecule alone at the batch's padded width (its own slice of the edge mask, live padded pairs included), summed in
    fp64; the batch in reverse order too - ``reduce_kernel`` adds the molecules in the order of ``b``."""
    inp = TC.build(case)
    dyn = TC.make_dyn(inp, DEV)
    B = inp.z.shape[0]
    whole = run(dyn, inp.args())
    parts = None
    for b in range(B):
        g = run(dyn, TC.molecule(inp, b))
        parts = {k: v.double() for k, v in g.items()} if parts is None else {k: parts[k] + g[k].double() for k in g}
    keys = list(whole)
    err = rel_l2(flat(whole, keys), flat(parts, keys))
    flip = lambda v: None if v is None else (v.flip(0) if v.shape[0] == B else v)                 # noqa: E731
    t, z, nm, lm, em, ctx, G = inp.args()
    N = inp.N
    back = run(dyn, (flip(t), flip(z), flip(nm), flip(lm), em.reshape(B, N, N).flip(0).reshape(B * N * N, 1), flip(ctx), flip(G)))
    err_back = rel_l2(flat(back, keys), flat(parts, keys))
    print(f'{case}: batch against the sum of its molecules: rel-L2 {err:.2e}; the batch reversed {err_back:.2e}')
    assert err <= SUM_BAR and err_back <= SUM_BAR, (err, err_back)


def test_linker_free_molecule_adds_exact_zeros_to_the_coordinate_mlp():
    """Molecule 1 of 'no_linker_molecule' has no linker atom: alone, its coordinate-MLP gradient is exactly zero (``lm = 0``
    multiplies every term), beside molecules whose gradient is not."""
    inp = TC.build('no_linker_molecule')
    dyn = TC.make_dyn(inp, DEV)
    alone = run(dyn, TC.molecule(inp, 1))
    other = run(dyn, TC.molecule(inp, 0))
    names = [k for k in alone if k.endswith(TC.COORD_MLP)]
    assert len(names) == len(TC.COORD_MLP)
    for k in names:
        assert not bool(alone[k].any()), k
        assert bool(other[k].any()), k
    assert all(bool(torch.isfinite(v).all()) for v in alone.values())
    assert any(bool(v.any()) for v in alone.values())


@pytest.mark.parametrize('b', [0, 1, 2])
def test_padding_invariance_is_exact(b):
    """A molecule of 'ragged' alone: un-padded, padded to the batch's width and padded to 300 rows (the per-atom loops wrap over
    rows that are almost all padding).  Every padded row and pair contributes an exact zero to every sum and the order of the
    real terms does not change, so the bits are the same - as the forward's ``test_padding_invariance_is_exact`` has it."""
    inp = TC.build('ragged')
    dyn = TC.make_dyn(inp, DEV)
    n = inp.sizes[b]
    bare = run(dyn, TC.molecule(inp, b, real=n))
    assert all(bool(torch.isfinite(v).all()) for v in bare.values()) and any(bool(v.any()) for v in bare.values())
    for width in (inp.N, 300):
        assert_same_bits(run(dyn, TC.molecule(inp, b, real=n, width=width)), bare, f'molecule {b} padded from {n} to {width}')


def test_grad_out_on_padded_rows_is_not_read():
    inp = TC.build('ragged')
    dyn = TC.make_dyn(inp, DEV)
    base = run(dyn, inp.args())
    padded = (inp.nm == 0).expand_as(inp.G)
    assert bool(padded.any())
    for fill in (-3.0, 1e30):
        G = torch.where(padded, torch.full_like(inp.G, fill), inp.G)
        args = inp.args()[:6] + (G,)
        assert_same_bits(run(dyn, args), base, f'grad_out = {fill} on padded rows')


def test_coordinate_grad_out_on_fragment_rows_is_not_read_under_a_linker_mask():
    """With a linker mask only linker atoms move, so the velocity of a fragment atom is zero whatever the weights are and its
    ``grad_out`` reaches no parameter.  (Centering is the exception: it spreads the mean over all real atoms.)"""
    inp = TC.build('ragged')
    assert inp.lm is not None and not inp.cfg.centering
    dyn = TC.make_dyn(inp, DEV)
    base = run(dyn, inp.args())
    frag = ((inp.nm != 0) & (inp.lm == 0)).expand(-1, -1, 3)
    assert bool(frag.any())
    G = inp.G.clone()
    G[..., :3] = torch.where(frag, -37.5 * G[..., :3], G[..., :3])
    assert not torch.equal(G, inp.G)
    assert_same_bits(run(dyn, inp.args()[:6] + (G,)), base, 'coordinate grad_out scaled on fragment rows')


def test_width_limit_raises_before_any_launch():
    from difflinker_amd import _lib
    inp = TC.build('tiny')
    dyn = TC.make_dyn(inp, DEV)
    N = int(_lib.load().dl_egnn_backward_max_atoms()) + 1
    D = 3 + inp.cfg.in_node_nf
    z = torch.zeros(1, N, D, device=DEV)
    nm = torch.zeros(1, N, 1, device=DEV)
    em = torch.zeros(N * N, 1, dtype=torch.int8, device=DEV)
    with pytest.raises(ValueError, match=f'at most {N - 1} atoms'):
        dyn.parameter_grad(torch.zeros(1, 1, device=DEV), z, nm, nm, em, nm, z)
    assert getattr(dyn, '_bwd_ws', None) is None              # not even the workspace was allocated
    assert all(bool(torch.isfinite(v).all()) for v in run(dyn, inp.args()).values())        # and the model still works


def test_workspace_grows_and_is_kept():
    """'tiny', then 'tile_64', then 'tiny' again on one model (``_bwd_ws`` grows once and is kept) against a fresh model each
    time.  The two cases share every hyper-parameter and the weights."""
    small, big = TC.build('tiny'), TC.build('tile_64')
    assert small.cfg == big.cfg and all(torch.equal(small.sd[k], big.sd[k]) for k in big.sd)
    dyn = TC.make_dyn(small, DEV)
    sizes = []
    for step, inp in enumerate((small, big, small)):
        got = run(dyn, inp.args())
        sizes.append((dyn._bwd_ws.data_ptr(), dyn._bwd_ws.numel()))
        assert_same_bits(got, run(TC.make_dyn(inp, DEV), inp.args()), f'call {step}')
    assert sizes[1][1] > sizes[0][1] and sizes[2] == sizes[1]
