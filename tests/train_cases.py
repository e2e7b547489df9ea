"""The case table of the fully-connected EGNN backward (csrc/egnn_backward.hip), shared by tests/test_train_cases_host.py (the
preconditions, on the CPU) and the GPU tests (tests/test_gpu_train.py, tests/test_gpu_train_edges.py).

A case is the inputs of ``Dynamics.parameter_grad`` - ``t, z, masks, context, G`` - with a seeded ``state_dict`` and the oracle's
``EGNNConfig``.  The four cases the backward has been held to from the start (``EXISTING``) are built exactly as before; the others
sit where the kernel's code can go wrong without those four noticing: real-atom counts around the 32-sender tile, a padded width
beyond the 256 threads of the per-atom loops, one-atom and linker-free molecules, an edge mask that is not symmetric,
``norm_constant`` of order one and zero, two atoms at one position, no context, no time channel, a wide input, three blocks and a
batch wider than the chip."""
import dataclasses
import functools

import torch

from helpers import ragged_fc_molecules, rel_l2, seeded_state_dict, trained_like_state_dict
from oracle import egnn_oracle

BAR_ALL, BAR_TENSOR = 2e-6, 1e-5        # the bars of tests/test_gpu_train.py, over all parameters and per tensor
FP32_CLASS = 2.0                        # and within 2x the error of fp32 eager autograd against the same fp64 gradient
FP32_THREADS = 8                        # threads of that fp32 run (``reference``)

DEFAULTS = dict(nf=8, ctx=1, L=1, S=2, per_mol_t=True, centering=False, trained=False, nc=1e-6, norm=100.0, coord_gain=0.02,
                condition_time=True, mask='collate', coincident=False)
_SMALL = dict(sizes=[12, 20, 7], linkers=[4, 6, 2])

CASES = {
    # the four cases of tests/test_gpu_train.py, unchanged
    'ragged': dict(sizes=[12, 20, 7], linkers=[4, 6, 2], ctx=2, L=2),
    'large': dict(sizes=[56, 110], linkers=[10, 20], S=1),
    'sub3_ctx3_centering': dict(sizes=[15, 9, 11], linkers=[5, 3, 4], nf=9, ctx=3, S=3, per_mol_t=False, centering=True),
    'sub4_trained': dict(sizes=[18, 25], linkers=[6, 8], ctx=2, L=2, S=4, trained=True),
    # real-atom counts on both sides of the 32-sender tile (TP = 32)
    'tile_32': dict(sizes=[31, 32, 33], linkers=[5, 5, 5]),
    'tile_64': dict(sizes=[63, 64, 65], linkers=[9, 9, 9]),
    'tile_32_trained_centering': dict(sizes=[31, 33], linkers=[5, 5], L=2, trained=True, centering=True, ctx=2),
    # the per-atom loops (n = tid; n < N; n += 256) wrap
    'wrap_257': dict(sizes=[257, 40], linkers=[30, 8], S=1),
    # degenerate molecules
    'tiny': dict(sizes=[1, 2, 3], linkers=[1, 1, 1]),
    'one_atom_alone': dict(sizes=[1], linkers=[1]),
    'one_fragment_atom': dict(sizes=[1, 4], linkers=[0, 2]),
    'no_linker_molecule': dict(sizes=[9, 12, 7], linkers=[3, 0, 2]),
    'no_linker_anywhere': dict(sizes=[9, 12], linkers=[0, 0]),
    # receiver and sender are told apart
    'asymmetric_mask': dict(_SMALL, mask='asymmetric'),
    # norm_constant where it weighs: the reference's EGNN default (1) and the default of Dynamics (0)
    'nc1_norm1': dict(_SMALL, L=2, nc=1.0, norm=1.0, coord_gain=1.0),
    'nc0': dict(_SMALL, nc=0.0),
    'coincident': dict(sizes=[12, 9], linkers=[4, 3], L=2, coincident=True),
    'coincident_nc0': dict(sizes=[12, 9], linkers=[4, 3], L=2, coincident=True, nc=0.0),
    # the width of the node input and every parameter offset behind it
    'no_context': dict(_SMALL, ctx=0),
    'no_time': dict(_SMALL, condition_time=False),
    'wide_input': dict(sizes=[12, 9], linkers=[4, 3], nf=16, ctx=3),         # 3 + nf = 19: beyond the kernels' state row (REFUSED)
    'wide_input_13': dict(sizes=[12, 9], linkers=[4, 3], nf=13, ctx=3),      # 3 + nf = 16, the widest row the kernels take
    'three_blocks': dict(_SMALL, L=3, S=1),
    # more molecules than compute units: the grid, the long workspace stride, the ordered reduce
    'many_small': dict(sizes=[4, 5, 3, 6] * 75, linkers=[1, 2, 1, 2] * 75),
}
# outside the scope of the HIP kernels, forward and backward (3 + in_node_nf <= 16): ``check_trainable`` says so, the oracle runs it
REFUSED = {'wide_input': 'in_node_nf=16'}
EXISTING = ('ragged', 'large', 'sub3_ctx3_centering', 'sub4_trained')
COORD_MLP = ('coord_mlp.0.weight', 'coord_mlp.0.bias', 'coord_mlp.2.weight', 'coord_mlp.2.bias', 'coord_mlp.4.weight')
# tensors whose gradient is exactly zero: with one atom coord_diff is zero, without a linker atom no coordinate moves
ZERO_COORD_MLP = ('one_atom_alone', 'no_linker_anywhere')
MASK_VALUES = (0, 0, -1, -2, 1, 3)      # 'asymmetric': drawn per (b, i, j), diagonal and padded pairs included


def spec(case):
    return {**DEFAULTS, **CASES[case]}


@dataclasses.dataclass(frozen=True)
class Inputs:
    t: torch.Tensor
    z: torch.Tensor
    nm: torch.Tensor
    lm: object            # None with centering, as the inpainting model calls the denoiser
    em: torch.Tensor      # int8 [B * N * N, 1]
    context: object       # None for context_node_nf = 0
    G: torch.Tensor
    sd: dict
    cfg: egnn_oracle.EGNNConfig
    sizes: tuple

    def args(self):
        return (self.t, self.z, self.nm, self.lm, self.em, self.context, self.G)

    @property
    def N(self):
        return self.z.shape[1]


def collated(sizes, linkers, nf, ctx, seed):
    """A collated ragged batch and its context: the fragment mask, then ``ctx - 1`` random channels (None for ``ctx = 0``)."""
    from difflinker_amd.datasets import collate
    b = collate(ragged_fc_molecules(sizes, linkers, nf, seed))
    g = torch.Generator().manual_seed(seed + 1)
    B, N = b['positions'].shape[:2]
    if ctx == 0:
        return b, None
    context = torch.cat([b['fragment_mask']] + [torch.rand(B, N, 1, generator=g) for _ in range(ctx - 1)], -1) * b['atom_mask']
    return b, context


def state_dict(s):
    wseed = 40 + s['L'] + s['S']
    sd = seeded_state_dict(s['nf'] + s['ctx'] + int(s['condition_time']), 128, s['L'], wseed, coord_gain=s['coord_gain'],
                           inv_sublayers=s['S'])
    return trained_like_state_dict(sd, wseed) if s['trained'] else sd


@functools.lru_cache(maxsize=None)
def build(case):
    s = spec(case)
    nf = s['nf']
    b, context = collated(s['sizes'], s['linkers'], nf, s['ctx'], seed=7)
    B, N = b['positions'].shape[:2]
    gen = torch.Generator().manual_seed(3)
    z = torch.cat([b['positions'], b['one_hot'] / 4], -1) + 0.5 * torch.randn(B, N, 3 + nf, generator=gen) * b['linker_mask']
    t = torch.rand(B, 1, generator=gen) if s['per_mol_t'] else torch.tensor([0.37])
    G = torch.randn(B, N, 3 + nf, generator=gen)
    em = b['edge_mask']
    if s['mask'] == 'asymmetric':
        draw = torch.randint(0, len(MASK_VALUES), (B, N, N), generator=torch.Generator().manual_seed(9))
        em = torch.tensor(MASK_VALUES, dtype=em.dtype)[draw].reshape(B * N * N, 1)
    if s['coincident']:                                  # molecule 0's fragment atoms 0 and 1 share a position
        z = z.clone()
        z[0, 1, :3] = z[0, 0, :3]
    cfg = egnn_oracle.EGNNConfig(in_node_nf=nf, context_node_nf=s['ctx'], n_layers=s['L'], inv_sublayers=s['S'],
                                 norm_constant=s['nc'], normalization_factor=s['norm'], condition_time=s['condition_time'],
                                 centering=s['centering'])
    return Inputs(t=t, z=z, nm=b['atom_mask'], lm=None if s['centering'] else b['linker_mask'], em=em, context=context, G=G,
                  sd=state_dict(s), cfg=cfg, sizes=tuple(s['sizes']))


def transposed_mask(inp):
    B, N = inp.z.shape[:2]
    return inp.em.reshape(B, N, N).transpose(1, 2).reshape(B * N * N, 1).contiguous()


def oracle_grads(inp, dtype=torch.float64):
    """Eager autograd of the oracle for ``sum(G * Dynamics.forward(...))`` in ``dtype``, per tensor of the state_dict."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in inp.sd.items()}
    d = lambda v: None if v is None else v.detach().to(dtype)                 # noqa: E731
    t, z, nm, lm, em, ctx, G = inp.args()
    out = egnn_oracle.dynamics_forward(p, inp.cfg, d(t), d(z), d(nm), d(lm), d(em), d(ctx))
    (out * d(G)).sum().backward()
    return {k: v.grad for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp64 gradient, fp32 eager gradient) of a case; computed once, read only.

    The fp32 run uses at most ``FP32_THREADS`` threads, so that its error - the yardstick of ``FP32_CLASS`` - does not depend on
    the host's core count: with 16 threads the BLAS of some hosts forms the [128, 258] weight gradients (a sum over up to 132 k
    edges) in another order and lands 2 to 7 times further from fp64 on those tensors ('large', 'tile_64', 'wrap_257': 1.3e-6
    over all parameters instead of 5.6e-7), which would loosen the criterion on those hosts only."""
    inp = build(case)
    ref = oracle_grads(inp)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(FP32_THREADS, threads))
    try:
        f32 = oracle_grads(inp, torch.float32)
    finally:
        torch.set_num_threads(threads)
    return ref, f32


def zero_tensors(ref):
    return sorted(k for k, v in ref.items() if not bool(v.any()))


def compare(got, ref):
    """rel-L2 over all parameters and the worst tensor's.  A tensor whose reference is exactly zero has no relative error: the
    callers hold it to exact zero instead (``zero_tensors``)."""
    keys = list(ref)
    a = torch.cat([got[k].double().reshape(-1) for k in keys])
    b = torch.cat([ref[k].double().reshape(-1) for k in keys])
    worst = max(rel_l2(got[k], ref[k]) for k in keys if ref[k].norm() > 0)
    return rel_l2(a, b), worst


# ---- the model under test -------------------------------------------------------------------------------------------------------
def make_dyn(inp, dev):
    from difflinker_amd import Dynamics
    c = inp.cfg
    dyn = Dynamics(n_dims=3, in_node_nf=c.in_node_nf, context_node_nf=c.context_node_nf, hidden_nf=128, n_layers=c.n_layers,
                   inv_sublayers=c.inv_sublayers, norm_constant=c.norm_constant, normalization_factor=c.normalization_factor,
                   condition_time=c.condition_time, centering=c.centering)
    dyn.load_state_dict({k: v.float() for k, v in inp.sd.items()}, strict=True)
    return dyn.to(dev)


def hip_grads(dyn, dev, t, z, nm, lm, em, ctx, G):
    g = lambda v: None if v is None else v.to(dev)                            # noqa: E731
    grads = dyn.parameter_grad(g(t), g(z), g(nm), g(lm), g(em), g(ctx), g(G))
    return {k: v.cpu() for k, v in zip([n for n, _ in dyn.named_parameters()], grads)}


# ---- one molecule of a batch, at any padded width -------------------------------------------------------------------------------
def molecule(inp, b, width=None, real=None):
    """The arguments of molecule ``b`` run alone: the first ``real`` rows (default: all ``N``), zero-padded to ``width``."""
    B, N = inp.z.shape[:2]
    real = N if real is None else real
    width = real if width is None else width

    def rows(v):
        if v is None:
            return None
        out = v.new_zeros((1, width) + tuple(v.shape[2:]))
        out[0, :real] = v[b, :real]
        return out
    em = inp.em.new_zeros(width, width)
    em[:real, :real] = inp.em.reshape(B, N, N)[b, :real, :real]
    t = inp.t[b:b + 1] if inp.t.numel() > 1 else inp.t
    return (t, rows(inp.z), rows(inp.nm), rows(inp.lm), em.reshape(width * width, 1), rows(inp.context), rows(inp.G))
