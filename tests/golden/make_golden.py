"""Generate the golden fixtures in this directory from the UNMODIFIED reference.

Run in the build container only (it imports /root/reference, which does not exist on the
GPU box):   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

Each fixture stores inputs + the reference's outputs; the weights are NOT stored, they are
regenerated from a numpy seed by ``tests/helpers.seeded_state_dict`` and loaded into the
reference modules here with ``load_state_dict(strict=True)``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')
sys.dont_write_bytecode = True

from src import utils as ref_utils                      # noqa: E402
from src.egnn import Dynamics, DynamicsWithPockets      # noqa: E402
from src.edm import EDM                                 # noqa: E402
from src.noise import PredefinedNoiseSchedule           # noqa: E402

from helpers import FLAG_CASES, seeded_state_dict, seeded_size_state_dict, GLUE_HPARAMS, glue_cases, glue_molecules, ragged_fc_molecules   # noqa: E402
from difflinker_amd import synthetic                    # noqa: E402
from difflinker_amd.datasets import collate             # noqa: E402


def save(name, **arrays):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name, {k: v.shape for k, v in out.items()})


def ref_dynamics(cls, nf, ctx, n_layers, graph_type, seed, coord_gain=0.02):
    dyn = cls(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, device='cpu', n_layers=n_layers,
              attention=False, tanh=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
              normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
              normalization='batch_norm', centering=False, graph_type=graph_type)
    sd = seeded_state_dict(nf + ctx + 1, 128, n_layers, seed, coord_gain=coord_gain)
    dyn.load_state_dict(sd, strict=True)
    return dyn.eval()


def gamma_tables():
    g500 = PredefinedNoiseSchedule('polynomial_2', timesteps=500, precision=1e-5).gamma.data
    g1000 = PredefinedNoiseSchedule('polynomial_2', timesteps=1000, precision=1e-5).gamma.data
    save('gamma_tables', g500=g500, g1000=g1000)


def ragged_fc_batch(sizes, linkers, nf, seed):
    return collate(ragged_fc_molecules(sizes, linkers, nf, seed))


@torch.no_grad()
def fc_forward():
    """Dynamics.forward, GEOM-like hparams, 2 blocks, ragged B=4 N=14, per-sample t."""
    nf, ctx, L = 9, 1, 2
    data = ragged_fc_batch([14, 9, 12, 5], [4, 3, 5, 2], nf, seed=11)
    inp = synthetic.sampler_inputs(data)
    g = torch.Generator().manual_seed(12)
    B, N = inp['x'].shape[:2]
    # a mid-chain state: fragments as given, linker rows noisy
    z = torch.cat([inp['x'], inp['h']], dim=2) * inp['fragment_mask'] + \
        torch.randn((B, N, 3 + nf), generator=g) * inp['linker_mask']
    t = torch.rand((B, 1), generator=g)
    dyn = ref_dynamics(Dynamics, nf, ctx, L, 'FC', seed=21)
    out = dyn.forward(t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'],
                      edge_mask=inp['edge_mask'], context=inp['context'])
    # the B=1 / scalar-t branch (egnn.py:397-399) on molecule 1, un-padded
    n1 = 9
    em1 = data['edge_mask'].view(B, N, N)[1, :n1, :n1].reshape(-1, 1)
    out1 = dyn.forward(t=t[1:2], xh=z[1:2, :n1], node_mask=inp['node_mask'][1:2, :n1],
                       linker_mask=inp['linker_mask'][1:2, :n1], edge_mask=em1, context=inp['context'][1:2, :n1])
    save('fc_forward', nf=nf, ctx=ctx, n_layers=L, weight_seed=21, coord_gain=0.02,
         t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'],
         context=inp['context'], out=out, out_mol1_unpadded=out1)


@torch.no_grad()
def fc_forward_flags():
    """Dynamics.forward with the optional hyper-parameters no released config uses (egnn.py:42-43,52-54 attention,
    :104-105 tanh, :315-319 mean aggregation, :281-292 sinusoidal distance embedding), same inputs as ``fc_forward``,
    plus a padded-width variant for 'mean' (the count is the padded width N, masked edges included)."""
    nf, ctx, L = 9, 1, 2
    data = ragged_fc_batch([14, 9, 12, 5], [4, 3, 5, 2], nf, seed=11)
    inp = synthetic.sampler_inputs(data)
    g = torch.Generator().manual_seed(12)
    B, N = inp['x'].shape[:2]
    z = torch.cat([inp['x'], inp['h']], dim=2) * inp['fragment_mask'] + \
        torch.randn((B, N, 3 + nf), generator=g) * inp['linker_mask']
    t = torch.rand((B, 1), generator=g)
    out = {}
    for tag, flags in FLAG_CASES:
        kw = dict(attention=False, tanh=False, sin_embedding=False, aggregation_method='sum')
        kw.update(flags)
        dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, device='cpu', n_layers=L,
                       norm_constant=1e-6, inv_sublayers=2, normalization_factor=100, model='egnn_dynamics',
                       normalization='batch_norm', centering=False, graph_type='FC', **kw)
        sd = seeded_state_dict(nf + ctx + 1, 128, L, 25, coord_gain=1.0 if kw['tanh'] else 0.02, attention=kw['attention'],
                               edge_feat_nf=24 if kw['sin_embedding'] else 2)
        dyn.load_state_dict(sd, strict=True)
        dyn.eval()
        out['out_' + tag] = dyn.forward(t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'],
                                        edge_mask=inp['edge_mask'], context=inp['context'])
    save('fc_forward_flags', nf=nf, ctx=ctx, n_layers=L, weight_seed=25, t=t, xh=z, node_mask=inp['node_mask'],
         linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'], context=inp['context'], **out)


@torch.no_grad()
def fc_chain():
    """EDM.sample_chain, ZINC-like hparams, 2 blocks, T=12 on a 500-entry gamma table, shared noise bank."""
    nf, ctx, L, T, keep = 8, 1, 2, 12, 3
    data = ragged_fc_batch([12, 7, 10], [4, 2, 3], nf, seed=31)
    inp = synthetic.sampler_inputs(data)
    B, N = inp['x'].shape[:2]
    g = torch.Generator().manual_seed(32)
    draws = []
    for _ in range(T + 2):
        draws.append(torch.randn((B, N, 3), generator=g))
        draws.append(torch.randn((B, N, nf), generator=g))
    pos = [0]

    def banked(size, device, node_mask):
        d = draws[pos[0]]
        assert tuple(d.shape) == tuple(size)
        pos[0] += 1
        return d * node_mask

    dyn = ref_dynamics(Dynamics, nf, ctx, L, 'FC', seed=22)
    edm = EDM(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
              noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10])
    edm.T = T                                             # generate.py:103-104
    orig = ref_utils.sample_gaussian_with_mask
    ref_utils.sample_gaussian_with_mask = banked
    try:
        chain = edm.sample_chain(x=inp['x'], h=inp['h'], node_mask=inp['node_mask'],
                                 fragment_mask=inp['fragment_mask'], linker_mask=inp['linker_mask'],
                                 edge_mask=inp['edge_mask'], context=inp['context'], keep_frames=keep)
    finally:
        ref_utils.sample_gaussian_with_mask = orig
    assert pos[0] == 2 * (T + 2)
    save('fc_chain', nf=nf, ctx=ctx, n_layers=L, T=T, keep_frames=keep, weight_seed=22, coord_gain=0.02,
         x=inp['x'], h=inp['h'], node_mask=inp['node_mask'], fragment_mask=inp['fragment_mask'],
         linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'], context=inp['context'],
         noise_x=torch.stack(draws[0::2]), noise_h=torch.stack(draws[1::2]), chain=chain)


@torch.no_grad()
def pocket_forward():
    """DynamicsWithPockets.forward, FC-10A-4A, 2 blocks, B=2 (8 fragment + 24 pocket + linker atoms)."""
    nf, ctx, L = 9, 2, 2
    mols = synthetic.pocket_molecules(2, n_frag=8, n_pocket=24, linker=(3, 6), nf=nf, seed=41)
    data = collate(mols)
    inp = synthetic.sampler_inputs(data, pockets=True)
    B, N = inp['x'].shape[:2]
    g = torch.Generator().manual_seed(42)
    z = torch.cat([inp['x'], inp['h']], dim=2) * inp['fragment_mask'] + \
        torch.cat([2.0 * torch.randn((B, N, 3), generator=g), torch.randn((B, N, nf), generator=g)], dim=2) \
        * inp['linker_mask']
    t = torch.rand((B, 1), generator=g)
    dyn = ref_dynamics(DynamicsWithPockets, nf, ctx, L, 'FC-10A-4A', seed=23)
    out = dyn.forward(t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'],
                      edge_mask=inp['edge_mask'], context=inp['context'])
    nm = inp['node_mask'].view(B * N, 1)
    x = (z.view(B * N, -1) * nm)[:, :3]
    edges = dyn.get_dist_edges(x, nm, inp['edge_mask'], inp['linker_mask'].view(B * N, 1),
                               inp['context'][..., -2].reshape(B * N, 1), inp['context'][..., -1].reshape(B * N, 1))
    save('pocket_forward', nf=nf, ctx=ctx, n_layers=L, weight_seed=23, coord_gain=0.02,
         t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'],
         context=inp['context'], out=out, edges=edges)


@torch.no_grad()
def collate_masks():
    """int8 mask semantics of the reference collate (datasets.py:366-369): ~eye on int8."""
    atom_mask = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.int8)
    edge_mask = atom_mask[:, None, :] * atom_mask[:, :, None]
    diag = ~torch.eye(4, dtype=torch.int8).unsqueeze(0)
    edge_mask *= diag
    save('collate_masks', atom_mask=atom_mask, edge_mask=edge_mask.view(-1, 1))


@torch.no_grad()
def inpainting_chain():
    """InpaintingEDM.sample_chain (src/edm.py:549-727) on a centred Dynamics, T=8 on the 500-entry gamma table, with the
    ``torch.randn`` calls of its noise helpers (utils.py:158-168,189-192) served from a bank."""
    from src.edm import InpaintingEDM
    nf, ctx, L, T, keep = 8, 1, 2, 8, 3
    data = ragged_fc_batch([12, 7, 10], [4, 2, 3], nf, seed=31)
    inp = synthetic.sampler_inputs(data)
    B, N = inp['x'].shape[:2]
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=ctx, hidden_nf=128, device='cpu', n_layers=L,
                   attention=False, tanh=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
                   normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
                   normalization='batch_norm', centering=True, graph_type='FC')
    dyn.load_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, 22, coord_gain=0.02), strict=True)
    dyn.eval()
    edm = InpaintingEDM(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
                        noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10])
    edm.T = T
    g = torch.Generator().manual_seed(32)
    draws = []
    for _ in range(1 + 2 * T + 2):                        # initial z, (p, q) per step, p and q of the decode
        draws.append(torch.randn((B, N, 3), generator=g))
        draws.append(torch.randn((B, N, nf), generator=g))
    pos = [0]
    real_randn = torch.randn

    def banked(size, device=None, **kw):
        d = draws[pos[0]]
        assert tuple(d.shape) == tuple(size)
        pos[0] += 1
        return d.clone()

    nm = inp['node_mask'].float()
    x = ref_utils.remove_mean_with_mask(inp['x'] * nm, nm)  # lightning.py:441-446: inpainting centres on all atoms
    torch.randn = banked
    try:
        chain = edm.sample_chain(x=x, h=inp['h'], node_mask=nm, edge_mask=inp['edge_mask'],
                                 fragment_mask=inp['fragment_mask'], linker_mask=inp['linker_mask'],
                                 context=inp['context'], keep_frames=keep)
    finally:
        torch.randn = real_randn
    assert pos[0] == len(draws)
    save('inpainting_chain', nf=nf, ctx=ctx, n_layers=L, T=T, keep_frames=keep, weight_seed=22, coord_gain=0.02,
         x=x, h=inp['h'], node_mask=inp['node_mask'], fragment_mask=inp['fragment_mask'],
         linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'], context=inp['context'],
         noise_x=torch.stack(draws[0::2]), noise_h=torch.stack(draws[1::2]), chain=chain)


@torch.no_grad()
def size_gnn():
    """Linker-size predictor: the unmodified ``SizeGNN`` (src/linker_size.py:45-91) driven exactly as
    ``SizeClassifier.forward`` does at inference (src/linker_size_lightning.py:83-110; that module itself needs
    pytorch_lightning, which this image lacks, so its ten lines of glue are restated here around the reference
    ``SizeGNN`` and ``coord2diff``)."""
    from src.linker_size import SizeGNN
    from src.egnn import coord2diff
    from difflinker_amd.datasets import collate_with_fragment_edges   # src/datasets.py needs rdkit (absent here)
    in_nf, hidden, out_nf = 8, 128, 10
    g = torch.Generator().manual_seed(77)
    mols = []
    for n, nl in [(12, 0), (27, 0), (9, 3), (33, 5)]:
        frag = torch.zeros(n)
        frag[:n - nl] = 1
        types = torch.randint(0, in_nf, (n,), generator=g)
        mols.append({'positions': 1.6 * torch.randn((n, 3), generator=g),
                     'one_hot': torch.nn.functional.one_hot(types, in_nf).float(),
                     'anchors': torch.zeros(n), 'fragment_mask': frag, 'linker_mask': 1 - frag,
                     'num_atoms': n, 'uuid': 0, 'name': 'm'})
    data = collate_with_fragment_edges(mols)
    out = {}
    for tag, n_layers, norm in (('plain', 3, None), ('bn', 2, 'batch_norm')):
        gnn = SizeGNN(in_node_nf=in_nf, hidden_nf=hidden, out_node_nf=out_nf, n_layers=n_layers, normalization=norm)
        gnn.load_state_dict(seeded_size_state_dict(in_nf, hidden, out_nf, n_layers, seed=500 + n_layers,
                                                   batch_norm=norm is not None), strict=True)
        gnn.eval()
        h, x = data['one_hot'], data['positions']
        fragment_mask, edge_mask, edges = data['fragment_mask'], data['edge_mask'], data['edges']
        x = x * fragment_mask
        h = h * fragment_mask
        bs, n_nodes = x.shape[0], x.shape[1]
        fm = fragment_mask.view(bs * n_nodes, 1)
        distances, _ = coord2diff(x.view(bs * n_nodes, -1), edges)
        distance_edge_mask = (edge_mask.bool() & (distances < 6)).long()
        output = gnn.forward(h.view(bs * n_nodes, -1), edges, distances, fm, distance_edge_mask)
        out['logits_' + tag] = output.view(bs, n_nodes, -1).mean(1)
        out['kept_edges_' + tag] = distance_edge_mask.sum()
    save('size_gnn', one_hot=data['one_hot'], positions=data['positions'], fragment_mask=data['fragment_mask'],
         linker_mask=data['linker_mask'], edge_mask=data['edge_mask'], **out)


@torch.no_grad()
def c1_chain():
    """BASELINE config C1 run by the reference itself: ZINC hparams (8 blocks, nf=8), B=8, N=30, ``edm.T = 50`` on the
    500-entry gamma table (generate.py:103-104), keep_frames=1.  Noise: ``oracle.edm_oracle.NoiseBank.generate`` (a
    seeded CPU generator; only the seed and a checksum are stored, the test regenerates the same bank)."""
    from oracle import edm_oracle
    nf, ctx, L, T, keep = 8, 1, 8, 50, 1
    sizes, linkers = [30, 24, 27, 29, 25, 30, 26, 28], [5, 3, 8, 4, 6, 7, 3, 5]
    data = ragged_fc_batch(sizes, linkers, nf, seed=71)
    inp = synthetic.sampler_inputs(data)
    B, N = inp['x'].shape[:2]
    bank = edm_oracle.NoiseBank.generate(T, B, N, 3, nf, seed=72)
    nx, nh = bank.stacked()
    draws = []
    for k in range(T + 2):
        draws += [nx[k], nh[k]]
    pos = [0]

    def banked(size, device, node_mask):
        d = draws[pos[0]]
        assert tuple(d.shape) == tuple(size)
        pos[0] += 1
        return d * node_mask

    dyn = ref_dynamics(Dynamics, nf, ctx, L, 'FC', seed=24, coord_gain=0.02)
    edm = EDM(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
              noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10])
    edm.T = T
    orig = ref_utils.sample_gaussian_with_mask
    ref_utils.sample_gaussian_with_mask = banked
    try:
        chain = edm.sample_chain(x=inp['x'], h=inp['h'], node_mask=inp['node_mask'],
                                 fragment_mask=inp['fragment_mask'], linker_mask=inp['linker_mask'],
                                 edge_mask=inp['edge_mask'], context=inp['context'], keep_frames=keep)
    finally:
        ref_utils.sample_gaussian_with_mask = orig
    assert pos[0] == 2 * (T + 2) and torch.isfinite(chain).all()
    save('c1_chain', nf=nf, ctx=ctx, n_layers=L, T=T, keep_frames=keep, weight_seed=24, coord_gain=0.02,
         sizes=np.array(sizes), linkers=np.array(linkers), data_seed=71, noise_seed=72,
         noise_checksum=np.array([float(nx.double().sum()), float(nh.double().sum())]), chain=chain)


C2_SLICE = 16                  # molecules 0 .. 15 of the benchmark's batch
C2_SLICE_NOISE_SEED = 5


@torch.no_grad()
def c2_slice_chain():
    """The benchmarked launch itself, pinned to the reference: molecules 0..15 of
    ``synthetic.make_batch('C2', seed=1000)`` - bench.py's batch - with bench.py's model (``torch.manual_seed(0)``, GEOM
    hparams, 6 blocks; the weights are regenerated by the test the same way), T = 500, keep_frames = 1, sampled by the
    UNMODIFIED ``src/edm.py::EDM.sample_chain``.  Noise: the in-kernel Philox stream restated on the CPU
    (``oracle/philox_oracle.normal_bank``, seed 5, global molecule index = row of the batch) and fed through the patched
    ``sample_gaussian_with_mask``.  Molecules never interact (edge_mask), so the rows a 16-molecule call produces are the rows
    the 256-molecule launch must produce.  ~10 CPU-minutes."""
    from oracle import philox_oracle
    from difflinker_amd import Dynamics as OurDynamics
    data, cfg = synthetic.make_batch('C2', seed=1000)
    full = synthetic.sampler_inputs(data)
    S = C2_SLICE
    N = full['x'].shape[1]
    inp = {k: (v.view(cfg['batch'], N * N, 1)[:S].reshape(-1, 1) if k == 'edge_mask' else v[:S]) for k, v in full.items()}
    nf, L, T = cfg['nf'], cfg['n_layers'], cfg['T']
    torch.manual_seed(0)                                      # bench.py: build_model
    ours = OurDynamics(n_dims=3, in_node_nf=nf, context_node_nf=cfg['ctx'], hidden_nf=128, n_layers=L, norm_constant=1e-6,
                       normalization='batch_norm', graph_type='FC')
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=cfg['ctx'], hidden_nf=128, device='cpu', n_layers=L,
                   attention=False, tanh=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False,
                   normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
                   normalization='batch_norm', centering=False, graph_type='FC')
    dyn.load_state_dict({k: v.detach().cpu().clone() for k, v in ours.state_dict().items()}, strict=True)
    dyn.eval()
    rx, rh = philox_oracle.normal_bank(C2_SLICE_NOISE_SEED, S, N, nf, T + 2)
    draws = []
    for k in range(T + 2):
        draws += [rx[k], rh[k]]
    pos = [0]

    def banked(size, device, node_mask):
        d = draws[pos[0]]
        assert tuple(d.shape) == tuple(size)
        pos[0] += 1
        return d * node_mask

    edm = EDM(dynamics=dyn, in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
              noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10])
    edm.T = T
    orig = ref_utils.sample_gaussian_with_mask
    ref_utils.sample_gaussian_with_mask = banked
    try:
        chain = edm.sample_chain(x=inp['x'], h=inp['h'], node_mask=inp['node_mask'],
                                 fragment_mask=inp['fragment_mask'], linker_mask=inp['linker_mask'],
                                 edge_mask=inp['edge_mask'], context=inp['context'], keep_frames=1)
    finally:
        ref_utils.sample_gaussian_with_mask = orig
    assert pos[0] == 2 * (T + 2) and torch.isfinite(chain).all()
    wsum = float(sum(v.double().abs().sum() for v in ours.state_dict().values()))
    save('c2_slice_chain', rows=S, batch_seed=1000, noise_seed=C2_SLICE_NOISE_SEED, T=T, weight_abs_sum=np.array([wsum]),
         sizes=inp['node_mask'].view(S, -1).sum(1).to(torch.int64), chain=chain)


def _stub_reference_dependencies():
    """``src/lightning.py`` and ``src/datasets.py`` import RDKit, pytorch_lightning, WandB, Biopython ... at module
    top, none of which the build image has; none of them is touched by ``collate``,
    ``create_templates_for_linker_generation`` or ``DDPM.sample_chain``.  An import hook fabricates empty stand-in
    modules for exactly those packages so the UNMODIFIED reference files import; ``pytorch_lightning.LightningModule``
    becomes a bare ``torch.nn.Module``."""
    import importlib.abc
    import importlib.machinery
    import types
    from unittest.mock import MagicMock
    roots = ('rdkit', 'wandb', 'pytorch_lightning', 'Bio', 'imageio', 'openbabel', 'networkx', 'matplotlib')

    class _Stub(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith('__'):
                raise AttributeError(name)
            m = MagicMock(name=f'{self.__name__}.{name}')
            setattr(self, name, m)
            return m

    class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        def find_spec(self, fullname, path, target=None):
            if fullname.split('.')[0] in roots:
                return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
            return None

        def create_module(self, spec):
            m = _Stub(spec.name)
            m.__path__ = []
            return m

        def exec_module(self, module):
            if module.__name__ == 'pytorch_lightning':
                class LightningModule(torch.nn.Module):
                    def save_hyperparameters(self, *a, **k):
                        pass
                module.LightningModule = LightningModule

    if not any(type(f).__name__ == '_Finder' for f in sys.meta_path):
        sys.meta_path.insert(0, _Finder())


@torch.no_grad()
def ddpm_glue():
    """The host glue of the hot path run by the UNMODIFIED reference: ``collate`` (src/datasets.py:332-375),
    ``create_templates_for_linker_generation`` (:483-512) and ``DDPM.sample_chain`` (src/lightning.py:405-463: context
    assembly with / without anchors, the pockets branch, the centre-of-mass mask selected by the dataset type) on a CPU
    ``DDPM`` with seeded weights, for the four cases of ``glue_cases``; noise from a seeded bank."""
    _stub_reference_dependencies()
    from src import datasets as ref_datasets
    from src.lightning import DDPM as RefDDPM
    from oracle import edm_oracle
    out = {}
    for tag, over, pockets, sizes in glue_cases():
        hp = dict(GLUE_HPARAMS, **over)
        nf, ctx, L, T = hp['in_node_nf'], hp['context_node_nf'], hp['n_layers'], 6
        ddpm = RefDDPM(**hp)
        ddpm.edm.dynamics.load_state_dict(seeded_state_dict(nf + ctx + 1, 128, L, 300 + len(tag), coord_gain=0.02), strict=True)
        ddpm.eval()
        ddpm.edm.T = T
        mols = glue_molecules(pockets, nf, seed=400 + len(tag))
        if pockets:
            ddpm.val_dataset = ref_datasets.MOADDataset(data=mols)       # generate_with_pocket.py:249-250
        data = ref_datasets.collate(mols)
        templ = ref_datasets.create_templates_for_linker_generation(data, torch.tensor(sizes))
        B, N = templ['positions'].shape[:2]
        bank = edm_oracle.NoiseBank.generate(T, B, N, 3, nf, seed=500 + len(tag))
        nx, nh = bank.stacked()
        draws = []
        for k in range(T + 2):
            draws += [nx[k], nh[k]]
        pos = [0]

        def banked(size, device, node_mask):
            d = draws[pos[0]]
            assert tuple(d.shape) == tuple(size)
            pos[0] += 1
            return d * node_mask

        orig = ref_utils.sample_gaussian_with_mask
        ref_utils.sample_gaussian_with_mask = banked
        try:
            chain, node_mask = ddpm.sample_chain(data, sample_fn=lambda d: torch.tensor(sizes), keep_frames=2)
        finally:
            ref_utils.sample_gaussian_with_mask = orig
        assert pos[0] == 2 * (T + 2) and torch.isfinite(chain).all()
        for k in ('positions', 'one_hot', 'anchors', 'fragment_mask', 'linker_mask', 'atom_mask', 'edge_mask') + \
                (('fragment_only_mask', 'pocket_mask') if pockets else ()):
            out[f'{tag}.collate.{k}'] = data[k]
            out[f'{tag}.template.{k}'] = templ[k]
        out[f'{tag}.chain'] = chain
        out[f'{tag}.node_mask'] = node_mask
        out[f'{tag}.noise_checksum'] = np.array([float(nx.double().sum()), float(nh.double().sum())])
    save('ddpm_glue', T=6, **out)


def xyz_writer():
    """``save_xyz_file`` of the reference (src/visualizer.py:14-31) run itself (its module imports imageio / matplotlib /
    RDKit-bound helpers at the top: stand-ins from ``_stub_reference_dependencies``): the text of the files it writes."""
    import tempfile
    _stub_reference_dependencies()
    from src.visualizer import save_xyz_file
    g = torch.Generator().manual_seed(5)
    out = {}
    for tag, nf, is_geom in (('zinc', 8, False), ('geom', 9, True)):
        B, N = 3, 7
        one_hot = torch.nn.functional.one_hot(torch.randint(0, nf, (B, N), generator=g), nf).float()
        pos = 10.0 * torch.randn((B, N, 3), generator=g)
        mask = (torch.rand((B, N, 1), generator=g) > 0.3).float()
        mask[:, 0] = 1
        with tempfile.TemporaryDirectory() as d:
            save_xyz_file(d, one_hot, pos, mask, names=[f'm{i}' for i in range(B)], is_geom=is_geom, suffix='x')
            text = [open(os.path.join(d, f'm{i}_x.xyz')).read() for i in range(B)]
        out[f'{tag}_one_hot'], out[f'{tag}_pos'], out[f'{tag}_mask'] = one_hot, pos, mask
        out[f'{tag}_text'] = np.array(text)
    save('xyz_writer', **out)


def reference_init():
    """``Dynamics`` as the reference initialises it after ``torch.manual_seed(7)`` (test_host_logic.py::
    test_same_seed_same_init_as_reference): per tensor, in registration order, its shape and the SHA-256 of its float32 bytes."""
    import hashlib
    import json
    torch.manual_seed(7)
    ref = Dynamics(n_dims=3, in_node_nf=8, context_node_nf=1, hidden_nf=128, n_layers=2, norm_constant=1e-6)
    out = [[k, list(v.shape), hashlib.sha256(v.detach().float().contiguous().numpy().tobytes()).hexdigest()]
           for k, v in ref.state_dict().items()]
    with open(os.path.join(HERE, 'reference_init_seed7.json'), 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(row) for row in out) + '\n]\n')
    print('wrote reference_init_seed7', len(out), 'tensors')


if __name__ == '__main__':
    torch.set_num_threads(8)
    if len(sys.argv) > 1:                                  # regenerate selected fixtures only
        for name in sys.argv[1:]:
            globals()[name]()
        sys.exit(0)
    c1_chain()
    ddpm_glue()
    reference_init()
    fc_forward_flags()
    xyz_writer()
    gamma_tables()
    collate_masks()
    fc_forward()
    fc_chain()
    pocket_forward()
    size_gnn()
    inpainting_chain()
    c2_slice_chain()
