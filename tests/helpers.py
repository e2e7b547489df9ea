"""Shared test helpers: numpy-seeded weights (reproducible without storing them), metrics."""
import contextlib
import math

import numpy as np
import torch


def dynamics_param_shapes(fin, hidden_nf, n_layers, inv_sublayers=2, prefix='dynamics', attention=False, edge_feat_nf=2):
    """(key, shape, fan_in, kind) for every tensor of the reference ``Dynamics`` state_dict
    (egnn_dynamics), in the reference's registration order (egnn.py:19-30,90-97,203-212)."""
    hn = hidden_nf
    out = []

    def lin(name, fo, fi, bias=True):
        out.append((f'{name}.weight', (fo, fi), fi, 'w'))
        if bias:
            out.append((f'{name}.bias', (fo,), fi, 'b'))

    lin(f'{prefix}.embedding', hn, fin)
    lin(f'{prefix}.embedding_out', fin, hn)
    for i in range(n_layers):
        blk = f'{prefix}.e_block_{i}'
        for j in range(inv_sublayers):
            lin(f'{blk}.gcl_{j}.edge_mlp.0', hn, 2 * hn + edge_feat_nf)
            lin(f'{blk}.gcl_{j}.edge_mlp.2', hn, hn)
            lin(f'{blk}.gcl_{j}.node_mlp.0', hn, 2 * hn)
            lin(f'{blk}.gcl_{j}.node_mlp.2', hn, hn)
            if attention:                                   # registered after node_mlp (egnn.py:42-43)
                lin(f'{blk}.gcl_{j}.att_mlp.0', 1, hn)
        lin(f'{blk}.gcl_equiv.coord_mlp.0', hn, 2 * hn + edge_feat_nf)
        lin(f'{blk}.gcl_equiv.coord_mlp.2', hn, hn)
        out.append((f'{blk}.gcl_equiv.coord_mlp.4.weight', (1, hn), hn, 'coord'))
    return out


def seeded_state_dict(fin, hidden_nf, n_layers, seed, coord_gain=0.02, inv_sublayers=2, prefix='dynamics',
                      dtype=torch.float32, attention=False, edge_feat_nf=2):
    """Weights from ``numpy.random.default_rng(seed)`` (PCG64: stable across versions), shaped
    like ``nn.Linear``'s default init (U(-1/sqrt(fan_in), 1/sqrt(fan_in))); the coordinate head
    uses xavier-uniform with ``coord_gain`` (0.001 = reference default egnn.py:90-91; 0.02 keeps
    T=500 chains finite but lively)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape, fan_in, kind in dynamics_param_shapes(fin, hidden_nf, n_layers, inv_sublayers, prefix, attention,
                                                          edge_feat_nf):
        if kind == 'coord':
            bound = coord_gain * math.sqrt(6.0 / (shape[0] + shape[1]))
        else:
            bound = 1.0 / math.sqrt(fan_in)
        sd[key] = torch.from_numpy(rng.uniform(-bound, bound, size=shape).astype(np.float32)).to(dtype)
    return sd


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def size_gnn_param_shapes(in_nf, hidden_nf, out_nf, n_layers, batch_norm=False):
    """(key, shape, fan_in, kind) of ``SizeGNN`` in ``state_dict`` order (linker_size.py:45-81; egnn.py:19-38)."""
    out = [('embedding_in.weight', (hidden_nf, in_nf), in_nf, 'w'), ('embedding_in.bias', (hidden_nf,), in_nf, 'b')]

    def gcl(pre):
        items = [(f'{pre}.edge_mlp.0.weight', (hidden_nf, 2 * hidden_nf + 1), 2 * hidden_nf + 1, 'w'),
                 (f'{pre}.edge_mlp.0.bias', (hidden_nf,), 2 * hidden_nf + 1, 'b'),
                 (f'{pre}.edge_mlp.2.weight', (hidden_nf, hidden_nf), hidden_nf, 'w'),
                 (f'{pre}.edge_mlp.2.bias', (hidden_nf,), hidden_nf, 'b'),
                 (f'{pre}.node_mlp.0.weight', (hidden_nf, 2 * hidden_nf), 2 * hidden_nf, 'w'),
                 (f'{pre}.node_mlp.0.bias', (hidden_nf,), 2 * hidden_nf, 'b')]
        second = 2
        if batch_norm:
            items += [(f'{pre}.node_mlp.1.{k}', (hidden_nf,), 0, k) for k in ('weight', 'bias', 'running_mean', 'running_var')]
            items += [(f'{pre}.node_mlp.1.num_batches_tracked', (), 0, 'count')]
            second = 3
        items += [(f'{pre}.node_mlp.{second}.weight', (hidden_nf, hidden_nf), hidden_nf, 'w'),
                  (f'{pre}.node_mlp.{second}.bias', (hidden_nf,), hidden_nf, 'b')]
        if batch_norm:
            items += [(f'{pre}.node_mlp.4.{k}', (hidden_nf,), 0, k) for k in ('weight', 'bias', 'running_mean', 'running_var')]
            items += [(f'{pre}.node_mlp.4.num_batches_tracked', (), 0, 'count')]
        return items

    out += gcl('gcl1')
    for i in range(n_layers - 1):
        out += gcl(f'gcl_layers.{i}')
    out += [('embedding_out.weight', (out_nf, hidden_nf), hidden_nf, 'w'), ('embedding_out.bias', (out_nf,), hidden_nf, 'b')]
    return out


def seeded_size_state_dict(in_nf, hidden_nf, out_nf, n_layers, seed, batch_norm=False, prefix=''):
    """``SizeGNN`` weights from ``numpy.random.default_rng(seed)``; BatchNorm statistics are non-trivial on purpose."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape, fan_in, kind in size_gnn_param_shapes(in_nf, hidden_nf, out_nf, n_layers, batch_norm):
        if kind in ('w', 'b'):
            bound = 1.0 / math.sqrt(fan_in)
            val = rng.uniform(-bound, bound, size=shape).astype(np.float32)
        elif kind == 'weight':
            val = rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
        elif kind == 'bias' or kind == 'running_mean':
            val = rng.uniform(-0.3, 0.3, size=shape).astype(np.float32)
        elif kind == 'running_var':
            val = rng.uniform(0.5, 2.0, size=shape).astype(np.float32)
        else:
            val = np.asarray(7, dtype=np.int64)
        sd[prefix + key] = torch.from_numpy(np.asarray(val))
    return sd


# ---- inputs shared by tests/golden/make_golden.py (which runs the reference on them) and the tests ----------------
def ragged_fc_molecules(sizes, linkers, nf, seed):
    """Per-molecule dicts of a ragged fully-connected batch: fragments first, the linker atoms last."""
    g = torch.Generator().manual_seed(seed)
    mols = []
    for n, nl in zip(sizes, linkers):
        frag = torch.zeros(n)
        frag[:n - nl] = 1
        types = torch.randint(0, nf, (n,), generator=g)
        mols.append({'positions': 2.0 * torch.randn((n, 3), generator=g),
                     'one_hot': torch.nn.functional.one_hot(types, nf).float(),
                     'anchors': torch.zeros(n), 'fragment_mask': frag, 'linker_mask': 1 - frag,
                     'num_atoms': n, 'uuid': 0, 'name': 'm'})
    return mols


GLUE_HPARAMS = dict(in_node_nf=8, n_dims=3, context_node_nf=1, hidden_nf=128, activation='silu', tanh=False, n_layers=1,
                    attention=False, norm_constant=1e-6, inv_sublayers=2, sin_embedding=False, normalization_factor=100,
                    aggregation_method='sum', diffusion_steps=500, diffusion_noise_schedule='polynomial_2',
                    diffusion_noise_precision=1e-5, diffusion_loss_type='l2', normalize_factors=[1, 4, 10],
                    include_charges=False, model='egnn_dynamics', data_path='d', train_data_prefix='zinc_final_train',
                    val_data_prefix='zinc_final_val', batch_size=8, lr=2e-4, torch_device='cpu', test_epochs=20,
                    n_stability_samples=10, normalization='batch_norm', anchors_context=False)


def glue_cases():
    """(tag, hparam overrides, pockets, linker sizes asked of ``sample_fn``) of the ``ddpm_glue`` fixture."""
    return [
        ('fc', {}, False, [4, 2, 6]),
        ('fc_anchors', dict(anchors_context=True, context_node_nf=2, center_of_mass='anchors'), False, [3, 5, 2]),
        ('pocket', dict(train_data_prefix='MOAD_train.full', val_data_prefix='MOAD_val.full', context_node_nf=2,
                        graph_type='FC-10A-4A', in_node_nf=9), True, [3, 4]),
        ('pocket_anchors', dict(train_data_prefix='MOAD_train.full', val_data_prefix='MOAD_val.full', context_node_nf=3,
                                anchors_context=True, in_node_nf=9), True, [2, 5]),
    ]


def glue_molecules(pockets, nf, seed):
    """Per-molecule dicts as the reference's datasets / generation scripts build them (datasets.py:56-100,
    generate_with_pocket.py:233-248): fragments first, then (pockets) the pocket atoms, then the linker."""
    g = torch.Generator().manual_seed(seed)
    mols = []
    for n_frag, n_pocket, n_link in ([(9, 14, 4), (7, 11, 3)] if pockets else [(9, 0, 4), (6, 0, 2), (11, 0, 5)]):
        n = n_frag + n_pocket + n_link
        types = torch.randint(0, nf, (n,), generator=g)
        role = torch.cat([torch.zeros(n_frag), torch.ones(n_pocket), 2 * torch.ones(n_link)])
        anchors = torch.zeros(n)
        anchors[0] = 1
        anchors[n_frag - 1] = 1
        m = {'uuid': len(mols), 'name': f'm{len(mols)}', 'positions': 2.5 * torch.randn((n, 3), generator=g),
             'one_hot': torch.nn.functional.one_hot(types, nf).float(), 'anchors': anchors,
             'fragment_mask': (role < 2).float(), 'linker_mask': (role == 2).float(), 'num_atoms': n}
        if pockets:
            m['fragment_only_mask'] = (role == 0).float()
            m['pocket_mask'] = (role == 1).float()
        mols.append(m)
    return mols




FLAG_CASES = [                       # optional hyper-parameters of Dynamics (tests/golden/fc_forward_flags.npz)
    ('attention', dict(attention=True)),
    ('tanh', dict(tanh=True)),
    ('mean', dict(aggregation_method='mean')),
    ('all', dict(attention=True, tanh=True, aggregation_method='mean')),
    ('sin', dict(sin_embedding=True)),
]


def trained_like_state_dict(sd, seed, sigma=1.5, outlier=2.0 ** 10, bias_gain=30.0):
    """Seeded-random weights reshaped towards the statistics of a TRAINED checkpoint, the regime the a-priori power-of-two
    scales of the f16x3 arithmetic have to survive: the rows of the first layer of every edge / node /
    coordinate MLP are rescaled by a log-normal factor (``sigma``), ONE row of each by ``outlier`` on top, and every bias by
    ``bias_gain``; the columns of the layer that consumes those features are divided by the same factors, so the function
    stays of order one while the hidden activations, the row-L1 norms and the bias maxima the scales are derived from spread
    over ~20 binades.  The second edge layer's rows get their own log-normal factors (no outlier), undone in the columns of
    the node MLP that read the message sum / in the coordinate head's last layer."""
    rng = np.random.default_rng(seed)
    out = {k: v.clone().double() for k, v in sd.items()}
    for k in out:
        if k.endswith('.bias'):
            out[k] *= bias_gain

    def factors(n, with_outlier):
        f = np.exp(sigma * rng.standard_normal(n))
        if with_outlier:
            f[int(rng.integers(n))] *= outlier
        return torch.from_numpy(f)
    stems = sorted({k.rsplit('.', 2)[0] for k in out if k.endswith('_mlp.0.weight')})
    for stem in stems:                                     # e.g. dynamics.e_block_0.gcl_1.edge_mlp
        if stem.endswith('att_mlp'):
            continue
        f = factors(out[f'{stem}.0.weight'].shape[0], True)
        out[f'{stem}.0.weight'] *= f[:, None]
        out[f'{stem}.0.bias'] *= f
        out[f'{stem}.2.weight'] /= f[None, :]
        if stem.endswith('edge_mlp') or stem.endswith('coord_mlp'):
            g = factors(out[f'{stem}.2.weight'].shape[0], False)
            out[f'{stem}.2.weight'] *= g[:, None]
            out[f'{stem}.2.bias'] *= g
            if stem.endswith('coord_mlp'):
                out[f'{stem}.4.weight'] /= g[None, :]
            else:                                          # SiLU sits between: undone only in magnitude, which is the point
                node0 = stem.replace('edge_mlp', 'node_mlp') + '.0.weight'
                hid = out[node0].shape[1] // 2
                out[node0][:, hid:] /= g[None, :]
    return {k: v.to(sd[k].dtype) for k, v in out.items()}


# ---- stale scratch and output memory (tests/test_gpu_scratch.py) ---------------------------------------------------------
POISON_PATTERNS = (0x00000000,      # the baseline: what a fresh process sees
                   0xFFFFFFFF,      # fp32 and fp16 NaN, int32 and int8 -1
                   0x7F7F7F7F,      # fp32 3.4e38 (finite; inf under any scale > 1), fp16 NaN, a large positive int
                   0x7F800000)      # fp32 +inf


class PoisonedAllocations:
    """What ``poisoned_allocations`` yields: ``records`` holds ``(device, nbytes, data_ptr)`` of every patched allocation."""

    def __init__(self, pattern):
        self.pattern = int(pattern) & 0xFFFFFFFF
        self.records = []

    def poisoned(self, device, at_least=1):
        """Patched allocations on ``device`` (a ``torch.device`` type such as 'cuda') of at least ``at_least`` bytes."""
        return [r for r in self.records if r[0].type == torch.device(device).type and r[1] >= at_least]


def _poison(tensor, state):
    """Fill the whole storage behind a freshly allocated tensor with the 32-bit pattern (little endian), through an int32
    view for the whole words and a uint8 view for the 1..3 bytes beyond them; record the allocation."""
    if tensor.device.type == 'meta' or tensor.is_sparse or tensor.layout != torch.strided:
        return tensor
    storage = tensor.untyped_storage()
    nbytes = storage.nbytes()
    if nbytes == 0:
        return tensor
    with torch.no_grad():
        raw = torch.tensor([], dtype=torch.uint8, device=tensor.device).set_(storage)        # every byte, whatever the dtype
        words = nbytes // 4
        signed = state.pattern - (1 << 32) if state.pattern >= (1 << 31) else state.pattern
        if words and storage.data_ptr() % 4 == 0:
            raw[:4 * words].view(torch.int32).fill_(signed)
            done = 4 * words
        else:
            done = 0
        for k in range(done, nbytes):                                       # the tail (or an unaligned buffer) byte by byte
            raw[k] = (state.pattern >> (8 * (k % 4))) & 0xFF
        if tensor.is_cuda:
            # the fill is ordered on the CURRENT stream only; the product may hand the buffer to a launch on another stream
            # (the team launch beside the main one), so it has to be over before the caller goes on: the poison goes in
            # before a launch, never while one is in flight
            torch.cuda.synchronize(tensor.device)
    state.records.append((tensor.device, nbytes, storage.data_ptr()))
    return tensor


def reset_product_caches(*objects):
    """Drop every cached workspace of the product so that the next call allocates it anew: the side-stream workspaces of
    ``difflinker_amd.edm`` (under their lock) and, for each given ``Dynamics`` / ``EDM`` (its ``dynamics``), ``_fc_ws``,
    ``_large_ws``, ``_bwd_ws`` and ``_workspaces``."""
    from difflinker_amd import edm as edm_mod
    with edm_mod._CACHE_LOCK:
        edm_mod._SIDE_WORKSPACE.clear()
    for obj in objects:
        for mod in (obj, getattr(obj, 'dynamics', None)):
            if mod is None:
                continue
            for name in ('_fc_ws', '_large_ws', '_bwd_ws'):
                if getattr(mod, name, None) is not None:
                    setattr(mod, name, None)
            if getattr(mod, '_workspaces', None):
                mod._workspaces = {}


@contextlib.contextmanager
def poisoned_allocations(pattern, monkeypatch, *objects):
    """While active, ``torch.empty``, ``torch.empty_like`` and ``Tensor.new_empty`` return tensors whose storage is filled with
    the 32-bit word ``pattern`` (sizes that are no multiple of 4 included), and every such allocation is recorded as
    ``(device, nbytes, data_ptr)`` in the yielded object's ``records``.  The product's workspace caches are dropped on entry
    (``reset_product_caches(*objects)``), so they are allocated again under the patch; build the models of a case inside the
    context, or pass them in.  ``monkeypatch`` is pytest's fixture: only attributes of ``torch`` are patched, and they are put
    back on exit (and again at the end of the test, should the body raise)."""
    state = PoisonedAllocations(pattern)
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    reset_product_caches(*objects)
    with monkeypatch.context() as patch:
        patch.setattr(torch, 'empty', lambda *a, **k: _poison(empty(*a, **k), state))
        patch.setattr(torch, 'empty_like', lambda *a, **k: _poison(empty_like(*a, **k), state))
        patch.setattr(torch.Tensor, 'new_empty', lambda self, *a, **k: _poison(new_empty(self, *a, **k), state))
        yield state
