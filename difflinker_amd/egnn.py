"""``Dynamics`` / ``DynamicsWithPockets`` — the denoiser boundary of DiffLinker, MI355X-native.

Drop-in for reference ``src/egnn.py::Dynamics`` (constructor egnn.py:324-329, ``forward`` :374-447):
same constructor signature, same attribute names, same ``state_dict`` keys
(``dynamics.embedding.weight`` ... ``dynamics.e_block_{i}.gcl_{j}.edge_mlp.{0,2}.{weight,bias}`` ...,
``dynamics.e_block_{i}.gcl_equiv.coord_mlp.{0,2,4}``), so a reference checkpoint loads unchanged.

The modules below only OWN the parameters (in the reference's registration order, so the same
``torch.manual_seed`` gives the same initial weights); all arithmetic of ``forward`` runs in the
hand-written HIP kernels of ``csrc/egnn_fc.hip`` through the C ABI (``include/difflinker_hip.h``).
There is no PyTorch/CPU fallback: CPU tensors, a missing HIP library or hyper-parameters outside
the HIP path raise.
"""
import ctypes
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib, utils


class TeamNotAssembled(RuntimeError):
    """Internal: a team of workgroups did not get all its members resident in time (``nan_flags`` bit 3).  Never reaches a
    caller: ``Dynamics.forward`` / ``EDM.sample_chain`` re-run the call on a path that needs no co-residency."""


class _ParamOnly(nn.Module):
    """Parameter container: its arithmetic lives in the HIP kernels."""

    def forward(self, *args, **kwargs):  # pragma: no cover
        raise RuntimeError(f'{type(self).__name__} holds parameters only; call Dynamics.forward '
                           '(HIP path, no PyTorch fallback)')


def _mlp(sizes, activation, last_activation):
    layers = []
    for k in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[k], sizes[k + 1]))
        if k < len(sizes) - 2 or last_activation:
            layers.append(activation)
    return nn.Sequential(*layers)


class GCL(_ParamOnly):
    """Edge MLP (2*nf+edges_in_d -> hidden -> hidden, activation after both) and node MLP
    (hidden+nf -> hidden -> nf; with ``normalization='batch_norm'`` a BatchNorm1d after each Linear, the layout
    the size predictor may use).  Parameters of reference ``GCL`` (egnn.py:10-43)."""

    def __init__(self, input_nf, output_nf, hidden_nf, normalization_factor, aggregation_method, activation,
                 edges_in_d=0, nodes_att_dim=0, attention=False, normalization=None):
        super().__init__()
        if nodes_att_dim:
            raise NotImplementedError('node attributes are outside the HIP path')
        self.normalization_factor = normalization_factor
        self.aggregation_method = aggregation_method
        self.attention = attention
        self.edge_mlp = _mlp([2 * input_nf + edges_in_d, hidden_nf, hidden_nf], activation, last_activation=True)
        if normalization is None:
            self.node_mlp = _mlp([hidden_nf + input_nf, hidden_nf, output_nf], activation, last_activation=False)
        elif normalization == 'batch_norm':
            self.node_mlp = nn.Sequential(nn.Linear(hidden_nf + input_nf, hidden_nf), nn.BatchNorm1d(hidden_nf),
                                          activation, nn.Linear(hidden_nf, output_nf), nn.BatchNorm1d(output_nf))
        else:
            raise NotImplementedError(normalization)
        if attention:                                              # registered last, like the reference (egnn.py:42-43)
            self.att_mlp = nn.Sequential(nn.Linear(hidden_nf, 1), nn.Sigmoid())


class EquivariantUpdate(_ParamOnly):
    """Coordinate MLP (2*hidden+edges_in_d -> hidden -> hidden -> 1, last layer bias-free with
    xavier gain 0.001).  Parameters of reference ``EquivariantUpdate`` (egnn.py:83-99)."""

    def __init__(self, hidden_nf, normalization_factor, aggregation_method, edges_in_d=1, activation=nn.SiLU(),
                 tanh=False, coords_range=10.0):
        super().__init__()
        self.tanh = tanh
        self.coords_range = coords_range
        head = nn.Linear(hidden_nf, 1, bias=False)                 # created first, like the reference
        torch.nn.init.xavier_uniform_(head.weight, gain=0.001)
        body = _mlp([2 * hidden_nf + edges_in_d, hidden_nf, hidden_nf], activation, last_activation=True)
        self.coord_mlp = nn.Sequential(*body, head)
        self.normalization_factor = normalization_factor
        self.aggregation_method = aggregation_method


class EquivariantBlock(_ParamOnly):
    """``inv_sublayers`` GCLs + one EquivariantUpdate (egnn.py:128-155)."""

    def __init__(self, hidden_nf, edge_feat_nf, activation, n_layers, norm_constant, normalization_factor,
                 aggregation_method, attention=False, tanh=False, coords_range=15.0):
        super().__init__()
        self.hidden_nf = hidden_nf
        self.n_layers = n_layers
        self.norm_constant = norm_constant
        self.coords_range_layer = float(coords_range)
        for i in range(n_layers):
            self.add_module(f'gcl_{i}', GCL(hidden_nf, hidden_nf, hidden_nf, normalization_factor,
                                            aggregation_method, activation, edges_in_d=edge_feat_nf, attention=attention))
        self.add_module('gcl_equiv', EquivariantUpdate(hidden_nf, normalization_factor, aggregation_method,
                                                       edges_in_d=edge_feat_nf, activation=activation, tanh=tanh,
                                                       coords_range=self.coords_range_layer))


class EGNN(_ParamOnly):
    """Embedding, ``n_layers`` EquivariantBlocks, output projection (egnn.py:181-216)."""

    def __init__(self, in_node_nf, hidden_nf, activation, n_layers, norm_constant, inv_sublayers,
                 normalization_factor, aggregation_method, out_node_nf=None, attention=False, tanh=False, coords_range=15,
                 sin_embedding=False):
        super().__init__()
        # SinusoidsEmbeddingNew (egnn.py:281-292) has no parameters: 6 frequencies x (sin, cos) for each of the two distances
        self.sin_embedding = bool(sin_embedding)
        edge_feat_nf = 24 if sin_embedding else 2               # egnn.py:193-198
        # the reference computes coords_range / n_layers here but hands the UNDIVIDED value to its blocks (egnn.py:192,213)
        self.coords_range_layer = float(coords_range / n_layers)
        out_node_nf = in_node_nf if out_node_nf is None else out_node_nf
        self.hidden_nf = hidden_nf
        self.n_layers = n_layers
        self.normalization_factor = normalization_factor
        self.aggregation_method = aggregation_method
        self.embedding = nn.Linear(in_node_nf, hidden_nf)
        self.embedding_out = nn.Linear(hidden_nf, out_node_nf)
        for i in range(n_layers):
            self.add_module(f'e_block_{i}', EquivariantBlock(
                hidden_nf, edge_feat_nf=edge_feat_nf, activation=activation, n_layers=inv_sublayers,
                norm_constant=norm_constant, normalization_factor=normalization_factor,
                aggregation_method=aggregation_method, attention=attention, tanh=tanh, coords_range=coords_range))


def egnn_tensor_order(n_layers, inv_sublayers=2, attention=False):
    """state_dict keys of the EGNN in the order ``dl_model_create`` expects (include/difflinker_hip.h)."""
    keys = ['embedding.weight', 'embedding.bias', 'embedding_out.weight', 'embedding_out.bias']
    for i in range(n_layers):
        for j in range(inv_sublayers):
            for mlp in ('edge_mlp', 'node_mlp'):
                for k in (0, 2):
                    keys += [f'e_block_{i}.gcl_{j}.{mlp}.{k}.weight', f'e_block_{i}.gcl_{j}.{mlp}.{k}.bias']
            if attention:
                keys += [f'e_block_{i}.gcl_{j}.att_mlp.0.weight', f'e_block_{i}.gcl_{j}.att_mlp.0.bias']
        for k in (0, 2):
            keys += [f'e_block_{i}.gcl_equiv.coord_mlp.{k}.weight', f'e_block_{i}.gcl_equiv.coord_mlp.{k}.bias']
        keys.append(f'e_block_{i}.gcl_equiv.coord_mlp.4.weight')
    return keys


HIDDEN_WIDTH = 128          # hidden_nf of the kernels (MFMA tiles of 4 x 32 features, the LDS layout of egnn_fc.hip)


def pad_to_kernel_width(key, t, hidden_nf, width=HIDDEN_WIDTH):
    """A tensor of a ``hidden_nf <= 128`` EGNN as the tensor of the 128-wide network that computes the same function: the extra
    hidden features get zero weights in and out (and zero biases), SiLU(0) = 0, so they never carry a value - every sum the
    kernels form gains exact zeros only.  ``edge_mlp.0`` / ``coord_mlp.0`` [h, 2h + e] -> [128, 256 + e] (sender block moved to
    column 128, the e distance columns to 256), ``node_mlp.0`` [h, 2h] -> [128, 256] (aggregate block to column 128)."""
    h = hidden_nf
    if h == width:
        return t.contiguous()
    if key.endswith('.bias'):
        if key.startswith('embedding_out') or 'att_mlp' in key:
            return t.contiguous()
        out = t.new_zeros(width)
        out[:h] = t
        return out
    if key == 'embedding.weight':                       # [h, fin]
        out = t.new_zeros(width, t.shape[1]); out[:h] = t; return out
    if key == 'embedding_out.weight':                   # [fin, h]
        out = t.new_zeros(t.shape[0], width); out[:, :h] = t; return out
    if key.endswith('edge_mlp.0.weight') or key.endswith('coord_mlp.0.weight'):
        e = t.shape[1] - 2 * h
        out = t.new_zeros(width, 2 * width + e)
        out[:h, :h] = t[:, :h]; out[:h, width:width + h] = t[:, h:2 * h]; out[:h, 2 * width:] = t[:, 2 * h:]
        return out
    if key.endswith('node_mlp.0.weight'):
        out = t.new_zeros(width, 2 * width)
        out[:h, :h] = t[:, :h]; out[:h, width:width + h] = t[:, h:]
        return out
    if key.endswith('att_mlp.0.weight') or key.endswith('coord_mlp.4.weight'):      # [1, h]
        out = t.new_zeros(1, width); out[:, :h] = t; return out
    assert t.shape == (h, h), (key, tuple(t.shape))     # edge_mlp.2, node_mlp.2, coord_mlp.2
    out = t.new_zeros(width, width); out[:h, :h] = t
    return out


class _HipModel:
    """Owner of one ``dl_model`` handle (packed weights in HBM of one device)."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                _lib.load().dl_model_destroy(self.handle)
        except Exception:  # pragma: no cover  (interpreter shutdown)
            pass
        self.handle = None


class Dynamics(nn.Module):
    """EGNN denoiser on the fully-connected molecular graph.  Reference: ``Dynamics`` egnn.py:323-467."""

    def __init__(
            self, n_dims, in_node_nf, context_node_nf, hidden_nf=64, device='cpu', activation=nn.SiLU(),
            n_layers=4, attention=False, condition_time=True, tanh=False, norm_constant=0, inv_sublayers=2,
            sin_embedding=False, normalization_factor=100, aggregation_method='sum', model='egnn_dynamics',
            normalization=None, centering=False, graph_type='FC',
    ):
        super().__init__()
        if model != 'egnn_dynamics':
            # reference: 'gnn_dynamics' builds a plain GNN, anything else NotImplementedError (egnn.py:355-370)
            raise NotImplementedError(f"model={model!r}: the HIP path implements 'egnn_dynamics' only")
        unsupported = []
        # attention, tanh and aggregation_method='mean' run in every kernel family (round 3: the pocket / large-molecule kernels
        # too); sin_embedding=True runs on the HBM-resident per-pass kernels only (every molecule is routed there, the fused
        # chain kernel is not used).  No released configuration uses any of them.
        if aggregation_method not in ('sum', 'mean'): unsupported.append(f'aggregation_method={aggregation_method!r}')
        if not isinstance(activation, nn.SiLU): unsupported.append(f'activation={activation!r}')
        # round 5: hidden_nf <= 128 (the reference's own default is 64) runs on the 128-wide kernels with the weights zero-padded -
        # exactly the narrower network, SiLU(0) = 0; inv_sublayers 1..4 and condition_time=False run natively
        if not 1 <= hidden_nf <= 128: unsupported.append(f'hidden_nf={hidden_nf} (the kernels are 128 wide)')
        if not 1 <= inv_sublayers <= 4: unsupported.append(f'inv_sublayers={inv_sublayers}')
        if n_dims != 3: unsupported.append(f'n_dims={n_dims}')
        if unsupported:
            raise NotImplementedError('hyper-parameters outside the HIP path (released configs use none of them): '
                                      + ', '.join(unsupported))
        self.device = device
        self.n_dims = n_dims
        self.in_node_nf = in_node_nf                   # atom-type channels (before time/context are appended)
        self.context_node_nf = context_node_nf
        self.condition_time = condition_time
        self.model = model
        self.centering = centering
        self.graph_type = graph_type
        self.norm_constant = norm_constant
        self.normalization_factor = normalization_factor
        self.attention, self.tanh, self.aggregation_method = bool(attention), bool(tanh), aggregation_method
        self.sin_embedding = bool(sin_embedding)
        # `normalization` (batch_norm in the YAMLs) is only forwarded to the GNN branch by the reference
        # (egnn.py:341-368): a no-op for egnn_dynamics, accepted and ignored here too.
        self.dynamics = EGNN(
            in_node_nf=in_node_nf + context_node_nf + int(condition_time), hidden_nf=hidden_nf,
            activation=activation, n_layers=n_layers, norm_constant=norm_constant, inv_sublayers=inv_sublayers,
            normalization_factor=normalization_factor, aggregation_method=aggregation_method, attention=attention,
            tanh=tanh, sin_embedding=sin_embedding)
        self.n_layers = n_layers
        self.inv_sublayers = inv_sublayers
        self.edge_cache = {}                           # kept for attribute parity; the kernels need no edge list
        self._hip_models = {}                          # device index -> (_HipModel, weight version)
        # arithmetic of the 128-wide GEMMs (not a reference hyper-parameter): 'f16x3' = scaled split-fp16 on the
        # matrix cores (default, fp32-class: 2..5e-7 rel-L2 on the node features of a forward), 'fp32' = exact fp32 MFMA,
        # 'f16x2' (opt-in, round 4) = f16x3 except the second layer of the GCL edge model, whose input enters as one fp16 rounded
        # to nearest (two MFMA terms instead of three: +9..11 % molecules/s; node features 3..9e-6 rel-L2 per forward, velocities
        # and sampled coordinates as f16x3 - inside the 1e-4 bar, not fp32-class; include/difflinker_hip.h).
        self.precision = os.environ.get('DIFFLINKER_PRECISION', 'f16x3')
        # compute units per molecule on the LDS-resident path (not a reference hyper-parameter): 'auto' = as many (1, 2,
        # 4 or 8) as keep the whole chip busy for the batch at hand - the reference's default sampling batch of 64
        # (generate.py:145) would otherwise light a quarter of it; 1 / 2 / 4 / 8 = fixed.  Samples agree across team sizes to
        # fp32 rounding (an atom's messages are summed in a team-size dependent order) and are bitwise repeatable for a
        # given one: pin it when a batch must give identical bits however it is split.
        self.team = os.environ.get('DIFFLINKER_TEAM', 'auto')
        self._fc_ws = None
        self._team_auto = {}
        self._no_teams = False                         # set while a call is re-run after a team failed to assemble
        # batch size the 'auto' team size is chosen for when it is larger than the batch at hand (None: the batch at hand):
        # EDM.sample_chain sets it to the size of the whole - possibly sharded - batch for the denoiser calls of a host-driven
        # chain, so that a sample does not depend on how the batch was split (the fused chain does the same through EDM.team_batch)
        self.team_batch = None

    # ---- packed weights -----------------------------------------------------------------------------
    def _weight_version(self):
        return (self.precision,) + tuple(p._version for p in self.dynamics.parameters()) + \
            tuple(p.data_ptr() for p in self.dynamics.parameters())

    def invalidate_packed(self):
        self._hip_models.clear()

    def _apply(self, fn, *args, **kwargs):
        self._hip_models.clear()
        return super()._apply(fn, *args, **kwargs)

    def hip_config(self):
        return _lib.DLConfig(n_dims=self.n_dims, in_node_nf=self.in_node_nf, context_node_nf=self.context_node_nf,
                             hidden_nf=HIDDEN_WIDTH, n_layers=self.n_layers, inv_sublayers=int(self.inv_sublayers),
                             condition_time=int(bool(self.condition_time)), norm_constant=float(self.norm_constant),
                             normalization_factor=float(self.normalization_factor),
                             precision=_lib.PRECISIONS[self.precision], attention=int(self.attention), tanh=int(self.tanh),
                             coords_range=15.0, aggregation_mean=int(self.aggregation_method == 'mean'),
                             sin_embedding=int(self.sin_embedding))

    def hip_model(self, device):
        """``dl_model`` handle for ``device`` (packs + uploads the weights on first use / after a change)."""
        if device.type != 'cuda':
            raise RuntimeError('difflinker_amd.Dynamics runs on the GPU only (HIP kernels, no CPU fallback); '
                               f'got tensors on {device}')
        lib = _lib.load()
        index = device.index if device.index is not None else torch.cuda.current_device()
        version = self._weight_version()
        cached = self._hip_models.get(index)
        if cached is not None and cached[1] == version:
            return cached[0].handle
        sd = self.dynamics.state_dict()
        host = [pad_to_kernel_width(k, sd[k].detach().to('cpu', torch.float32), self.dynamics.hidden_nf)
                for k in egnn_tensor_order(self.n_layers, inv_sublayers=self.inv_sublayers, attention=self.attention)]
        cfg = self.hip_config()
        assert lib.dl_model_num_tensors(ctypes.byref(cfg)) == len(host)
        arr = (ctypes.c_void_p * len(host))(*[t.data_ptr() for t in host])
        handle = ctypes.c_void_p()
        with torch.cuda.device(index):
            _lib.check(lib.dl_model_create(ctypes.byref(cfg), arr, len(host), ctypes.byref(handle)),
                       'dl_model_create')
        self._hip_models[index] = (_HipModel(handle), version)
        return handle

    # ---- forward ------------------------------------------------------------------------------------
    @staticmethod
    def _f32(t):
        return None if t is None else t.to(torch.float32).contiguous()

    def _flags(self):
        return self.attention or self.tanh or self.aggregation_method != 'sum'

    def fits_lds(self, node_mask):
        """True when every molecule fits the LDS-resident kernels: <= ``dl_max_atoms()`` real atoms on one compute unit, <=
        ``dl_team_max_atoms(2)`` on a team of them.  Bigger ones run on the HBM-resident per-pass kernels
        (``dl_egnn_forward_fc_large``): same numbers, several times slower."""
        n_nodes = node_mask.shape[1]
        limit = self._atom_limit()
        return n_nodes <= limit or int(node_mask.reshape(node_mask.shape[0], n_nodes).ne(0).sum(1).max()) <= limit

    def _atom_limit(self):
        lib = _lib.load()
        return int(lib.dl_max_atoms()) if self._no_teams else int(lib.dl_team_max_atoms(2))

    def size_classes(self, nm):
        """Index tensors (small, medium, big) of a batch by real-atom count: one compute unit per molecule possible / a team
        needed / beyond the LDS-resident kernels.  ``None`` for an empty class; no host sync when the padded width already
        says 'all small'."""
        lim1 = int(_lib.load().dl_max_atoms())
        if nm.shape[1] <= lim1:
            return None, None, None                     # every molecule is small: the whole batch, no index tensors
        sizes = nm.ne(0).sum(1)
        lim2 = self._atom_limit()
        small, big = sizes <= lim1, sizes > lim2
        med = ~small & ~big
        pick = lambda m: torch.nonzero(m).flatten() if bool(m.any()) else None      # noqa: E731
        return pick(small), pick(med), pick(big)

    def team_chunks(self, idx, device):
        """Molecules that need a team (more atoms than one compute unit holds): pieces of the batch small enough for teams of
        at least two workgroups to be resident at once."""
        cap = int(idx.numel())
        while int(self.team_for_size(cap, device)) < 2 and cap > 8:
            cap = (cap + 1) // 2
        return [idx[k:k + cap] for k in range(0, int(idx.numel()), cap)]

    def team_for_size(self, batch_size, device):
        """``dl_team_max`` for a batch size on ``device`` (cached)."""
        saved, self.team = self.team, 'auto'
        try:
            return self.team_for(batch_size, device)
        finally:
            self.team = saved

    def prepare(self, node_mask, linker_mask, edge_mask, context):
        """Everything of a call that does not change along a sampling chain (mask conversions, the size check that picks
        the kernel family); ``launch`` then only enqueues kernels."""
        dev = node_mask.device
        bs, n_nodes = node_mask.shape[0], node_mask.shape[1]
        prep = dict(bs=bs, n=n_nodes, dev=dev, large=False, team=None, handle=self.hip_model(dev),
                    nm=node_mask.reshape(bs, n_nodes).to(torch.int8).contiguous(),
                    lm=self._f32(linker_mask.reshape(bs, n_nodes)) if linker_mask is not None else None,
                    em=edge_mask.reshape(bs, n_nodes, n_nodes).to(torch.int8).contiguous() if edge_mask is not None else None,
                    ctx=self._f32(context.reshape(bs, n_nodes, self.context_node_nf)) if context is not None else None,
                    node_mask3=node_mask.reshape(bs, n_nodes, 1))
        if type(self) is not Dynamics:
            return prep
        if self.sin_embedding:                                     # HBM-resident kernels for every molecule
            prep['large'] = True
            return prep
        small, med, big = self.size_classes(prep['nm'])
        if small is None and med is None and big is None:
            return prep

        def part(idx, large, team=None):
            sub = {k: (v[idx].contiguous() if torch.is_tensor(v) else v) for k, v in prep.items()}
            sub.update(bs=int(idx.numel()), large=large, idx=idx, team=team)
            return sub
        parts = []
        if small is not None:
            parts.append(part(small, False))
        if med is not None:                                        # a team per molecule, at least two workgroups
            for chunk in self.team_chunks(med, dev):
                parts.append(part(chunk, False, team=max(2, self.team_for_size(max(int(chunk.numel()), int(self.team_batch or 0)), dev))))
        if big is not None:
            parts.append(part(big, True))
        if len(parts) == 1 and parts[0]['bs'] == bs:               # one class only: no scatter needed
            prep.update(large=parts[0]['large'], team=parts[0]['team'])
        else:
            prep['split'] = parts
        return prep

    def launch(self, prep, t, xh, center=True):
        """Enqueue one denoiser call for prepared masks; returns ``(eps_hat, nan_flags)`` without synchronising.
        ``center=False`` skips the centring of a ``centering=True`` denoiser (callers that fuse it into their own tail)."""
        out, flags = self._launch_forward(t, xh, None, None, None, None, large=prep['large'], prep=prep)
        if self.centering and center:                          # inpainting only (egnn.py:444-445)
            out = self._center_velocity(out, prep['node_mask3'])
        return out, flags

    def _center_velocity(self, out, node_mask3):
        """``remove_mean_with_mask`` on the velocity part (egnn.py:444-445, utils.py:56-63) without the reference's
        masking assert, whose ``.item()`` would synchronise the host once per reverse step."""
        nm = node_mask3.to(out.dtype)
        vel = out[:, :, :self.n_dims]
        vel = vel - (vel.sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm
        return torch.cat([vel, out[:, :, self.n_dims:]], dim=2)

    def _launch_forward(self, t, xh, node_mask, linker_mask, edge_mask, context, large=False, prep=None):
        lib = _lib.load()
        dev = xh.device
        bs, n_nodes = xh.shape[0], xh.shape[1]
        if prep is not None and prep.get('split') is not None:     # molecules of several size classes
            out = torch.zeros_like(self._f32(xh))
            flags = torch.zeros(bs, dtype=torch.int32, device=dev)
            t_rows = t.to(dev).reshape(-1) if torch.is_tensor(t) and t.numel() == bs and bs > 1 else None
            for sub in prep['split']:
                o, f = self._launch_forward(t if t_rows is None else t_rows[sub['idx']], xh[sub['idx']], None, None, None, None,
                                            large=sub['large'], prep=sub)
                out[sub['idx']] = o
                flags[sub['idx']] = f
            return out, flags
        handle = prep['handle'] if prep is not None else self.hip_model(dev)   # a chain packs / looks up the weights once
        xh = self._f32(xh)
        if not torch.is_tensor(t):
            t = torch.tensor([float(t)])
        t = t.to(dev, torch.float32).contiguous().view(-1)
        t_is_scalar = int(t.numel() == 1)                       # egnn.py:397-399
        assert t_is_scalar or t.numel() == bs
        if prep is not None:
            nm, lm, em, ctx = prep['nm'], prep['lm'], prep['em'], prep['ctx']
        else:
            nm = node_mask.reshape(bs, n_nodes).to(torch.int8).contiguous()
            lm = self._f32(linker_mask.reshape(bs, n_nodes)) if linker_mask is not None else None
            em = edge_mask.reshape(bs, n_nodes, n_nodes).to(torch.int8).contiguous() if edge_mask is not None else None
            ctx = self._f32(context.reshape(bs, n_nodes, self.context_node_nf)) if context is not None else None
        out = torch.empty_like(xh)
        flags = torch.empty(bs, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if not large:
                team = prep.get('team') if prep is not None else None
                if team is None:
                    team = 1 if self._no_teams else self.team_for(max(bs, int(self.team_batch or 0)), dev)
                ws, need = self.workspace(bs, team, dev)
                _lib.check(lib.dl_egnn_forward_fc_team(handle, bs, n_nodes, _lib.ptr(xh), _lib.ptr(t), t_is_scalar,
                                                       _lib.ptr(nm), _lib.ptr(lm), _lib.ptr(em), _lib.ptr(ctx),
                                                       _lib.ptr(out), _lib.ptr(flags), team, _lib.ptr(ws), need,
                                                       ctypes.c_void_p(stream)), 'dl_egnn_forward_fc_team')
            else:
                if em is None:
                    raise ValueError('the HBM-resident kernels (molecules beyond the LDS-resident limit, sin_embedding) need edge_mask')
                need = int(lib.dl_pocket_workspace_bytes(bs, n_nodes))
                ws = getattr(self, '_large_ws', None)
                if ws is None or ws.numel() < need or ws.device != dev:
                    ws = self._large_ws = torch.empty(need, dtype=torch.uint8, device=dev)
                _lib.check(lib.dl_egnn_forward_fc_large(handle, bs, n_nodes, _lib.ptr(xh), _lib.ptr(t), t_is_scalar,
                                                        _lib.ptr(nm), _lib.ptr(lm), _lib.ptr(em), _lib.ptr(ctx),
                                                        _lib.ptr(out), _lib.ptr(flags), _lib.ptr(ws), need,
                                                        ctypes.c_void_p(stream)), 'dl_egnn_forward_fc_large')
        return out, flags

    def team_for(self, batch_size, device=None):
        """Workgroups (compute units) per molecule for a batch of ``batch_size``: ``self.team``, 'auto' = ``dl_team_max``
        (a property of the device: asked once per device and batch size)."""
        if self.team in ('auto', None):
            if device is not None and device.index is not None:
                index = device.index
            else:
                index = torch.cuda.current_device() if torch.cuda.is_available() else -1
            key = (index, int(batch_size))
            if key not in self._team_auto:
                if index >= 0:
                    with torch.cuda.device(index):
                        self._team_auto[key] = int(_lib.load().dl_team_max(int(batch_size)))
                else:                                              # no device: a query, answers 1
                    self._team_auto[key] = int(_lib.load().dl_team_max(int(batch_size)))
            return self._team_auto[key]
        team = int(self.team)
        if team not in (1, 2, 4, 8):
            raise ValueError(f'Dynamics.team must be "auto", 1, 2, 4 or 8, not {self.team!r}')
        return team

    def workspace(self, batch_size, team, device):
        """Caller-owned scratch of the fully-connected entry points (``dl_workspace_bytes``), cached per model; launches of
        one model are ordered on the current stream, so one buffer serves them all."""
        need = int(_lib.load().dl_workspace_bytes(int(batch_size), int(team)))
        ws = self._fc_ws
        if ws is None or ws.numel() < need or ws.device != device:
            ws = self._fc_ws = torch.empty(need, dtype=torch.uint8, device=device)
        return ws, need

    def _raise_on_flags(self, flags):
        """One D2H sync per forward, like the reference's ``torch.any(torch.isnan(..))`` (egnn.py:441-442)."""
        if bool(flags.any()):
            f = flags.cpu()
            if bool((f & 8).any()):
                raise TeamNotAssembled('a team of workgroups did not assemble in time (another kernel held compute units)')
            if bool((f & 4).any()):
                raise ValueError('molecule with more real atoms than the LDS-resident fully-connected kernels take '
                                 f'({_lib.load().dl_max_atoms()} on one compute unit, {_lib.load().dl_team_max_atoms(2)} on a team)')
            raise utils.FoundNaNException.from_flags(f)

    def without_teams(self, fn):
        """Run ``fn()``; if a team of workgroups could not assemble (another kernel held compute units for seconds), run it
        once more with one compute unit per molecule (molecules that need a team: on the HBM-resident kernels) - the
        reference's callers catch ``FoundNaNException`` only (generate.py:154-161), nothing else may reach them."""
        try:
            return fn()
        except TeamNotAssembled:
            # (said once per occurrence: the re-run doubles the cost of the call - ADVICE round 5)
            warnings.warn('a team of workgroups did not assemble in time (another kernel held compute units, or a launch queued behind '
                          'a long one outlived the bounded wait): the call is re-run with one compute unit per molecule, from the same '
                          'draws', RuntimeWarning, stacklevel=2)
            saved, self._no_teams = self._no_teams, True
            try:
                return fn()
            finally:
                self._no_teams = saved

    def forward(self, t, xh, node_mask, linker_mask, edge_mask, context):
        """
        - t: (B, 1), (B) or a single value  - xh: (B, N, 3 + nf)     - node_mask: (B, N, 1) or (B, N)
        - linker_mask: (B, N, 1), (B, N) or None  - edge_mask: (B*N*N, 1) or (B, N, N), int8 {0,-1,-2}  - context: (B, N, C)
        Any strides, storage offset and real or bool dtype whose values are exact in fp32 / int8.
        Returns eps_hat (B, N, 3 + nf) = cat[vel, h_final]; raises ``utils.FoundNaNException``.
        """
        assert self.graph_type == 'FC'
        if xh.shape[0] == 0:                       # an empty batch: the reference's empty edge list gives an empty output (egnn.py:449-464)
            return torch.zeros_like(xh)

        def run():
            prep = self.prepare(node_mask, linker_mask, edge_mask, context)
            out, flags = self._launch_forward(t, xh, None, None, None, None, large=prep['large'], prep=prep)
            self._raise_on_flags(flags)
            return out
        out = self.without_teams(run)
        if self.centering:                                     # inpainting only (egnn.py:444-445)
            nm = node_mask.reshape(xh.shape[0], xh.shape[1], 1).to(out.dtype)
            vel = utils.remove_mean_with_mask(out[:, :, :self.n_dims], nm)
            out = torch.cat([vel, out[:, :, self.n_dims:]], dim=2)
        return out

    def get_edges(self, n_nodes, batch_size):
        """Fully-connected edge list ``e = b*N*N + i*N + j`` (egnn.py:449-467).  Not used by the
        kernels (pairs are enumerated by index arithmetic on chip); kept for API parity."""
        cache = self.edge_cache.setdefault(n_nodes, {})
        if batch_size not in cache:
            e = torch.arange(batch_size * n_nodes * n_nodes)
            b, i, j = e // (n_nodes * n_nodes), (e // n_nodes) % n_nodes, e % n_nodes
            cache[batch_size] = [(b * n_nodes + i).to(self.device), (b * n_nodes + j).to(self.device)]
        return cache[batch_size]


class DynamicsWithPockets(Dynamics):
    """Pocket-conditioned denoiser on the radius graph.  Reference: ``DynamicsWithPockets`` egnn.py:470-596.

    ``edge_mask`` is the per-node batch-index vector ``[B*N]`` of the pockets' ``collate`` (datasets.py:359-364);
    the last two context channels are the fragment-only / pocket-only masks.  The graph (ligand-ligand fully
    connected, pocket-pocket <= 4 A, ligand-pocket <= 10 A or 4 A) is rebuilt on the GPU every call and the EGNN
    runs without an edge mask.  Same arithmetic modes as ``Dynamics`` (``precision`` = 'f16x3' | 'fp32' | 'f16x2')."""

    GRAPH_TYPES = {'4A': 0, 'FC-4A': 1, 'FC-10A-4A': 2}

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._workspaces = {}

    def prepare(self, node_mask, linker_mask, edge_mask, context):
        """Everything of a call that does not change along a sampling chain: mask conversions, the reference's role
        assert (egnn.py:488), the batch-index check, the workspace.  ``launch`` then only enqueues kernels."""
        assert self.graph_type in ['4A', 'FC-4A', 'FC-10A-4A']
        lib = _lib.load()
        dev = node_mask.device
        bs, n_nodes = node_mask.shape[0], node_mask.shape[1]
        nm = node_mask.reshape(bs, n_nodes).to(torch.int8).contiguous()
        lm = self._f32(linker_mask.reshape(bs, n_nodes))
        ctx = self._f32(context.reshape(bs, n_nodes, self.context_node_nf))
        # frag-only | pocket-only | linker == node_mask, like the reference's assert (egnn.py:488)
        roles = (ctx[..., -2] != 0) | (ctx[..., -1] != 0) | (lm != 0)
        assert bool(torch.all(roles == (nm != 0))), 'fragment/pocket/linker masks do not cover node_mask'
        if edge_mask is not None:
            want = torch.arange(bs, device=dev, dtype=edge_mask.dtype).repeat_interleave(n_nodes)
            assert edge_mask.numel() == bs * n_nodes and bool(torch.all(edge_mask.view(-1) == want)), \
                'edge_mask must be the positional batch-index vector of collate (datasets.py:359-364)'
        need = int(lib.dl_pocket_workspace_bytes(bs, n_nodes))
        key = (dev.index, bs, n_nodes)
        ws = self._workspaces.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._workspaces = {key: ws}
        return dict(bs=bs, n=n_nodes, nm=nm, lm=lm, ctx=ctx, ws=ws, need=need, handle=self.hip_model(dev), dev=dev,
                    node_mask3=node_mask.reshape(bs, n_nodes, 1))

    def launch(self, prep, t, xh, center=True):
        """Enqueue one denoiser call for prepared masks; returns ``(eps_hat, nan_flags)`` without synchronising."""
        lib = _lib.load()
        dev, bs, n_nodes = prep['dev'], prep['bs'], prep['n']
        xh = self._f32(xh)
        if not torch.is_tensor(t):
            t = torch.tensor([float(t)])
        t = t.to(dev, torch.float32).contiguous().view(-1)
        t_is_scalar = int(t.numel() == 1)
        out = torch.empty_like(xh)
        flags = torch.empty(bs, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.dl_egnn_forward_pocket(
                prep['handle'], bs, n_nodes, self.GRAPH_TYPES[self.graph_type], _lib.ptr(xh), _lib.ptr(t), t_is_scalar,
                _lib.ptr(prep['nm']), _lib.ptr(prep['lm']), _lib.ptr(prep['ctx']), _lib.ptr(out), _lib.ptr(flags),
                _lib.ptr(prep['ws']), prep['need'], ctypes.c_void_p(stream)), 'dl_egnn_forward_pocket')
        if self.centering and center:
            out = self._center_velocity(out, prep['node_mask3'])
        return out, flags

    def forward(self, t, xh, node_mask, linker_mask, edge_mask, context):
        if xh.shape[0] == 0:
            return torch.zeros_like(xh)
        out, flags = self.launch(self.prepare(node_mask, linker_mask, edge_mask, context), t, xh)
        self._raise_on_flags(flags)
        return out


# ---- training: the backward of the denoiser (csrc/egnn_backward.hip: fully connected; csrc/egnn_backward_sparse.hip: pockets) ----
TRAINABLE_POCKET_GRAPHS = ('FC-4A', 'FC-10A-4A')
MAX_STATE_WIDTH = 16                  # row width of the per-atom state [x(3), h(in_node_nf)] (csrc/pack_layout.h: DMAX)


def check_trainable(dyn):
    """Raise ``NotImplementedError`` for a denoiser outside the backward's scope: fully-connected ``Dynamics`` and
    ``DynamicsWithPockets`` on the ``FC-4A`` / ``FC-10A-4A`` radius graphs, with the released hyper-parameters."""
    out = []
    pocket = type(dyn) is DynamicsWithPockets
    if not pocket and type(dyn) is not Dynamics:
        out.append(f'{type(dyn).__name__}')
    graph = getattr(dyn, 'graph_type', 'FC')
    if pocket:
        if graph not in TRAINABLE_POCKET_GRAPHS:
            out.append(f'{type(dyn).__name__} with graph_type={graph!r} (pocket training covers {", ".join(TRAINABLE_POCKET_GRAPHS)})')
    elif graph != 'FC':
        out.append(f'graph_type={graph!r}')
    if dyn.attention: out.append('attention=True')
    if dyn.tanh: out.append('tanh=True')
    if dyn.aggregation_method != 'sum': out.append(f'aggregation_method={dyn.aggregation_method!r}')
    if dyn.sin_embedding: out.append('sin_embedding=True')
    if dyn.dynamics.hidden_nf != HIDDEN_WIDTH: out.append(f'hidden_nf={dyn.dynamics.hidden_nf} (the backward is 128 wide)')
    if 3 + dyn.in_node_nf > MAX_STATE_WIDTH:
        out.append(f'in_node_nf={dyn.in_node_nf} (the kernels take 3 + in_node_nf <= {MAX_STATE_WIDTH})')
    if out:
        raise NotImplementedError('training (the HIP backward) covers fully-connected Dynamics and DynamicsWithPockets on the '
                                  'FC-4A / FC-10A-4A graphs, with the released hyper-parameters only; outside it: '
                                  + ', '.join(out))


POCKET_BACKWARD_MAX_ATOMS = 2048      # dl_egnn_backward_pocket's limit on the padded width (include/difflinker_hip.h)


def backward_args(dyn, B, N):
    return _lib.DLBackwardArgs(B=int(B), N=int(N), in_node_nf=dyn.in_node_nf, context_node_nf=dyn.context_node_nf,
                               condition_time=int(bool(dyn.condition_time)), hidden_nf=int(dyn.dynamics.hidden_nf),
                               n_layers=int(dyn.n_layers), inv_sublayers=int(dyn.inv_sublayers),
                               centering=int(bool(dyn.centering)), norm_constant=float(dyn.norm_constant),
                               normalization_factor=float(dyn.normalization_factor))


class _DenoiserFn(torch.autograd.Function):
    """``Dynamics.forward`` with a HIP backward: the forward runs the unchanged inference kernels (its values are the
    inference values bit for bit); the backward hands d eps_hat to ``dl_egnn_backward_fc`` and splits the flat gradient
    (``Dynamics.parameters()`` order) over the parameters.  No gradient for the inputs (out of scope)."""

    @staticmethod
    def forward(ctx, dyn, t, xh, node_mask, linker_mask, edge_mask, context, *params):
        out = dyn.forward(t=t, xh=xh, node_mask=node_mask, linker_mask=linker_mask, edge_mask=edge_mask, context=context)
        ctx.dyn = dyn
        ctx.save_for_backward(t, xh, node_mask, linker_mask, edge_mask, context)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        dyn = ctx.dyn
        t, xh, node_mask, linker_mask, edge_mask, context = ctx.saved_tensors
        grads = dyn.parameter_grad(t, xh, node_mask, linker_mask, edge_mask, context, grad_out)
        return (None,) * 7 + tuple(grads)


def _dynamics_parameter_grad(self, t, xh, node_mask, linker_mask, edge_mask, context, grad_out):
    """Gradients of ``sum(grad_out * self.forward(...))`` for every parameter, in ``parameters()`` order (HIP backward)."""
    check_trainable(self)
    dev = xh.device
    if dev.type != 'cuda':
        raise _lib.HipLibraryError('the EGNN backward runs on the HIP device only (no CPU fallback): '
                                   f'got tensors on {dev}')
    lib = _lib.load()
    bs, n = xh.shape[0], xh.shape[1]
    params = list(self.parameters())
    if bs == 0:
        return [torch.zeros_like(p) for p in params]
    pocket = isinstance(self, DynamicsWithPockets)
    limit = POCKET_BACKWARD_MAX_ATOMS if pocket else int(lib.dl_egnn_backward_max_atoms())
    if n > limit or (pocket and bs * n * n >= 2 ** 31):
        raise ValueError(f'the EGNN backward takes molecules of at most {limit} atoms (padded width)'
                         + (' and batches with B * N * N < 2^31' if pocket else '') + f'; got B = {bs}, N = {n}')
    f32 = lambda v: None if v is None else v.to(dev, torch.float32).contiguous()      # noqa: E731
    flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params]).contiguous()
    if not torch.is_tensor(t):
        t = torch.tensor([float(t)], device=dev)
    tt = f32(t).reshape(-1)
    args = backward_args(self, bs, n)
    want = int(lib.dl_egnn_backward_fc_num_params(ctypes.byref(args)))
    if want != flat.numel():
        raise ValueError(f'parameter count {flat.numel()} != the backward layout {want}')
    if pocket:
        graph = self.GRAPH_TYPES[self.graph_type]
        need = int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(args), graph))
    else:
        need = int(lib.dl_egnn_backward_fc_workspace_bytes(ctypes.byref(args)))
    ws = getattr(self, '_bwd_ws', None)
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = self._bwd_ws = None
        ws = self._bwd_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xh_ = f32(xh)
    nm = f32(node_mask.reshape(bs, n))
    lm = f32(linker_mask.reshape(bs, n)) if linker_mask is not None else None
    em = None if pocket else edge_mask.reshape(bs, n, n).to(dev, torch.int8).contiguous()   # pockets: the batch-index vector, unused
    ctx_ = f32(context.reshape(bs, n, self.context_node_nf)) if context is not None and self.context_node_nf else None
    go = f32(grad_out)
    grad = torch.empty_like(flat)
    args.params, args.n_params = flat.data_ptr(), flat.numel()
    args.xh, args.t, args.t_is_scalar = xh_.data_ptr(), tt.data_ptr(), int(tt.numel() == 1)
    args.node_mask, args.linker_mask = nm.data_ptr(), lm.data_ptr() if lm is not None else None
    args.edge_mask = em.data_ptr() if em is not None else None
    args.context = ctx_.data_ptr() if ctx_ is not None else None
    args.grad_out, args.grad_params = go.data_ptr(), grad.data_ptr()
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    if pocket:
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.dl_egnn_backward_pocket(ctypes.byref(args), graph, stream), 'dl_egnn_backward_pocket')
    else:
        _lib.launch('dl_egnn_backward_fc', args, dev)
    out, k = [], 0
    for p in params:
        out.append(grad[k:k + p.numel()].view_as(p).to(p.dtype))
        k += p.numel()
    return out


def _dynamics_training_forward(self, t, xh, node_mask, linker_mask, edge_mask, context):
    """``forward`` whose output carries a gradient to the parameters (HIP backward).  Same values as ``forward``."""
    check_trainable(self)
    if xh.device.type != 'cuda':
        raise _lib.HipLibraryError('Dynamics.training_forward runs on the HIP device only (no CPU fallback): '
                                   f'got tensors on {xh.device}')
    for name, v in (('t', t), ('xh', xh), ('context', context)):
        if torch.is_tensor(v) and v.requires_grad:
            raise NotImplementedError(f'gradients with respect to the input {name} are out of scope (parameters only)')
    if not torch.is_tensor(t):
        t = torch.tensor([float(t)], device=xh.device)
    return _DenoiserFn.apply(self, t, xh, node_mask, linker_mask, edge_mask, context, *self.parameters())


Dynamics.parameter_grad = _dynamics_parameter_grad
Dynamics.training_forward = _dynamics_training_forward
