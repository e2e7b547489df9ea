"""``EDM`` — the ancestral sampler of DiffLinker, MI355X-native.

Drop-in for the SAMPLING surface of reference ``src/edm.py::EDM`` (constructor edm.py:15-39,
``sample_chain`` :126-176 and the helpers it uses).  With a fully-connected ``Dynamics`` the whole
chain — T reverse steps (:178-208) + final decode (:210-242) — is ONE kernel launch
(``dl_sample_chain_fc``): every molecule keeps its state in LDS of one compute unit for all T+1
denoiser calls.  The noise is drawn up front with the reference's ``torch.randn`` call sequence
(x-part then h-part, 2(T+2) calls on the tensors' device), so the same ``torch.manual_seed`` gives
the same noise stream as the reference run on the same device.

``InpaintingEDM`` (edm.py:466-727, sampling side) is here too: one HIP denoiser call + one fused HIP tail per step.

Parity note: the per-step scalars (gamma lookup, expm1 / softplus / logsigmoid algebra) are evaluated on CPU fp32 tensors
of the reference's ``[B,1]`` shape (``step_coefficients``).  The reference evaluates them on the tensors' device; the
cancellation in sigma^2_{t|s} amplifies a 1-ulp difference of a device's transcendental to ~2e-5, so "same seed, same
samples" is claimed — and tested (golden fixtures) — against the reference run on the CPU.

``EDM.forward`` / ``InpaintingEDM.forward`` (edm.py:41-124, :467-548) evaluate the diffusion loss and the VLB terms of held-out
data (:244-326): a HIP noising prologue, the unchanged denoiser, a HIP per-molecule epilogue; no backward.

Out of scope (training only): the backward pass of the loss, the learned ``GammaNetwork`` schedule.
"""
import ctypes
import functools
import os
import threading
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, utils
from .egnn import Dynamics, DynamicsWithPockets
from .noise import PredefinedNoiseSchedule


# measured +2.8 .. 3.2 % on the C2 headline, same box (profiles/r05/ab_split_chain.log); DIFFLINKER_SPLIT_CHAIN=0 turns it off
SPLIT_CHAIN_DEFAULT = os.environ.get('DIFFLINKER_SPLIT_CHAIN', '1') == '1'


def compute_units(dev):
    """compute units of the device (256 on an MI355X): what one-molecule-per-compute-unit launches fill"""
    return torch.cuda.get_device_properties(dev).multi_processor_count


@functools.lru_cache(maxsize=None)
def xcd_layout(bs):
    """Launch positions of a size-sorted batch of `bs` molecules that fits the chip in one wave: ``order[xcd_layout(bs)]``.
    Workgroup k runs on XCD k % 8 (observed dispatch pattern; only speed depends on it), and the compute units of an XCD share
    one 4 MB L2 through which each of them streams the same 5.8 MB of weights per forward.  Molecules of SIMILAR SIZE on one XCD
    stay in phase, and a weight chunk one of them pulled in is still there when the others ask: the sorted batch is cut into
    16 runs of ceil(bs / 16) and every XCD gets two, one from the big end and one from the small end, dealt in a zig-zag (run
    xcd and run 15 - xcd): the same load on every XCD.  A CPU int64 tensor, a permutation of range(bs)."""
    ln = -(-bs // 16)
    k = np.arange(16 * ln)
    xcd, j = k % 8, k // 8
    idx = np.where(j < ln, xcd, 15 - xcd) * ln + j % ln
    return torch.from_numpy(idx[idx < bs])


def _pass_steps(receivers, senders):
    """pair-loop steps of one pass (egnn_fc.hip: slot_plan): `receivers` atoms share 256 slots, a slot walks ceil(senders / g) senders"""
    if receivers <= 0:
        return 0
    g = max(1, min(256 // receivers, senders))
    return -(-senders // g)


def forward_cost(n, n_linker, n_layers, sublayers, team=1):
    """Relative cost of one denoiser call for a molecule of `n` atoms (`n_linker` of them receivers of the coordinate pass) on
    `team` compute units, in units of one pair-loop step: steps of the GCL and coordinate passes plus a per-pass overhead fitted
    to the measured forward times (profiles/r04/forward_time_vs_n.log: 0.68 / 0.86 / 1.02 / 1.14 ms at n = 35 / 40 / 43 / 50 on one
    compute unit, 0.68 ms at n = 50 on a team of two).  Only the RATIOS matter: they place the hand-over step of split_plan."""
    own, own_l = -(-n // team), -(-max(n_linker, 1) // team)
    a_gcl, a_eq = (1.6, 1.1) if team == 1 else (1.7, 1.3)
    return n_layers * (sublayers * (_pass_steps(own, n) + a_gcl) + _pass_steps(own_l, n) + a_eq)


# The plan cache, and per device the side stream and the cached workspaces of the fused chain, are shared by every EDM of the
# process; _CACHE_LOCK guards the three dicts (lookup and insertion), not the tensors or streams in them.  EVERY CACHED WORKSPACE
# IS TIED TO THE ONE STREAM THAT SERIALISES ITS USES, which is what makes it safe for any number of EDMs, caller streams and threads:
#   (device, 'teams')          the team launch beside the main one (side_launch of _sample_chain_fused).  It always runs on the
#                              device's one side stream, whichever stream or thread the caller is on.
#   (device, 'join', stream)   the exchange rows, arrival words and join words of dl_sample_chain_fc_join.  That launch, and the
#                              hipMemsetAsync that clears its words, run on the CALLER's stream, so the buffer is keyed by that
#                              stream: two chains on two streams never share handshake words.  (torch hands out streams from a
#                              fixed pool, so the number of keys is bounded.)
# A buffer that has to grow is replaced, and the old tensor may still be in use by a launch another thread queued: 'teams' buffers
# are therefore marked as used by the side stream when they are made (record_stream: the allocator hands the block out again
# only after the side stream's work queued up to the release has completed); a 'join' buffer is allocated on, used on and
# released to the pool of the same stream, whose order covers it.
# The stream and thread contract of the Python layer ("Streams and threads"; tests/test_gpu_streams.py):
# DISTINCT Dynamics / EDM / SizeClassifier objects may run on any streams and threads at once.  ONE object caches one workspace
# each (_fc_ws, _large_ws, _bwd_ws, _workspaces), so it is used on one stream at a time and may move to another stream once
# that stream waits on the first.  This is narrower than the C ABI, where one dl_model may be shared by any number of streams.
_CACHE_LOCK = threading.Lock()
_PLAN_CACHE = {}
_SIDE_STREAMS = {}
_SIDE_WORKSPACE = {}


def split_plan(sizes, linkers, n_calls, compute_units, n_layers, sublayers, min_gain=0.02, grid=48):
    """The static hand-over inside a ragged batch that holds one compute unit per molecule.  FIRST launch: every molecule on its
    compute unit for about the same time tau - the small molecules complete their chain, every other molecule b stops after
    s_b = floor(tau / cost_b) denoiser calls and leaves its state in HBM.  SECOND launch: the unfinished molecules finish on TEAMS
    OF TWO, which take the compute units the small ones left (2 x teams <= compute units).  tau runs over a grid between the
    cheapest and the dearest molecule's chain; the plan with the smallest predicted makespan wins, provided it beats the single
    launch by `min_gain`.  A function of the sizes alone (cached by them).
    Returns (q_end of the first launch [B], molecules for teams) or None."""
    B = len(sizes)
    if B > compute_units or B == 0:
        return None
    key = (tuple(sizes), tuple(linkers), n_calls, compute_units, n_layers, sublayers, min_gain, grid)
    with _CACHE_LOCK:
        if key in _PLAN_CACHE:
            return _PLAN_CACHE[key]
    table = {}
    for n, l in set(zip(sizes, linkers)):
        table[(n, l)] = (forward_cost(n, l, n_layers, sublayers, 1), forward_cost(n, l, n_layers, sublayers, 2))
    c1 = np.array([table[k][0] for k in zip(sizes, linkers)])
    c2 = np.array([table[k][1] for k in zip(sizes, linkers)])
    single = float(c1.max()) * n_calls
    lo = float(c1.min()) * n_calls
    best = None
    for i in range(1, grid):
        tau = lo + (single - lo) * i / grid
        q_end = np.clip((tau / c1).astype(np.int64), 1, n_calls)
        rest = np.nonzero(q_end < n_calls)[0]
        if rest.size == 0 or 2 * rest.size > compute_units:        # every unfinished molecule on a team of two
            continue
        left1 = (n_calls - q_end[rest]) * c1[rest]
        teams = rest[np.lexsort((rest, -left1))]                    # most work left first; ties by index: deterministic
        total = float((q_end * c1).max()) + float(((n_calls - q_end[teams]) * c2[teams]).max())
        if best is None or total < best[0]:
            best = (total, q_end.tolist(), teams.tolist())
    plan = None if best is None or best[0] > (1.0 - min_gain) * single else (best[1], best[2])
    with _CACHE_LOCK:
        if len(_PLAN_CACHE) > 64:
            _PLAN_CACHE.clear()
        _PLAN_CACHE[key] = plan
    return plan


def join_plan(sizes, linkers, n_calls, compute_units, n_layers, sublayers, margin=0.03):
    """The hand-over of split_plan inside ONE launch (dl_sample_chain_fc_join): the same molecules (OWNERS, split_plan's teams)
    move to a team of two, but each as soon as a HELPER - a molecule that finished its own chain - is free, instead of all
    together behind the slowest molecule of a first launch.  Helpers are the molecules that split_plan leaves on one compute
    unit, matched in order: the earliest-finishing helper to the owner with the most work (pair i of both sorted lists).
    The owner's switch call is the first one it reaches a fraction `margin` after its helper's predicted finish: the helper
    usually arrives first and waits off the critical path, the owner seldom does.  A function of the sizes alone (cached).
    Returns (q_end [B]: switch call of an owner, n_calls for everybody else, owners [teams], helpers [teams]) or None: no
    split_plan, or fewer finished molecules than teams."""
    split = split_plan(sizes, linkers, n_calls, compute_units, n_layers, sublayers)
    if split is None:
        return None
    key = ('join', tuple(sizes), tuple(linkers), n_calls, compute_units, n_layers, sublayers, margin)
    with _CACHE_LOCK:
        if key in _PLAN_CACHE:
            return _PLAN_CACHE[key]
    owners = list(split[1])
    in_team = set(owners)
    rest = [b for b in range(len(sizes)) if b not in in_team]
    plan = None
    if len(rest) >= len(owners):
        c1 = [forward_cost(n, l, n_layers, sublayers, 1) for n, l in zip(sizes, linkers)]
        owners.sort(key=lambda b: (-c1[b], b))                     # most work first; ties by index: deterministic
        rest.sort(key=lambda b: (c1[b], b))                         # earliest finish first
        helpers = rest[:len(owners)]
        q_end = [n_calls] * len(sizes)
        for o, hp in zip(owners, helpers):
            arrive = n_calls * c1[hp] * (1.0 + margin)
            q_end[o] = int(min(max(-(-arrive // c1[o]), 1), n_calls - 1))
        plan = (q_end, owners, helpers)
    with _CACHE_LOCK:
        if len(_PLAN_CACHE) > 64:
            _PLAN_CACHE.clear()
        _PLAN_CACHE[key] = plan
    return plan


def join_makespan(plan, sizes, linkers, n_calls, n_layers, sublayers):
    """Makespan of a join_plan by the cost model (forward_cost units): a team starts when the later of owner and helper is there."""
    q_end, owners, helpers = plan
    c1 = [forward_cost(n, l, n_layers, sublayers, 1) for n, l in zip(sizes, linkers)]
    end = [n_calls * c for c in c1]
    for o, hp in zip(owners, helpers):
        start = max(q_end[o] * c1[o], end[hp])
        end[o] = start + (n_calls - q_end[o]) * forward_cost(sizes[o], linkers[o], n_layers, sublayers, 2)
    return max(end)


class EDM(torch.nn.Module):
    def __init__(
            self,
            dynamics,
            in_node_nf: int,
            n_dims: int,
            timesteps: int = 1000,
            noise_schedule='learned',
            noise_precision=1e-4,
            loss_type='vlb',
            norm_values=(1., 1., 1.),
            norm_biases=(None, 0., 0.),
    ):
        super().__init__()
        if noise_schedule == 'learned':
            raise NotImplementedError("noise_schedule='learned' (GammaNetwork) is training-only and out of scope; "
                                      'released configs use polynomial_2')
        self.gamma = PredefinedNoiseSchedule(noise_schedule, timesteps=timesteps, precision=noise_precision)
        self.dynamics = dynamics
        self.in_node_nf = in_node_nf
        self.n_dims = n_dims
        self.T = timesteps                      # callers overwrite it for --n_steps (generate.py:103-104)
        self.norm_values = norm_values
        self.norm_biases = norm_biases
        # 'torch' (default): the reference's own stream — torch.randn on the device in the reference's call order, so the
        # same torch.manual_seed reproduces the reference's draws.  'philox': counter-based draws generated inside the
        # kernels (no 2(T+2) randn launches, no noise bank in HBM), keyed by (noise_seed, global molecule index, atom,
        # draw) and therefore independent of the batch split; noise_seed advances by one per sampled chain.
        self.noise_source = 'torch'
        self.noise_seed = 0
        # batch size the per-step scalars are evaluated for (None: the batch at hand).  The reference evaluates them on
        # [B,1] tensors and PyTorch's CPU kernels round differently on their vector (B >= 16) and scalar paths, so a
        # shard of a batch pins this to the size of the whole batch to sample exactly what the unsharded call would.
        self.coef_batch = None
        # batch size the team size (compute units per molecule, Dynamics.team = 'auto') is chosen for (None: the batch at
        # hand).  A shard of a batch pins it to the whole batch as well: the order in which an atom's messages are summed
        # depends on the team size, so bitwise-identical samples for any split need one team size for all of them.
        self.team_batch = None
        # a batch of up to 1.25x the number of compute units: the molecules beyond one per compute unit are sampled by teams in a
        # second, concurrent launch (see _sample_chain_fused) instead of waiting for a second round.  Their messages are then
        # summed in the team's order: False keeps every molecule on one compute unit (bitwise the numbers of any other split).
        self.overflow_teams = True
        # a ragged batch that fills the chip (one molecule per compute unit): the chain runs in TWO launches - every molecule on its
        # compute unit until the small ones are done, then the big ones finish on teams of two that take the freed compute units
        # (see _sample_chain_fused / split_plan).  The steps a molecule runs on a team are summed in the team's order (fp32
        # rounding); the plan is a function of the batch's sizes alone, so a batch is sampled bit for bit the same every time.
        # False: one launch, every molecule on one compute unit for the whole chain.
        self.split_chain = SPLIT_CHAIN_DEFAULT
        # the launch route of the LAST fused chain (_sample_chain_fused; a batch sampled in parts: of its last part), set before
        # anything is launched: 'one' (dl_sample_chain_fc alone), 'join' (dl_sample_chain_fc_join: join_plan), 'two_launch' (the
        # first launch plus the resumed teams on the side stream: split_plan without a join_plan) or 'overflow_teams' (the molecules
        # beyond one per compute unit on teams beside the main launch).  An observable for tests and logs; nothing reads it.
        self.last_route = None

    @staticmethod
    def _side_stream(dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        with _CACHE_LOCK:
            if key not in _SIDE_STREAMS:
                _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
            return _SIDE_STREAMS[key]

    @staticmethod
    def _side_workspace(key, need, dev, used_on=None):
        """A cached workspace of the fused chain, one buffer per key - (device, 'teams') or (device, 'join', caller's stream):
        grown, never shrunk, reused by every chain on the stream that serialises its uses (see _CACHE_LOCK).  ``used_on``: the
        stream of the launches when it is not the one the buffer is allocated on; a buffer replaced by a bigger one is then
        kept from the allocator until what that stream holds at the release has run."""
        with _CACHE_LOCK:
            ws = _SIDE_WORKSPACE.get(key)
            if ws is None or ws.numel() < need:
                ws = _SIDE_WORKSPACE[key] = torch.empty(need, dtype=torch.uint8, device=dev)
                if used_on is not None:
                    ws.record_stream(used_on)
            return ws

    # ---- loss / VLB of held-out data (edm.py:41-124) -------------------------------------------------------
    def forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context=None, *, t_int=None, noise=None,
                mol_offset=0):
        """``EDM.forward`` (edm.py:41-124) for EVALUATION: one ``t`` per molecule, ``z_t`` from ``q(z_t | x, h)``, one denoiser
        call, the diffusion L2 loss and the VLB terms.  Returns the reference's 7-tuple ``(delta_log_px, kl_prior, loss_term_t,
        loss_term_0, l2_loss, noise_t, noise_0)`` with its batch reductions: ``loss_term_t`` / ``noise_t`` are NaN when no
        molecule has ``t > 0`` (the reference's 0/0), ``loss_term_0`` / ``noise_0`` the float ``0.`` when none has ``t = 0``.

        Three HIP launches: the noising prologue (``dl_edm_loss_prologue``), ``self.dynamics.forward`` (every kernel family,
        pockets, teams and FoundNaNException as in sampling), the per-molecule epilogue (``dl_edm_loss_epilogue``).
        Draws: ``noise_source='torch'`` - the reference's ``torch.randint`` then x- and h-``torch.randn`` on the tensors'
        device; ``'philox'`` - drawn in the kernels from (``noise_seed``, ``mol_offset`` + row, atom), ``noise_seed`` advances
        by one per call.  ``t_int`` (``[B]`` or ``[B,1]`` integers in ``0..T``) and ``noise = (noise_x [B,N,3], noise_h
        [B,N,nf])`` (unmasked) override the draws; neither is in the reference signature.

        Inference only: there is no backward (training is out of scope), so a call under grad mode with trainable dynamics
        parameters raises instead of returning losses that silently carry no gradient."""
        self._check_no_grad()
        rows, t_int_d = self._loss_rows(x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, t_int, noise,
                                        mol_offset)
        return self._reduce_loss_rows(rows, t_int_d)

    _inpainting = False

    def _check_no_grad(self):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.dynamics.parameters()):
            raise NotImplementedError('EDM.forward evaluates the loss without a backward pass (training is out of scope): '
                                      'wrap the call in torch.no_grad()')

    def _loss_rows(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, t_int, noise, mol_offset,
                   train_state=None):
        """Prologue, denoiser, epilogue.  Returns (rows [B, _lib.LOSS_ROW] fp32, t_int [B] int32), both on the device.
        ``train_state`` (a dict, training only): the denoiser output carries a gradient to the parameters, and the dict
        receives the kernel arguments and the tensors they point to (for ``dl_edm_loss_grad`` in the backward)."""
        dev = x.device
        if dev.type != 'cuda':
            raise _lib.HipLibraryError(f'{type(self).__name__}.forward runs on the HIP device only (no CPU fallback): '
                                       f'got tensors on {dev}')
        lib = _lib.load()
        bs, n = x.size(0), x.size(1)
        nf, T = self.in_node_nf, int(self.T)
        f32 = lambda t_, shape: t_.reshape(shape).to(dev, torch.float32).contiguous()      # noqa: E731
        # (fp32 first, then normalised: the arithmetic is fp32 whatever dtype the caller's tensors have)
        xn, hn = self.normalize(x.to(torch.float32), h.to(torch.float32))
        xh = torch.cat([xn, hn], dim=2).contiguous()
        nm = f32(node_mask, (bs, n))
        fm = f32(fragment_mask, (bs, n)) if fragment_mask is not None else None
        lm = f32(linker_mask, (bs, n)) if linker_mask is not None else None
        philox = self.noise_source == 'philox'
        if mol_offset and not philox and (t_int is None or noise is None):
            raise NotImplementedError("a shard of a batch (mol_offset) needs noise_source='philox' or explicit t_int and noise: "
                                      'the torch.randn stream is a property of the whole batch')
        if t_int is None and not philox:            # the reference's call order: randint, then the x- and h-randn
            t_int = torch.randint(0, T + 1, size=(bs, 1), device=dev)
        if noise is None and not philox:
            noise = (torch.randn((bs, n, self.n_dims), device=dev), torch.randn((bs, n, nf), device=dev))
        seed = 0
        if philox and (t_int is None or noise is None):
            seed = int(self.noise_seed) & 0xFFFFFFFFFFFFFFFF
            self.noise_seed = int(self.noise_seed) + 1
        t_given = t_int is not None
        t_int_d = (t_int.reshape(bs).to(dev, torch.int32).contiguous() if t_given
                   else torch.empty(bs, dtype=torch.int32, device=dev))
        nx = nh = None
        if noise is not None:
            nx, nh = f32(noise[0], (bs, n, self.n_dims)), f32(noise[1], (bs, n, nf))
        table = self.gamma.gamma.detach().to(dev, torch.float32).contiguous()
        prior = self._prior_constants(bs, dev)
        t_f = torch.empty(bs, dtype=torch.float32, device=dev)
        gam = torch.empty((bs, 2), dtype=torch.float32, device=dev)
        z_t = torch.empty_like(xh)
        rows = torch.empty((bs, _lib.LOSS_ROW), dtype=torch.float32, device=dev)
        if bs == 0:
            return rows, t_int_d
        args = _lib.DLLossArgs(
            B=bs, N=n, nf=nf, T=T, timesteps=int(self.gamma.timesteps), inpainting=int(self._inpainting),
            xh=xh.data_ptr(), node_mask=nm.data_ptr(), fragment_mask=fm.data_ptr() if fm is not None else None,
            linker_mask=lm.data_ptr() if lm is not None else None, gamma_table=table.data_ptr(),
            noise_x=nx.data_ptr() if nx is not None else None, noise_h=nh.data_ptr() if nh is not None else None,
            noise_seed=seed, mol_offset=int(mol_offset), t_given=int(t_given), t_int=t_int_d.data_ptr(), t=t_f.data_ptr(),
            gamma=gam.data_ptr(), z_t=z_t.data_ptr(), eps_hat=None, norm_h=float(self.norm_values[1]),
            bias_h=float(self.norm_biases[1]), prior=prior.data_ptr(), rows=rows.data_ptr())
        _lib.launch('dl_edm_loss_prologue', args, dev)
        # (InpaintingEDM denoises every atom: linker_mask=None, edm.py:499-506)
        eps_hat = self._loss_denoise(z_t, t_f.reshape(bs, 1), node_mask, None if self._inpainting else linker_mask, edge_mask,
                                     context, train=train_state is not None)
        eps_hat = eps_hat.to(torch.float32).contiguous()
        args.eps_hat = eps_hat.data_ptr()
        _lib.launch('dl_edm_loss_epilogue', args, dev)
        if train_state is not None:
            train_state.update(args=args, eps_hat=eps_hat, keep=(xh, nm, fm, lm, table, nx, nh, t_int_d, t_f, gam, z_t, prior,
                                                                 rows))
        return rows, t_int_d

    # ---- training (edm.py:41-124 with loss.backward()) ------------------------------------------------------------
    def training_forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context=None, *, t_int=None,
                         noise=None, mol_offset=0):
        """``forward`` for TRAINING: the same draws and the same 7-tuple, bit for bit, and ``l2_loss``, ``loss_term_t``,
        ``loss_term_0``, ``noise_t`` and ``noise_0`` carry a gradient to the parameters of ``self.dynamics`` (the others do
        not depend on them).  The backward is HIP: ``dl_edm_loss_grad`` forms d eps_hat from the per-molecule weights of the
        batch means, ``dl_egnn_backward_fc`` (pocket models: ``dl_egnn_backward_pocket``) the parameter gradients
        (``Dynamics.training_forward``).  Fully-connected ``Dynamics`` and ``DynamicsWithPockets`` on the FC-4A / FC-10A-4A
        graphs, with the released hyper-parameters only (``egnn.check_trainable``; anything else raises
        ``NotImplementedError``)."""
        from .egnn import check_trainable
        check_trainable(self.dynamics)
        if x.device.type != 'cuda':
            raise _lib.HipLibraryError(f'{type(self).__name__}.training_forward runs on the HIP device only (no CPU fallback): '
                                       f'got tensors on {x.device}')
        state = {}
        rows, t_int_d = self._loss_rows(x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, t_int, noise,
                                        mol_offset, train_state=state)
        if rows.size(0) == 0:
            return self._reduce_loss_rows(rows, t_int_d)
        vals = {}
        loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = _LossTerms.apply(state['eps_hat'], self, rows, t_int_d, state,
                                                                               vals)
        if vals['no_t0']:
            loss_term_0, noise_0 = 0., 0.
        return vals['delta_log_px'], vals['kl_prior'], loss_term_t, loss_term_0, l2_loss, noise_t, noise_0

    def _prior_constants(self, batch_size, dev):
        """``(alpha_T, sigma_T, log(1 / sigma_T))`` per molecule, device fp32 ``[B,3]``: ``kl_prior``'s constants
        (edm.py:244-272) evaluated as the reference evaluates them, on ``[B,1]`` CPU fp32 tensors (its vectorised and scalar
        paths may round differently, see ``step_coefficients``).  Each term of the KL cancels to a few ulp of these values,
        so the epilogue takes them as inputs.  Cached per batch size and table version."""
        key = (int(batch_size), self.gamma.gamma._version, str(dev))
        cached = getattr(self, '_prior_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        gamma = self.gamma.gamma.detach().to('cpu', torch.float32)
        gamma_T = gamma[torch.round(torch.ones((batch_size, 1)) * self.gamma.timesteps).long()]
        alpha_T = torch.sqrt(torch.sigmoid(-gamma_T))
        sigma_T = torch.sqrt(torch.sigmoid(gamma_T))
        log_inv = torch.log(torch.ones_like(sigma_T) / sigma_T)
        prior = torch.cat([alpha_T, sigma_T, log_inv], 1).to(dev).contiguous()
        self._prior_cache = (key, prior)
        return prior

    def _loss_denoise(self, z_t, t, node_mask, linker_mask, edge_mask, context, train=False):
        """The denoiser call of the loss (edm.py:77-84): ``Dynamics.forward`` unchanged; team sizes follow ``EDM.team_batch``
        when a shard of a batch pins it, and a team that cannot assemble means one more run on one compute unit per
        molecule from the same ``z_t``."""
        dyn = self.dynamics
        bs = z_t.size(0)

        def call():
            fn = dyn.training_forward if train else dyn.forward
            return fn(xh=z_t, t=t, node_mask=node_mask, linker_mask=linker_mask, context=context, edge_mask=edge_mask)
        if not hasattr(dyn, 'without_teams'):
            return call()
        saved = dyn.team_batch
        dyn.team_batch = bs if self.team_batch is None else max(bs, int(self.team_batch))
        try:
            return dyn.without_teams(call)
        finally:
            dyn.team_batch = saved

    def _reduce_loss_rows(self, rows, t_int):
        """The reference's batch reductions (edm.py:64-66, 89-121) of the per-molecule rows of ``dl_edm_loss_epilogue``."""
        error_t, noise, kl, log_px, log_ph, log_const, snr_weight, n_mask = rows.unbind(1)
        d = (n_mask - 1) * self.n_dims if self._inpainting else n_mask * self.n_dims
        delta_log_px = (-d * np.log(self.norm_values[0])).mean()
        t_is_zero = (t_int == 0).float()
        t_is_not_zero = 1 - t_is_zero
        l2_loss = (error_t / ((self.n_dims + self.in_node_nf) * n_mask)).mean()
        kl_prior = kl.mean()
        loss_term_t = self.T * 0.5 * snr_weight * error_t
        loss_term_t = (loss_term_t * t_is_not_zero).sum() / t_is_not_zero.sum()
        noise_t = (noise * t_is_not_zero).sum() / t_is_not_zero.sum()
        if t_is_zero.sum() > 0:                     # one host sync: the branch of edm.py:105
            loss_term_0 = -(log_px + log_ph) + (-log_const)
            loss_term_0 = (loss_term_0 * t_is_zero).sum() / t_is_zero.sum()
            noise_0 = (noise * t_is_zero).sum() / t_is_zero.sum()
        else:
            loss_term_0 = 0.
            noise_0 = 0.
        return delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0

    # ---- gamma algebra (host scalars; edm.py:369-403) -----------------------------------------------
    def sigma(self, gamma, target_tensor):
        return self.inflate_batch_array(torch.sqrt(torch.sigmoid(gamma)), target_tensor)

    def alpha(self, gamma, target_tensor):
        return self.inflate_batch_array(torch.sqrt(torch.sigmoid(-gamma)), target_tensor)

    def SNR(self, gamma):
        return torch.exp(-gamma)

    def sigma_and_alpha_t_given_s(self, gamma_t, gamma_s, target_tensor):
        sigma2_t_given_s = self.inflate_batch_array(
            -torch.expm1(F.softplus(gamma_s) - F.softplus(gamma_t)), target_tensor)
        log_alpha2_t_given_s = F.logsigmoid(-gamma_t) - F.logsigmoid(-gamma_s)
        alpha_t_given_s = self.inflate_batch_array(torch.exp(0.5 * log_alpha2_t_given_s), target_tensor)
        return sigma2_t_given_s, torch.sqrt(sigma2_t_given_s), alpha_t_given_s

    @staticmethod
    def inflate_batch_array(array, target):
        return array.view((array.size(0),) + (1,) * (len(target.size()) - 1))

    @staticmethod
    def numbers_of_nodes(mask):
        return torch.sum(mask.squeeze(2), dim=1)

    # ---- (un)normalisation (edm.py:347-361) ---------------------------------------------------------
    def normalize(self, x, h):
        return x / self.norm_values[0], (h.float() - self.norm_biases[1]) / self.norm_values[1]

    def unnormalize(self, x, h):
        return x * self.norm_values[0], h * self.norm_values[1] + self.norm_biases[1]

    def unnormalize_z(self, z):
        assert z.size(2) == self.n_dims + self.in_node_nf
        x, h = self.unnormalize(z[:, :, :self.n_dims], z[:, :, self.n_dims:])
        return torch.cat([x, h], dim=2)

    # ---- noise (edm.py:328-345) ---------------------------------------------------------------------
    def sample_combined_position_feature_noise(self, n_samples, n_nodes, mask):
        z_x = utils.sample_gaussian_with_mask(size=(n_samples, n_nodes, self.n_dims), device=mask.device,
                                              node_mask=mask)
        z_h = utils.sample_gaussian_with_mask(size=(n_samples, n_nodes, self.in_node_nf), device=mask.device,
                                              node_mask=mask)
        return torch.cat([z_x, z_h], dim=2)

    def sample_normal(self, mu, sigma, node_mask):
        return mu + sigma * self.sample_combined_position_feature_noise(mu.size(0), mu.size(1), node_mask)

    def draw_noise_bank(self, n_samples, n_nodes, device, n_steps=None):
        """All 2(T+2) standard-normal draws of one chain, in the reference's call order and shapes
        (x-part ``[B,N,3]`` then h-part ``[B,N,nf]``; initial z, T steps, decode), unmasked — the kernels
        apply ``linker_mask``.  Returns (noise_x [T+2,B,N,3], noise_h [T+2,B,N,nf])."""
        n_steps = self.T if n_steps is None else n_steps
        noise_x = torch.empty((n_steps + 2, n_samples, n_nodes, self.n_dims), device=device)
        noise_h = torch.empty((n_steps + 2, n_samples, n_nodes, self.in_node_nf), device=device)
        for k in range(n_steps + 2):
            # randn(size, out=slice) consumes the generator exactly like randn(size) does (same element count, same
            # launch) but writes in place: no temporary, no copy kernel (tests/test_gpu_philox.py checks the equality)
            torch.randn((n_samples, n_nodes, self.n_dims), out=noise_x[k])
            torch.randn((n_samples, n_nodes, self.in_node_nf), out=noise_h[k])
        return noise_x, noise_h

    # ---- per-step scalars ---------------------------------------------------------------------------
    def step_coefficients(self, batch_size=1):
        """Host (CPU fp32) restatement of the scalar algebra of every reverse step, in execution order
        s = T-1 ... 0 (edm.py:147-150,180-185,199,202) and of the final decode (:213-216,237-242).

        Evaluated per step on ``[batch_size, 1]`` tensors exactly as the reference does: PyTorch's CPU
        transcendentals round differently on its vectorised and scalar paths, and the cancellation in
        sigma^2_{t|s} amplifies that to ~2e-5, so the shape is part of the parity contract.
        Returns (coefs [T,4] = (t, alpha_ts, c_eps, sigma), (inv_alpha0, sigma0, sigma_x))."""
        if self.coef_batch is not None:
            batch_size = self.coef_batch
        key = (self.T, int(batch_size))
        cached = getattr(self, '_coef_cache', None)
        if cached is not None and cached[0] == key and cached[1] == self.gamma.gamma._version:
            return cached[2]
        gamma = self.gamma.gamma.detach().to('cpu', torch.float32)
        timesteps = self.gamma.timesteps
        lookup = lambda tt: gamma[torch.round(tt * timesteps).long()]
        rows = []
        for s_int in reversed(range(0, self.T)):
            s = torch.full((batch_size, 1), fill_value=s_int)
            t = (s + 1) / self.T
            s = s / self.T
            gamma_s, gamma_t = lookup(s), lookup(t)
            sigma2_ts, sigma_ts, alpha_ts = self.sigma_and_alpha_t_given_s(gamma_t, gamma_s, gamma_t)
            sigma_s = torch.sqrt(torch.sigmoid(gamma_s))
            sigma_t = torch.sqrt(torch.sigmoid(gamma_t))
            c_eps = sigma2_ts / alpha_ts / sigma_t
            sigma = sigma_ts * sigma_s / sigma_t
            rows.append(torch.stack([t[0, 0], alpha_ts[0, 0], c_eps[0, 0], sigma[0, 0]]))
        coefs = torch.stack(rows).to(torch.float32).contiguous()
        gamma_0 = lookup(torch.zeros(batch_size, 1))
        sigma_x = self.SNR(-0.5 * gamma_0)[0, 0]
        inv_alpha0 = (1. / torch.sqrt(torch.sigmoid(-gamma_0)))[0, 0]
        sigma0 = torch.sqrt(torch.sigmoid(gamma_0))[0, 0]
        out = (coefs, (float(inv_alpha0), float(sigma0), float(sigma_x)))
        self._coef_cache = (key, self.gamma.gamma._version, out)
        return out

    # ---- one reverse step / decode, host-driven (edm.py:178-242) --------------------------------------
    def sample_p_zs_given_zt_only_linker(self, s, t, z_t, node_mask, fragment_mask, linker_mask, edge_mask, context):
        """Samples z_s ~ p(z_s | z_t) for the linker atoms (edm.py:178-208): HIP denoiser + fused HIP tail."""
        gamma_s, gamma_t = self.gamma(s), self.gamma(t)
        sigma2_ts, sigma_ts, alpha_ts = self.sigma_and_alpha_t_given_s(gamma_t, gamma_s, z_t)
        sigma_s, sigma_t = self.sigma(gamma_s, target_tensor=z_t), self.sigma(gamma_t, target_tensor=z_t)
        eps_hat = self.dynamics.forward(xh=z_t, t=t, node_mask=node_mask, linker_mask=linker_mask,
                                        context=context, edge_mask=edge_mask)
        c_eps = sigma2_ts / alpha_ts / sigma_t
        sigma = sigma_ts * sigma_s / sigma_t
        bs, n, d = z_t.shape
        noise = torch.cat([torch.randn((bs, n, self.n_dims), device=z_t.device),
                           torch.randn((bs, n, self.in_node_nf), device=z_t.device)], dim=2)
        # the reference broadcasts per-sample scalars that are identical across the batch (edm.py:147-150)
        coef = _lib.DLStepCoef(float(t.reshape(-1)[0]), float(alpha_ts.reshape(-1)[0]), float(c_eps.reshape(-1)[0]),
                               float(sigma.reshape(-1)[0]))
        return self._sampler_step(z_t, eps_hat, noise, fragment_mask, linker_mask, coef)

    def _sampler_step(self, z_t, eps_hat, noise, fragment_mask, linker_mask, coef):
        lib = _lib.load()
        if z_t.device.type != 'cuda':
            raise RuntimeError('difflinker_amd.EDM runs on the GPU only (no CPU fallback)')
        bs, n, d = z_t.shape
        z_t, eps_hat, noise = z_t.float().contiguous(), eps_hat.float().contiguous(), noise.float().contiguous()
        fm = fragment_mask.reshape(bs, n).float().contiguous()
        lm = linker_mask.reshape(bs, n).float().contiguous()
        z_s = torch.empty_like(z_t)
        with torch.cuda.device(z_t.device):
            stream = torch.cuda.current_stream(z_t.device).cuda_stream
            _lib.check(lib.dl_sampler_step(bs, n, d, _lib.ptr(z_t), _lib.ptr(eps_hat), _lib.ptr(noise), _lib.ptr(fm),
                                           _lib.ptr(lm), coef, _lib.ptr(z_s), ctypes.c_void_p(stream)),
                       'dl_sampler_step')
        return z_s

    def compute_x_pred(self, eps_t, z_t, gamma_t):
        sigma_t = self.sigma(gamma_t, target_tensor=eps_t)
        alpha_t = self.alpha(gamma_t, target_tensor=eps_t)
        return 1. / alpha_t * (z_t - sigma_t * eps_t)

    def sample_p_xh_given_z0_only_linker(self, z_0, node_mask, fragment_mask, linker_mask, edge_mask, context):
        """Samples x,h ~ p(x,h | z_0) for the linker atoms (edm.py:210-235), host-driven."""
        zeros = torch.zeros(size=(z_0.size(0), 1), device=z_0.device)
        gamma_0 = self.gamma(zeros)
        sigma_x = self.SNR(-0.5 * gamma_0).unsqueeze(1)
        eps_hat = self.dynamics.forward(t=zeros, xh=z_0, node_mask=node_mask, linker_mask=linker_mask,
                                        edge_mask=edge_mask, context=context)
        eps_hat = eps_hat * linker_mask
        mu_x = self.compute_x_pred(eps_t=eps_hat, z_t=z_0, gamma_t=gamma_0)
        xh = self.sample_normal(mu=mu_x, sigma=sigma_x, node_mask=linker_mask)
        xh = z_0 * fragment_mask + xh * linker_mask
        x, h = self.unnormalize(xh[:, :, :self.n_dims], xh[:, :, self.n_dims:])
        h = F.one_hot(torch.argmax(h, dim=2), self.in_node_nf) * node_mask
        return x, h

    # ---- the chain ------------------------------------------------------------------------------------
    def _fused_ok(self):
        return isinstance(self.dynamics, Dynamics) and not isinstance(self.dynamics, DynamicsWithPockets) \
            and self.dynamics.graph_type == 'FC' and not self.dynamics.centering and not self.dynamics.sin_embedding

    @torch.no_grad()
    def sample_chain(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames=None,
                     noise_bank=None, mol_offset=0):
        """``EDM.sample_chain`` (edm.py:126-176).  Returns ``chain [keep_frames, B, N, 3+nf]`` whose frame 0
        is the final sample ``[x, one_hot(h)]``.

        ``noise_bank`` (optional, not in the reference signature) = ``(noise_x [T+2,B,N,3], noise_h
        [T+2,B,N,nf])`` replaces the internal ``torch.randn`` draws (parity tests share one bank with the
        CPU oracle).  ``mol_offset``: global index of the first molecule of this batch (``noise_source='philox'``
        with a batch sharded over ranks).
        """
        if keep_frames is None:
            keep_frames = self.T
        else:
            assert keep_frames <= self.T
        bs, n = x.size(0), x.size(1)
        if bs == 0:                                 # an empty batch is an empty chain in the reference (every op runs on empty tensors)
            return torch.zeros((keep_frames, 0, n, self.n_dims + self.in_node_nf), dtype=x.dtype, device=x.device)
        if not self._fused_ok():
            philox_draws = None
            if noise_bank is None and self.noise_source == 'philox':
                philox_draws = (int(self.noise_seed) & 0xFFFFFFFFFFFFFFFF, int(mol_offset))   # one draw per step, no bank
                self.noise_seed = int(self.noise_seed) + 1
            # a centering / sin_embedding Dynamics may still pick a team for its forward calls (small batch, 56..110 atoms): should
            # one fail to assemble, the chain is sampled again without teams - from the SAME draws (generator state restored) - and
            # nothing but FoundNaNException reaches the caller
            if not hasattr(self.dynamics, 'without_teams'):
                return self._sample_chain_host_loop(x, h, node_mask, fragment_mask, linker_mask, edge_mask, context,
                                                    keep_frames, noise_bank, philox_draws)
            # team sizes of the denoiser calls: those of the WHOLE batch (a shard pins EDM.team_batch), as on the fused chain
            self.dynamics.team_batch = bs if self.team_batch is None else max(bs, int(self.team_batch))
            rng = None
            if noise_bank is None and philox_draws is None and x.device.type == 'cuda':
                rng = torch.cuda.get_rng_state(x.device)

            def host_loop():
                if rng is not None:
                    torch.cuda.set_rng_state(rng, x.device)
                return self._sample_chain_host_loop(x, h, node_mask, fragment_mask, linker_mask, edge_mask, context,
                                                    keep_frames, noise_bank, philox_draws)
            try:
                return self.dynamics.without_teams(host_loop)
            finally:
                self.dynamics.team_batch = None
        dev = x.device
        if dev.type != 'cuda':
            raise RuntimeError('difflinker_amd.EDM.sample_chain runs on the GPU only (HIP kernels, no CPU fallback)')
        philox = noise_bank is None and self.noise_source == 'philox'
        seed = 0
        if philox:
            seed = int(self.noise_seed) & 0xFFFFFFFFFFFFFFFF
            self.noise_seed = int(self.noise_seed) + 1
        elif noise_bank is None:
            noise_bank = self.draw_noise_bank(bs, n, dev)       # the reference's call sequence, for the whole batch
        else:
            noise_bank = tuple(t.to(dev, torch.float32).contiguous() for t in noise_bank)
            assert tuple(noise_bank[0].shape) == (self.T + 2, bs, n, self.n_dims) and \
                tuple(noise_bank[1].shape) == (self.T + 2, bs, n, self.in_node_nf)
        # the draws are fixed by now: should a team of workgroups fail to assemble (another kernel holding compute units), the
        # same chain is sampled again on one compute unit per molecule - nothing but FoundNaNException reaches the caller
        return self.dynamics.without_teams(lambda: self._sample_chain_by_size(
            x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames, noise_bank, philox, seed, mol_offset))

    def _sample_chain_by_size(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames, noise_bank,
                              philox, seed, mol_offset):
        """Molecules of <= 55 atoms: the fused chain with one compute unit (or a team) per molecule; up to 110: the fused chain
        with a team of at least two, in pieces the chip holds at once; beyond: the HBM-resident kernels under a host-driven
        loop.  Noise rows and per-step scalars are those of the WHOLE batch, so every molecule gets the sample it would get
        from any of the paths alone."""
        bs, n = x.size(0), x.size(1)
        dev = x.device
        dyn = self.dynamics
        small, med, big = dyn.size_classes(node_mask.reshape(bs, n).to(torch.int8))
        if small is None and med is None and big is None:
            return self._sample_chain_fused(x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames,
                                            noise_bank, seed, mol_offset, None)
        em = edge_mask.reshape(bs, n * n) if edge_mask is not None else None

        def part(idx):
            return dict(x=x[idx], h=h[idx], node_mask=node_mask[idx], fragment_mask=fragment_mask[idx], linker_mask=linker_mask[idx],
                        edge_mask=em[idx].reshape(-1, 1) if em is not None else None,
                        context=context[idx] if context is not None else None)
        pinned, pinned_team = self.coef_batch, self.team_batch
        if pinned is None:
            self.coef_batch = bs
        if pinned_team is None:
            # the team sizes of every part follow the size of the WHOLE batch, exactly as in a shard of it
            # (distributed.sample_chain_sharded pins the same number; a pinned EDM.team_batch also keeps the chain in ONE launch
            # - no split_plan, no surplus teams): world = 1 and world > 1 sample the same bits for every molecule that the
            # unsharded call runs in one launch as well (a batch beyond the number of compute units, or split_chain = False)
            self.team_batch = bs
        try:
            chain = torch.zeros((keep_frames, bs, n, self.n_dims + self.in_node_nf), device=dev)
            fused = []
            if small is not None:
                fused.append((small, None))
            if med is not None:
                # team size of the 56..110-atom molecules: that of the WHOLE (possibly sharded) batch when the caller pinned it
                # (EDM.team_batch, distributed.sample_chain_sharded) - an atom's messages are summed in a team-size dependent
                # order, so a sample must not depend on how the batch was split - else of the piece at hand
                def med_team(count):
                    return max(2, dyn.team_for_size(max(count, int(self.team_batch)), dev))
                fused += [(c, med_team(int(c.numel()))) for c in dyn.team_chunks(med, dev)]
            # every part reports NaNs in ITS numbering, for ITS first offending denoiser call; the reference raises at the first
            # call whose output holds a NaN with the molecules that are NaN THERE (egnn.py:441-442) and its callers index the batch
            # with the sets of the exception (lightning.py:353-361): collect the sets in whole-batch numbering with their call
            # index, keep those of the earliest call, raise once.  Every part runs even after one has failed at call 0: the
            # molecules of another part that are NaN at call 0 too belong to the sets the reference reports (the
            # exception is rare and its callers re-sample the batch anyway, generate.py:154-161)
            nan_sets = []

            def run_part(idx, fn):
                try:
                    return fn()
                except utils.FoundNaNException as e:
                    rows = idx.tolist()
                    nan_sets.append((int(getattr(e, 'first_step', 0)),
                                     tuple({rows[k] for k in s_} for s_ in (e.x_h_nan_idx, e.only_x_nan_idx, e.only_h_nan_idx,
                                                                            getattr(e, 'f16_range_idx', ())))))
                    return None
            for idx, team in fused:
                bank = None if philox else (noise_bank[0][:, idx].contiguous(), noise_bank[1][:, idx].contiguous())
                got = run_part(idx, lambda: self._sample_chain_fused(keep_frames=keep_frames, noise_bank=bank, seed=seed,
                                                                     mol_offset=mol_offset, mol_index=idx.to(torch.int32).contiguous(),
                                                                     team=team, **part(idx)))
                if got is not None:
                    chain[:, idx] = got
            if big is not None:
                bank = None if philox else (noise_bank[0][:, big], noise_bank[1][:, big])
                large = run_part(big, lambda: self._sample_chain_host_loop(
                    keep_frames=keep_frames, noise_bank=bank, philox_draws=(seed, int(mol_offset), big, bs) if philox else None,
                    **part(big)))
                if large is not None:
                    chain[:, big] = large.to(chain.dtype)
            if nan_sets:
                first = min(step for step, _ in nan_sets)
                err = utils.FoundNaNException.from_index_sets(*(set().union(*(s_[k] for step, s_ in nan_sets if step == first))
                                                                for k in range(4)))
                err.first_step = first
                raise err
        finally:
            self.coef_batch = pinned
            self.team_batch = pinned_team
        return chain

    def _sample_chain_fused(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames, noise_bank,
                            seed, mol_offset, mol_index, team=None):
        """The whole chain as ONE launch (``dl_sample_chain_fc``) on the current stream, plus at most one launch of teams beside
        it on the side stream: the molecules beyond one per compute unit (overflow teams), or those that resume after the first
        launch's q_end (split_plan).  ``noise_bank`` = device tensors, or None: draws generated in the kernel from ``seed`` and
        the molecules' global indices ``mol_offset + mol_index[b]`` (``mol_index`` None: b)."""
        dev = x.device
        lib = _lib.load()
        bs, n = x.size(0), x.size(1)
        nf, T = self.in_node_nf, self.T
        handle = self.dynamics.hip_model(dev)
        philox = noise_bank is None
        noise_x, noise_h = (None, None) if philox else noise_bank
        coefs, (inv_alpha0, sigma0, sigma_x) = self.step_coefficients(bs)
        coefs = coefs.to(dev)
        f32 = lambda t_, shape: t_.reshape(shape).to(torch.float32).contiguous()
        xs, hs = f32(x, (bs, n, self.n_dims)), f32(h, (bs, n, nf))
        nm = node_mask.reshape(bs, n).to(torch.int8).contiguous()
        fm, lm = f32(fragment_mask, (bs, n)), f32(linker_mask, (bs, n))
        em = edge_mask.reshape(bs, n, n).to(torch.int8).contiguous() if edge_mask is not None else None
        ctx = f32(context, (bs, n, self.dynamics.context_node_nf)) if context is not None else None
        # longest-processing-time order: a molecule holds one compute unit for the whole chain and a workgroup's cost grows
        # with n_b^2, so the big ones are launched first (matters once the batch exceeds the number of compute units)
        n_real = nm.ne(0).sum(1)
        order = torch.argsort(n_real, descending=True, stable=True).to(torch.int32).contiguous()
        cus = compute_units(dev)
        if 16 <= bs <= cus:                 # a batch that fits the chip in one wave of workgroups: two size runs per XCD
            order = order[xcd_layout(bs).to(dev)].contiguous()
        chain = torch.zeros((keep_frames, bs, n, self.n_dims + nf), device=dev)
        flags = torch.zeros(bs, dtype=torch.int32, device=dev)
        steps = torch.full((bs,), -1, dtype=torch.int32, device=dev)
        # a batch smaller than the chip: several compute units per molecule (Dynamics.team)
        if team is None:
            team = 1 if self.dynamics._no_teams else \
                self.dynamics.team_for(bs if self.team_batch is None else max(bs, int(self.team_batch)), dev)
        # A batch just above the number of compute units: with one compute unit per molecule for the whole chain the molecules
        # beyond that number start only when others have finished (measured round 4: B = 257 costs 1.3x B = 256 on 256 compute
        # units).  The few molecules over - the smallest, last in the longest-first order - go to TEAMS of compute units in a
        # second launch on another stream instead: its workgroups take the compute units the smallest molecules of the first
        # launch leave after ~0.6 of the chain, and a team of four samples a 35-atom molecule in a quarter of the chain.
        over = 0
        if team == 1 and self.overflow_teams and self.team_batch is None and not self.dynamics._no_teams:
            if cus < bs <= cus + cus // 4:
                over = bs - cus
                team2 = 4 if over <= cus // 16 else 2
                # (the entry point refuses a team the device cannot hold at once - its round-up to whole groups of eight molecules
                # may not fit when the number of compute units is no multiple of 16: then everybody keeps one compute unit)
                while team2 > 1 and int(lib.dl_team_max(over)) < team2:
                    team2 //= 2
                if team2 < 2:
                    over = 0
            elif cus < bs < 2 * cus and not getattr(EDM, '_warned_off_sweet_spot', False):
                EDM._warned_off_sweet_spot = True              # say so once
                warnings.warn(f'EDM.sample_chain: a batch of {bs} molecules on {cus} compute units runs one molecule per compute unit '
                              f'for the whole chain, so the {bs - cus} molecules beyond {cus} start only when others have finished; '
                              f'batches of k x {cus} molecules (or up to {cus + cus // 4}, whose surplus is sampled by teams beside '
                              f'the rest) use the chip evenly', RuntimeWarning, stacklevel=3)
        ws, ws_bytes = self.dynamics.workspace(bs - over, team, dev)

        # the hand-over inside a ragged batch that fills the chip: ONE launch in which split_plan's teams form as helpers free up
        # (join_plan, dl_sample_chain_fc_join); two launches (split_plan) only when too few molecules finish early to help
        # (not for a shard of a batch - EDM.team_batch pinned, distributed.sample_chain_sharded: the plan follows the sizes of the
        # molecules at hand, and a molecule's sample must not depend on how its batch was split - SURVEY 8e)
        plan = join = None
        if team == 1 and over == 0 and self.split_chain and self.team_batch is None and not self.dynamics._no_teams \
                and bs <= cus and T >= 20:
            counts = torch.stack([n_real, lm.ne(0).sum(1)]).cpu()             # ONE device-to-host copy: sizes and linker sizes
            sizes_h, linkers_h = counts[0].tolist(), counts[1].tolist()
            if max(sizes_h) <= int(lib.dl_max_atoms()) and min(sizes_h) > 0:
                sub = int(getattr(self.dynamics, 'inv_sublayers', 2))
                plan = split_plan(sizes_h, linkers_h, T + 1, cus, self.dynamics.n_layers, sub)
                if plan is not None and int(lib.dl_team_max(len(plan[1]))) < 2:
                    plan = None                                               # the teams would not fit at once
                if plan is not None:
                    # one launch: each of split_plan's teams forms as soon as a molecule that finished its chain can join it
                    join = join_plan(sizes_h, linkers_h, T + 1, cus, self.dynamics.n_layers, sub)
                    if join is not None:
                        plan = None
        self.last_route = 'join' if join is not None else 'two_launch' if plan is not None else 'overflow_teams' if over else 'one'
        q_end_t = z_state = None
        if plan is not None or join is not None:
            q_end_t = torch.tensor((join or plan)[0], dtype=torch.int32, device=dev)
            z_state = torch.empty((bs, n, self.n_dims + nf), device=dev)

        def chain_args(flags_, steps_, team_, ws_, ws_bytes_, order_, first, count, q_begin=None, q_end=None, skip=None):
            return _lib.DLChainArgs(
                q_begin=q_begin.data_ptr() if q_begin is not None else None, q_end=q_end.data_ptr() if q_end is not None else None,
                z_state=z_state.data_ptr() if z_state is not None else None, skip_flags=skip.data_ptr() if skip is not None else None,
                B=bs, N=n, T=T, keep_frames=keep_frames,
                x=xs.data_ptr(), h=hs.data_ptr(), node_mask=nm.data_ptr(), fragment_mask=fm.data_ptr(),
                linker_mask=lm.data_ptr(), edge_mask=em.data_ptr() if em is not None else None,
                context=ctx.data_ptr() if ctx is not None else None,
                noise_x=None if philox else noise_x.data_ptr(), noise_h=None if philox else noise_h.data_ptr(),
                noise_seed=seed, mol_offset=int(mol_offset), team=team_, coefs=coefs.data_ptr(),
                inv_alpha0=inv_alpha0, sigma0=sigma0, sigma_x=sigma_x,
                norm_x=float(self.norm_values[0]), norm_h=float(self.norm_values[1]), bias_h=float(self.norm_biases[1]),
                chain=chain.data_ptr(), nan_flags=flags_.data_ptr(), nan_step=steps_.data_ptr(), order=order_.data_ptr(),
                workspace=ws_.data_ptr(), workspace_bytes=ws_bytes_,
                mol_index=mol_index.data_ptr() if mol_index is not None else None, order_first=first, order_count=count)

        def side_launch(after, team_, order_, first, count, q_begin=None):
            """The launch of teams beside the main one: on the device's side stream behind the event `after`, the current stream
            behind it.  `q_begin`: the molecules resume from z_state, skipping those the first launch flagged.  Its own flag
            arrays (the team entry point clears them on its stream); returns flags and steps merged with the main launch's."""
            side = self._side_stream(dev)
            flags2 = torch.empty(bs, dtype=torch.int32, device=dev)
            steps2 = torch.empty(bs, dtype=torch.int32, device=dev)
            need = int(lib.dl_workspace_bytes(count, team_))
            ws2 = self._side_workspace((dev.index, 'teams'), need, dev, used_on=side)
            skip = flags if q_begin is not None else None
            args2 = chain_args(flags2, steps2, team_, ws2, need, order_, first, count, q_begin=q_begin, skip=skip)
            side.wait_event(after)
            _lib.check(lib.dl_sample_chain_fc(handle, ctypes.byref(args2), ctypes.c_void_p(side.cuda_stream)),
                       'dl_sample_chain_fc (teams, beside the main launch)')
            done = torch.cuda.Event()
            done.record(side)
            cur.wait_event(done)
            for t_ in (xs, hs, nm, fm, lm, em, ctx, coefs, order_, chain, noise_x, noise_h, mol_index, q_begin, z_state, skip):
                if t_ is not None:
                    t_.record_stream(side)                 # the caching allocator must not hand these out while the side launch runs
            return flags | flags2, torch.where(steps2 >= 0, steps2, steps)

        args = chain_args(flags, steps, team, ws, ws_bytes, order, 0, bs - over if over else 0, q_end=q_end_t)
        profile = bool(getattr(self, 'profile_events', False))      # bench.py: HIP events right around the launches
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if profile:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(cur)
            if over:
                ready = torch.cuda.Event()
                ready.record(cur)                          # inputs, coefficients, noise bank: enqueued on the current stream
            if join is not None:
                _, owners, helpers = join
                team_of = [-1] * bs
                for j_, (o_, hp_) in enumerate(zip(owners, helpers)):
                    team_of[o_] = team_of[hp_] = j_
                maps = torch.tensor(team_of + owners, dtype=torch.int32, device=dev)
                need = int(lib.dl_join_workspace_bytes(len(owners)))
                jws = self._side_workspace((dev.index, 'join', cur.cuda_stream), need, dev)
                jargs = _lib.DLJoinArgs(teams=len(owners), team_of=maps.data_ptr(), team_mol=maps.data_ptr() + 4 * bs,
                                        workspace=jws.data_ptr(), workspace_bytes=need, wait_ticks=None)
                _lib.check(lib.dl_sample_chain_fc_join(handle, ctypes.byref(args), ctypes.byref(jargs),
                                                       ctypes.c_void_p(cur.cuda_stream)), 'dl_sample_chain_fc_join')
                self.last_split_event = None
            else:
                _lib.check(lib.dl_sample_chain_fc(handle, ctypes.byref(args), ctypes.c_void_p(cur.cuda_stream)),
                           'dl_sample_chain_fc')
            if over:
                # the molecules beyond one per compute unit, on teams beside the first launch
                flags, steps = side_launch(ready, team2, order, bs - over, over)
            if plan is not None:
                # the molecules with the most work left resume from z_state on teams of two, behind the first launch, biggest first
                after_first = torch.cuda.Event(enable_timing=profile)
                after_first.record(cur)
                self.last_split_event = after_first
                teams = sorted(plan[1], key=lambda b_: (-sizes_h[b_], b_))
                flags, steps = side_launch(after_first, 2, torch.tensor(teams, dtype=torch.int32, device=dev), 0, len(teams),
                                           q_begin=q_end_t)
            if profile:
                ev1.record(cur)
                self.last_kernel_events = (ev0, ev1)
        self._raise_on_chain_flags(flags, steps)
        bias = float(self.norm_biases[1])
        if bias != 0.0 and keep_frames > 1:
            # the kernel writes the rows of real atoms; the reference's intermediate frames are unnormalize_z of the WHOLE z
            # (edm.py:357-361), whose padding rows - zeros - come out as the feature bias (no released configuration has one)
            chain[1:, :, :, self.n_dims:] += bias * (1.0 - node_mask.to(chain.dtype).reshape(bs, n, 1))
        return chain

    def philox_noise_bank(self, n_samples, n_nodes, device, mol_offset=0, seed=None, n_draws=None):
        """The in-kernel stream as a bank ``(noise_x [T+2,B,N,3], noise_h [T+2,B,N,nf])`` (``dl_philox_fill``; ``n_draws``: another
        number of draws); advances ``noise_seed`` unless ``seed`` is given."""
        if torch.device(device).type != 'cuda':
            raise RuntimeError('the Philox noise bank is generated on the GPU (no CPU fallback)')
        if seed is None:
            seed = int(self.noise_seed)
            self.noise_seed = seed + 1
        n_draws = self.T + 2 if n_draws is None else int(n_draws)
        noise_x = torch.empty((n_draws, n_samples, n_nodes, self.n_dims), device=device)
        noise_h = torch.empty((n_draws, n_samples, n_nodes, self.in_node_nf), device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(_lib.load().dl_philox_fill(int(seed) & 0xFFFFFFFFFFFFFFFF, int(mol_offset), None, n_samples, n_nodes,
                                                  self.in_node_nf, 0, n_draws, noise_x.data_ptr(), noise_h.data_ptr(),
                                                  ctypes.c_void_p(stream)), 'dl_philox_fill')
        return noise_x, noise_h

    def _raise_on_chain_flags(self, flags, steps):
        """The reference raises at the first denoiser call whose output holds a NaN (egnn.py:441-442);
        the fused chain reports, per molecule, its first offending call — raise for the earliest one."""
        if bool(flags.any()):
            f, st = flags.cpu(), steps.cpu()
            if bool((f & 8).any()):
                from .egnn import TeamNotAssembled
                raise TeamNotAssembled('a team of workgroups did not assemble in time (another kernel held compute units)')
            if bool((f & 4).any()):
                raise ValueError('molecule with more real atoms than the LDS-resident fully-connected kernels take')
            first = int(st[f != 0].min())
            err = utils.FoundNaNException.from_flags(torch.where((st == first) & (f != 0), f, torch.zeros_like(f)))
            err.first_step = first          # the denoiser call (0 .. T) the exception stands for: a batch sampled in parts keeps the earliest
            raise err

    def _philox_draw(self, seed, mol_offset, k, n_samples, n_nodes, device, mol_index=None):
        """Draw number ``k`` of the in-kernel stream as one ``[B,N,3+nf]`` tensor (``dl_philox_fill`` with one draw);
        ``mol_index`` (device int32 ``[B]``): the rows of these molecules of a larger batch, and nothing else."""
        nx = torch.empty((1, n_samples, n_nodes, self.n_dims), device=device)
        nh = torch.empty((1, n_samples, n_nodes, self.in_node_nf), device=device)
        if mol_index is not None:
            mol_index = mol_index.to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(_lib.load().dl_philox_fill(seed, mol_offset, _lib.ptr(mol_index), n_samples, n_nodes, self.in_node_nf, k, 1,
                                                  nx.data_ptr(), nh.data_ptr(), ctypes.c_void_p(stream)), 'dl_philox_fill')
        return torch.cat([nx[0], nh[0]], dim=2)

    def _sample_chain_host_loop(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, keep_frames,
                                noise_bank=None, philox_draws=None):
        """Reference-shaped loop for dynamics the fused kernel does not cover (pockets): one HIP denoiser call
        and one fused HIP tail per step (edm.py:126-176).  Noise: the reference's ``torch.randn`` call order,
        or the given bank ``(noise_x [T+2,B,N,3], noise_h [T+2,B,N,nf])``."""
        n_samples, n_nodes = x.size(0), x.size(1)
        dev = x.device
        draw_idx = [0]

        def draw():
            k = draw_idx[0]
            draw_idx[0] += 1
            if noise_bank is not None:
                return torch.cat([noise_bank[0][k].to(dev, torch.float32), noise_bank[1][k].to(dev, torch.float32)], dim=2)
            if philox_draws is not None:
                if len(philox_draws) == 4:       # (seed, mol_offset, rows, size of the whole batch): a non-contiguous part of it
                    rows = philox_draws[2].to(torch.int32).contiguous()
                    return self._philox_draw(philox_draws[0], philox_draws[1], k, n_samples, n_nodes, dev, mol_index=rows)
                return self._philox_draw(philox_draws[0], philox_draws[1], k, n_samples, n_nodes, dev)
            return torch.cat([torch.randn((n_samples, n_nodes, self.n_dims), device=dev),
                              torch.randn((n_samples, n_nodes, self.in_node_nf), device=dev)], dim=2)

        x, h = self.normalize(x.to(torch.float32), h.to(torch.float32))          # (fp32 first, as in _loss_rows)
        xh = torch.cat([x, h], dim=2)
        z = xh * fragment_mask + (draw() * linker_mask) * linker_mask
        chain = torch.zeros((keep_frames,) + z.size(), device=dev)
        coefs, (inv_alpha0, sigma0, sigma_x) = self.step_coefficients(n_samples)
        # pocket dynamics: convert / check the masks once per chain and only enqueue kernels per step; the NaN flags of
        # every call are OR-ed on the device and examined once at the end (a NaN never heals along the chain)
        prep = self.dynamics.prepare(node_mask, linker_mask, edge_mask, context) if hasattr(self.dynamics, 'prepare') else None
        seen = torch.zeros(n_samples, dtype=torch.int32, device=dev) if prep is not None else None
        first_bad = torch.full((n_samples,), -1, dtype=torch.int32, device=dev) if prep is not None else None

        def denoise(z_, t_arr_, q_):
            if prep is None:
                return self.dynamics.forward(xh=z_, t=t_arr_, node_mask=node_mask, linker_mask=linker_mask,
                                             context=context, edge_mask=edge_mask)
            out, flags = self.dynamics.launch(prep, t_arr_, z_)
            if q_ == 0 and not isinstance(self.dynamics, DynamicsWithPockets) and not self.dynamics._no_teams:
                # a Dynamics may run this loop on teams of workgroups (small batch, 56..110 atoms): should they fail to assemble
                # (a co-tenant kernel holding compute units), say so after the FIRST launch - every further one would spin to the
                # limit as well - and let without_teams() repeat the chain on one compute unit per molecule
                if bool((flags & 8).any()):
                    from .egnn import TeamNotAssembled
                    raise TeamNotAssembled('a team of workgroups did not assemble in time (another kernel held compute units)')
            newly = (flags != 0) & (seen == 0)
            first_bad.masked_fill_(newly, q_)
            seen.bitwise_or_(flags)
            return out

        t_arr = torch.empty((n_samples, 1), device=dev)
        for q, s in enumerate(reversed(range(0, self.T))):
            t_, a_, c_, sg_ = (float(v) for v in coefs[q])
            t_arr.fill_(t_)
            eps_hat = denoise(z, t_arr, q)
            z = self._sampler_step(z, eps_hat, draw(), fragment_mask, linker_mask, _lib.DLStepCoef(t_, a_, c_, sg_))
            widx = (s * keep_frames) // self.T
            if s == 0 or ((s - 1) * keep_frames) // self.T != widx:       # only the last writer of a frame survives
                chain[widx] = self.unnormalize_z(z)
        # final decode (edm.py:210-235)
        zeros = torch.zeros(size=(n_samples, 1), device=dev)
        eps_hat = denoise(z, zeros, self.T) * linker_mask
        if prep is not None:
            self._raise_on_chain_flags(seen, first_bad)
        mu_x = inv_alpha0 * (z - sigma0 * eps_hat)
        xh = mu_x + sigma_x * (draw() * linker_mask)
        xh = z * fragment_mask + xh * linker_mask
        x, h = self.unnormalize(xh[:, :, :self.n_dims], xh[:, :, self.n_dims:])
        h = F.one_hot(torch.argmax(h, dim=2), self.in_node_nf) * node_mask
        chain[0] = torch.cat([x, h], dim=2)
        return chain


class _LossTerms(torch.autograd.Function):
    """The eps_hat-dependent batch terms of ``EDM.forward`` (values from ``_reduce_loss_rows``, unchanged) with their
    gradient: per molecule the weights of error_t, |eps_hat| and log p(x | z_0) in the batch means, then
    ``dl_edm_loss_grad``."""

    @staticmethod
    def forward(ctx, eps_hat, edm, rows, t_int, state, vals):
        ctx.set_materialize_grads(False)
        delta_log_px, kl_prior, loss_term_t, loss_term_0, l2_loss, noise_t, noise_0 = edm._reduce_loss_rows(rows, t_int)
        vals.update(delta_log_px=delta_log_px, kl_prior=kl_prior, no_t0=not torch.is_tensor(loss_term_0))
        ctx.edm, ctx.state = edm, state
        ctx.save_for_backward(rows, t_int)
        zero = torch.zeros((), dtype=torch.float32, device=rows.device)
        return (loss_term_t, loss_term_0 if torch.is_tensor(loss_term_0) else zero, l2_loss, noise_t,
                noise_0 if torch.is_tensor(noise_0) else zero.clone())

    @staticmethod
    def backward(ctx, g_lt, g_l0, g_l2, g_nt, g_n0):
        edm, state = ctx.edm, ctx.state
        rows, t_int = ctx.saved_tensors
        bs = rows.size(0)
        error_t, noise, kl, log_px, log_ph, log_const, snr_weight, n_mask = rows.unbind(1)
        tz = (t_int == 0).float()
        tnz = 1 - tz
        w_err = torch.zeros_like(error_t)
        w_noise = torch.zeros_like(error_t)
        w_logpx = torch.zeros_like(error_t)
        if g_l2 is not None:                                # l2_loss = mean(error_t / ((3 + nf) n))
            w_err = w_err + g_l2 / (bs * (edm.n_dims + edm.in_node_nf) * n_mask)
        if g_lt is not None:                                # loss_term_t = sum(T / 2 SNR_w error_t [t > 0]) / count(t > 0)
            w_err = w_err + g_lt * (edm.T * 0.5) * snr_weight * tnz / tnz.sum()
        if g_nt is not None:
            w_noise = w_noise + g_nt * tnz / tnz.sum()
        if g_l0 is not None:                                # loss_term_0 = -(log p(x) + log p(h)) - const over t = 0
            w_logpx = w_logpx - g_l0 * tz / tz.sum()
        if g_n0 is not None:
            w_noise = w_noise + g_n0 * tz / tz.sum()
        weights = torch.stack([w_err, w_noise, w_logpx], 1).to(torch.float32).contiguous()
        eps_hat = state['eps_hat']
        grad = torch.empty_like(eps_hat)
        dev = eps_hat.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.dl_edm_loss_grad(ctypes.byref(state['args']), _lib.ptr(weights), _lib.ptr(grad), stream),
                       'dl_edm_loss_grad')
        return grad, None, None, None, None, None


class InpaintingEDM(EDM):
    """``InpaintingEDM`` (edm.py:466-727), sampling side: every atom is denoised (``linker_mask=None``, centred dynamics),
    the linker atoms keep the ``p(z_s | z_t)`` sample, the fragment atoms are re-drawn from ``q(z_s | z_t, x)``, and the
    centre of gravity is projected out after every step.  One HIP denoiser call + one fused HIP tail
    (``dl_inpaint_step``) per step; no released configuration uses it."""

    _inpainting = True

    def forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context=None, *, t_int=None, noise=None,
                mol_offset=0):
        """``InpaintingEDM.forward`` (edm.py:467-548): ``EDM.forward`` with noise on every atom of ``node_mask`` (the x-part
        centre-of-gravity free, edm.py:715-727), ``z_t = alpha_t xh + sigma_t eps`` for every atom, the denoiser output
        unmasked and ``dimensionality = (n - 1) * 3``.  Same draws, overrides and return value as ``EDM.forward``."""
        return EDM.forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, t_int=t_int, noise=noise,
                           mol_offset=mol_offset)

    def training_forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context=None, *, t_int=None,
                         noise=None, mol_offset=0):
        """``InpaintingEDM.forward`` for training: ``EDM.training_forward`` with the inpainting draws (the denoiser must be
        ``centering=True``, as ``DDPM(inpainting=True)`` builds it)."""
        return EDM.training_forward(self, x, h, node_mask, fragment_mask, linker_mask, edge_mask, context, t_int=t_int,
                                    noise=noise, mol_offset=mol_offset)

    def inpaint_coefficients(self, batch_size=1):
        """Per-step scalars in execution order: ``(t, alpha_ts, c_eps, sigma, a_q, b_q)`` (edm.py:616-672), evaluated on
        ``[batch_size, 1]`` CPU tensors like ``EDM.step_coefficients``."""
        if self.coef_batch is not None:
            batch_size = self.coef_batch
        gamma = self.gamma.gamma.detach().to('cpu', torch.float32)
        timesteps = self.gamma.timesteps
        lookup = lambda tt: gamma[torch.round(tt * timesteps).long()]       # noqa: E731
        rows = []
        for s_int in reversed(range(0, self.T)):
            s = torch.full((batch_size, 1), fill_value=s_int)
            t = (s + 1) / self.T
            s = s / self.T
            gamma_s, gamma_t = lookup(s), lookup(t)
            sigma2_ts, sigma_ts, alpha_ts = self.sigma_and_alpha_t_given_s(gamma_t, gamma_s, gamma_t)
            sigma_s = torch.sqrt(torch.sigmoid(gamma_s))
            sigma_t = torch.sqrt(torch.sigmoid(gamma_t))
            alpha_s = torch.sqrt(torch.sigmoid(-gamma_s))
            c_eps = sigma2_ts / alpha_ts / sigma_t
            sigma = sigma_ts * sigma_s / sigma_t
            a_q = alpha_ts * (sigma_s ** 2) / (sigma_t ** 2)
            b_q = alpha_s * sigma2_ts / (sigma_t ** 2)
            rows.append([float(v[0, 0]) for v in (t, alpha_ts, c_eps, sigma, a_q, b_q)])
        return rows

    def draw_inpainting_noise_bank(self, n_samples, n_nodes, device):
        """The ``torch.randn`` calls of one chain in the reference's order: initial z, then (p, q) per step, then the p
        and q draws of the decode; each an x-part ``[B,N,3]`` and an h-part ``[B,N,nf]`` (utils.py:158-168,189-192)."""
        n = 1 + 2 * self.T + 2
        noise_x = torch.empty((n, n_samples, n_nodes, self.n_dims), device=device)
        noise_h = torch.empty((n, n_samples, n_nodes, self.in_node_nf), device=device)
        for k in range(n):
            torch.randn((n_samples, n_nodes, self.n_dims), out=noise_x[k])
            torch.randn((n_samples, n_nodes, self.in_node_nf), out=noise_h[k])
        return noise_x, noise_h

    @torch.no_grad()
    def sample_chain(self, x, h, node_mask, edge_mask, fragment_mask, linker_mask, context, keep_frames=None,
                     noise_bank=None, mol_offset=0):
        """``InpaintingEDM.sample_chain`` (edm.py:549-610).  Noise: the reference's ``torch.randn`` sequence, an explicit bank of
        ``1 + 2T + 2`` draws (initial z, then the p and q draw of every step, then the two of the decode), or - round 5 -
        ``noise_source='philox'``: that bank generated on the device from (``noise_seed``, GLOBAL molecule index = ``mol_offset`` +
        row, atom, draw), so a shard of a batch samples what the whole batch would (``distributed.sample_chain_sharded``); the
        ``torch.randn`` stream cannot be sharded (``mol_offset`` raises with it)."""
        philox = noise_bank is None and self.noise_source == 'philox'
        if mol_offset and not philox and noise_bank is None:
            raise NotImplementedError("a shard of a batch (mol_offset) needs noise_source='philox' or the shard's rows of an explicit "
                                      'noise_bank: the torch.randn stream is a property of the whole batch')
        dev = x.device
        if dev.type != 'cuda':
            raise RuntimeError('difflinker_amd.InpaintingEDM.sample_chain runs on the GPU only (HIP kernels, no CPU fallback)')
        if not getattr(self.dynamics, 'centering', False):
            raise ValueError('InpaintingEDM needs a centred denoiser (Dynamics(centering=True), lightning.py:99)')
        lib = _lib.load()
        bs, n = x.size(0), x.size(1)
        nf, T = self.in_node_nf, self.T
        keep_frames = T if keep_frames is None else keep_frames
        assert keep_frames <= T
        if bs == 0:
            return torch.zeros((keep_frames, 0, n, self.n_dims + nf), dtype=x.dtype, device=dev)
        if philox:
            noise_x, noise_h = self.philox_noise_bank(bs, n, dev, mol_offset=mol_offset, n_draws=1 + 2 * T + 2)
        elif noise_bank is None:
            noise_x, noise_h = self.draw_inpainting_noise_bank(bs, n, dev)
        else:
            noise_x, noise_h = (t_.to(dev, torch.float32).contiguous() for t_ in noise_bank)
            assert noise_x.shape[0] == 1 + 2 * T + 2
        # (the draws are fixed: a team of workgroups that cannot assemble means one more run on one compute unit per molecule;
        # team sizes follow the WHOLE batch when this is a shard of one: EDM.team_batch)
        self.dynamics.team_batch = bs if self.team_batch is None else max(bs, int(self.team_batch))
        try:
            return self.dynamics.without_teams(lambda: self._inpaint_chain(x, h, node_mask, edge_mask, fragment_mask, linker_mask,
                                                                           context, keep_frames, noise_x, noise_h))
        finally:
            self.dynamics.team_batch = None

    def _inpaint_chain(self, x, h, node_mask, edge_mask, fragment_mask, linker_mask, context, keep_frames, noise_x, noise_h):
        lib = _lib.load()
        dev = x.device
        bs, n = x.size(0), x.size(1)
        nf, T = self.in_node_nf, self.T
        f32 = lambda t_, shape: t_.reshape(shape).to(torch.float32).contiguous()      # noqa: E731
        nm, fm, lm = f32(node_mask, (bs, n)), f32(fragment_mask, (bs, n)), f32(linker_mask, (bs, n))
        xn, hn = self.normalize(x.to(torch.float32), h.to(torch.float32))        # (fp32 first, as in _loss_rows)
        xh = torch.cat([xn, hn], dim=2)
        xh_frag = (xh * fm.unsqueeze(-1)).contiguous()
        # initial z: centre-of-gravity-free position noise + feature noise on the node mask (edm.py:559, :715-727)
        nm3 = nm.unsqueeze(-1)
        zx = noise_x[0] * nm3
        zx = zx - (zx.sum(1, keepdim=True) / nm3.sum(1, keepdim=True)) * nm3
        z = torch.cat([zx, noise_h[0] * nm3], dim=2).contiguous()
        chain = torch.zeros((keep_frames,) + z.size(), device=dev)
        rows = self.inpaint_coefficients(bs)
        _, (inv_alpha0, sigma0, sigma_x) = self.step_coefficients(bs)
        prep = self.dynamics.prepare(node_mask, None, edge_mask, context)
        seen = torch.zeros(bs, dtype=torch.int32, device=dev)
        first_bad = torch.full((bs,), -1, dtype=torch.int32, device=dev)
        t_arr = torch.empty((bs, 1), device=dev)
        norm = dict(norm_x=float(self.norm_values[0]), norm_h=float(self.norm_values[1]), bias_h=float(self.norm_biases[1]))

        def tail(z_, eps_, k_p, k_q, coef):
            out = torch.empty_like(z_)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(lib.dl_inpaint_step(bs, n, nf, _lib.ptr(z_), _lib.ptr(eps_), _lib.ptr(xh_frag),
                                               _lib.ptr(noise_x[k_p]), _lib.ptr(noise_h[k_p]), _lib.ptr(noise_x[k_q]),
                                               _lib.ptr(noise_h[k_q]), _lib.ptr(nm), _lib.ptr(fm), _lib.ptr(lm), coef,
                                               _lib.ptr(out), ctypes.c_void_p(stream)), 'dl_inpaint_step')
            return out

        def denoise(z_, q_):
            eps_, flags = self.dynamics.launch(prep, t_arr, z_, center=False)      # dl_inpaint_step centres the velocity
            first_bad.masked_fill_((flags != 0) & (seen == 0), q_)
            seen.bitwise_or_(flags)
            return eps_

        for q, s in enumerate(reversed(range(0, T))):
            t_, a_, c_, sg_, aq_, bq_ = rows[q]
            t_arr.fill_(t_)
            eps_hat = denoise(z, q)
            coef = _lib.DLInpaintCoef(alpha_ts=a_, c_eps=c_, sigma=sg_, a_q=aq_, b_q=bq_, decode=0, inv_alpha0=0.0,
                                      sigma0=0.0, sigma_x=0.0, **norm)
            z = tail(z, eps_hat, 1 + 2 * q, 2 + 2 * q, coef)
            widx = (s * keep_frames) // T
            if s == 0 or ((s - 1) * keep_frames) // T != widx:
                chain[widx] = self.unnormalize_z(z)
        t_arr.fill_(0.0)
        eps_hat = denoise(z, T)
        self._raise_on_chain_flags(seen, first_bad)
        coef = _lib.DLInpaintCoef(alpha_ts=1.0, c_eps=0.0, sigma=0.0, a_q=0.0, b_q=0.0, decode=1, inv_alpha0=inv_alpha0,
                                  sigma0=sigma0, sigma_x=sigma_x, **norm)
        chain[0] = tail(z, eps_hat, 1 + 2 * T, 2 + 2 * T, coef)
        return chain
