"""The workspace contract of every HIP entry point: THE DEFINED PART OF EVERY RESULT, AND EVERY STATUS FLAG, IS A FUNCTION OF
THE INPUTS ALONE, BIT FOR BIT, WHATEVER THE SCRATCH AND OUTPUT BUFFERS HELD ON ENTRY (include/difflinker_hip.h).

Every workspace and every output of the Python layer comes from ``torch.empty`` / ``torch.empty_like`` and is cached and reused,
so what a kernel finds there is an accident: zero pages in a fresh process (what every other test of this suite sees), whatever
the caching allocator last freed in a long-running sampler or trainer.  Each case here runs its entry point once un-patched and
once under each of four fill patterns (``helpers.poisoned_allocations``: zeros, all ones = NaN / -1, 0x7F7F7F7F = 3.4e38 / fp16
NaN / a huge integer, fp32 +inf), on fresh objects from the same seeded weights, inputs and draws, and asserts

  * no exception and no warning of the product (no ``FoundNaNException``, no ``TeamNotAssembled`` re-run),
  * status / NaN flags and the defined region of every output ``torch.equal`` (as bits) to the zero-filled run's,
  * the zero-filled run equal to the un-patched one (the patch changes nothing but the initial bytes),
  * the workspace the entry point really used - at least the size the library asks for - among the recorded poisoned buffers.

"Defined region" is what the API documents as written: whole tensors everywhere (eps_hat, flags, chains, gradients, loss rows,
logits, ``valence`` / ``component`` / ``colour`` with their documented padding values, ``rmsd`` / ``best`` / ``status``) except
the bond list, of which only ``bonds[b, :min(n_bonds[b], capacity)]`` is written (difflinker_hip.h: "entries from n_bonds on
are not written").  The poison goes in before a call, never while a launch is in flight.

The padding-atom columns of ``stream_phase`` (egnn_fc.hip) are the known place where this hangs by a thread: they are rows of
never-written HBM scratch times 0, i.e. NaN under three of the four patterns, and nothing may ever read them.  The cases
``[33]`` (31 padding columns) and ``[55, 32, 31, 2, 40]`` (9 .. 62) of the forward are the guard of that.

Order: the one-compute-unit cases first, then teams, then the chain routes with a hand-over."""
import ctypes
import warnings

import pytest
import torch

import test_gpu_edm_loss as LS
import test_gpu_flags as F
import test_gpu_join as J
import test_gpu_metrics as MT
import test_gpu_parity as P
import test_gpu_rmsd as RM
import test_gpu_size_gnn as SG
import test_gpu_size_train as ST
import test_gpu_train as TR
from helpers import POISON_PATTERNS, poisoned_allocations, seeded_state_dict
from oracle import edm_oracle
from size_train_ref import size_batch

pytestmark = pytest.mark.gpu

ALL_FLAGS = dict(attention=True, tanh=True, aggregation_method='mean')


# ---- the harness of every case ---------------------------------------------------------------------------------------------
def bits(v):
    """A value as comparable bits on the host: NaN equals NaN, -0.0 differs from 0.0."""
    t = torch.as_tensor(v).detach().cpu().contiguous()
    if t.is_floating_point():
        t = t.reshape(-1).view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for name in want:
        a, b = got[name], want[name]
        assert type(a) is type(b), f'{what}: {name} is a {type(a).__name__}, the baseline a {type(b).__name__}'
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and a.shape == b.shape, f'{what}: {name}'
        assert torch.equal(bits(a), bits(b)), f'{what}: {name} differs'


def storage_ptr(t):
    return t.untyped_storage().data_ptr()


def product_workspaces(*models):
    """Every cached workspace the product holds right now: those of the given denoisers and the side-stream ones."""
    from difflinker_amd import edm as edm_mod
    found = {}
    for k, dyn in enumerate(models):
        for name in ('_fc_ws', '_large_ws', '_bwd_ws'):
            if getattr(dyn, name, None) is not None:
                found[f'{k}.{name}'] = getattr(dyn, name)
        for key, ws in (getattr(dyn, '_workspaces', None) or {}).items():
            found[f'{k}._workspaces{key}'] = ws
    with edm_mod._CACHE_LOCK:
        for key, ws in edm_mod._SIDE_WORKSPACE.items():
            found[f'side{key}'] = ws
    return found


class Ran:
    """What one run of a case hands back: ``outputs`` (name -> tensor / float, the defined regions), ``buffers`` ([(name, tensor,
    least bytes)]: tensors that must have been poisoned allocations) and ``sizes`` ([(name, bytes, count)]: per-call buffers the
    test cannot reach - at least ``count`` poisoned allocations of exactly ``bytes`` on the device)."""

    def __init__(self, outputs, buffers=(), sizes=()):
        self.outputs = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in outputs.items()}
        self.buffers, self.sizes = list(buffers), list(sizes)


def check_contract(monkeypatch, run):
    """``run()`` builds the case's objects, calls the entry point and returns a ``Ran``.  Once un-patched, once per pattern."""
    from difflinker_amd import edm as edm_mod
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        plain = run()
        torch.cuda.synchronize()
        seen = {}
        for pattern in POISON_PATTERNS:
            with poisoned_allocations(pattern, monkeypatch) as poison:
                ran = run()
                torch.cuda.synchronize()
            ptrs = {r[2]: r[1] for r in poison.records if r[0].type == 'cuda'}
            assert ran.buffers or ran.sizes, 'a case names the buffers it cares about'
            for name, tensor, least in ran.buffers:
                assert tensor is not None and tensor.is_cuda, f'{name}: no such buffer after the call'
                assert tensor.untyped_storage().nbytes() >= least, f'{name}: {tensor.untyped_storage().nbytes()} bytes < {least}'
                assert ptrs.get(storage_ptr(tensor), -1) >= least, f'{name} was not allocated under the patch ({pattern:#010x})'
            for name, nbytes, count in ran.sizes:
                assert nbytes > 0 and sum(1 for v in ptrs.values() if v == nbytes) >= count, f'{name}: no poisoned buffer of {nbytes} bytes'
            seen[pattern] = ran.outputs
            del ran
            with edm_mod._CACHE_LOCK:
                edm_mod._SIDE_WORKSPACE.clear()                   # nothing poisoned outlives its run
    # no warning of the product: a RuntimeWarning (the re-run without teams, the off-sweet-spot batch) or anything raised
    # from this repository; a deprecation notice of a foreign library is not the subject
    ours = [w for w in caught if issubclass(w.category, RuntimeWarning) or 'difflinker_amd' in (w.filename or '')]
    assert not ours, [str(w.message) for w in ours]
    assert_same(seen[POISON_PATTERNS[0]], plain.outputs, 'zero-filled run against the un-patched one')
    for pattern in POISON_PATTERNS[1:]:
        assert_same(seen[pattern], seen[POISON_PATTERNS[0]], f'pattern {pattern:#010x} against the zero-filled run')
    return seen[POISON_PATTERNS[0]]


def on(v):
    return None if v is None else v.to(P.dev())


# ---- a / b. one forward of the fully-connected denoiser ----------------------------------------------------------------------
FWD_SIZES = {'5': ([5], [2]),                                    # one partial tile
             '33': ([33], [5]),                                  # stream_phase with 31 padding columns
             'lds-limit': ([55, 32, 31, 2, 40], [6, 3, 4, 1, 12])}   # the LDS limit; 9, 32, 33, 62 and 24 padding columns


def forward_closure(make, sizes, linkers, nf, team, large=False, seed=11):
    """Make the closure of a forward case (shared with tests/test_gpu_streams.py): ``build()`` makes a fresh denoiser and returns
    it with ``launch(place)``, which puts the inputs on the device through ``place`` and enqueues the launch - no host read
    before it - returning ``(eps_hat, nan_flags)``.  Also returns the host inputs."""
    inp, z, t = P.ragged_inputs(sizes, linkers, nf, seed=seed)

    def build():
        dyn = make()
        dyn.team = team

        def launch(place=on):
            return dyn._launch_forward(place(t), place(z), place(inp['node_mask']), place(inp['linker_mask']), place(inp['edge_mask']),
                                       place(inp['context']), large=large)
        return dyn, launch
    return build, inp, z, t


def forward_case(monkeypatch, make, sizes, linkers, nf, team, large=False, seed=11):
    from difflinker_amd import _lib
    build, inp, z, t = forward_closure(make, sizes, linkers, nf, team, large, seed)
    B, N = z.shape[:2]
    lib = _lib.load()

    def run():
        dyn, launch = build()
        out, flags = launch()
        torch.cuda.synchronize()
        if large:
            ws, need = dyn._large_ws, int(lib.dl_pocket_workspace_bytes(B, N))
        else:
            ws, need = dyn._fc_ws, int(lib.dl_workspace_bytes(B, team))
        assert need > 0
        return Ran({'eps_hat': out, 'nan_flags': flags},
                   [('workspace', ws, need), ('eps_hat', out, 4 * out.numel()), ('nan_flags', flags, 4 * B)])
    got = check_contract(monkeypatch, run)
    assert not bool(got['nan_flags'].any()) and torch.isfinite(got['eps_hat']).all()
    assert float((got['eps_hat'] * (1 - inp['node_mask'].float())).abs().max()) == 0.0, 'padding rows are written, as zeros'
    return got


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
@pytest.mark.parametrize('case', list(FWD_SIZES))
def test_forward_on_one_compute_unit(monkeypatch, case, precision):
    """a. ``dl_egnn_forward_fc_team`` with team 1, L = 2."""
    forward_case(monkeypatch, lambda: P.make_dynamics(8, 1, 2, seed=14, precision=precision)[0], *FWD_SIZES[case], 8, 1)


def test_forward_on_one_compute_unit_f16x2(monkeypatch):
    forward_case(monkeypatch, lambda: P.make_dynamics(8, 1, 2, seed=14, precision='f16x2')[0], *FWD_SIZES['lds-limit'], 8, 1)


def test_forward_on_one_compute_unit_with_attention_tanh_and_mean(monkeypatch):
    forward_case(monkeypatch, lambda: F.make(8, 1, 2, 210, ALL_FLAGS, 'f16x3', 1.0)[0], *FWD_SIZES['lds-limit'], 8, 1)


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_forward_on_the_hbm_resident_kernels(monkeypatch, precision):
    """b. ``dl_egnn_forward_fc_large`` at 56 and 110 atoms."""
    forward_case(monkeypatch, lambda: P.make_dynamics(8, 1, 2, seed=15, precision=precision)[0], [56, 110], [10, 20], 8, 1, large=True)


def test_forward_on_the_hbm_resident_kernels_with_sin_embedding(monkeypatch):
    forward_case(monkeypatch, lambda: F.make(9, 1, 2, 250, dict(sin_embedding=True), 'f16x3', 0.02)[0], [12, 9], [4, 3], 9, 1,
                 large=True)


# ---- c. the radius graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('attention', [False, True], ids=['plain', 'attention'])
def test_forward_on_the_pocket_graph(monkeypatch, attention):
    """c. ``dl_egnn_forward_pocket``: B = 3, 14 fragment + 90 pocket + 5..9 linker atoms (test_flags_on_the_pocket_graph_vs_oracle)."""
    from difflinker_amd import DynamicsWithPockets
    nf, L = 9, 2
    flags = dict(attention=True) if attention else {}
    inp, z, t = P.pocket_inputs(batch=3, n_frag=14, n_pocket=90, linker=(5, 9), nf=nf, seed=241)
    B = z.shape[0]

    def run():
        dyn = DynamicsWithPockets(n_dims=3, in_node_nf=nf, context_node_nf=2, hidden_nf=128, n_layers=L, norm_constant=1e-6,
                                  normalization='batch_norm', graph_type='FC-10A-4A', **flags)
        dyn.load_state_dict(seeded_state_dict(nf + 3, 128, L, 240, coord_gain=0.02, attention=attention), strict=True)
        dyn = dyn.to(P.dev())
        prep = dyn.prepare(on(inp['node_mask']), on(inp['linker_mask']), on(inp['edge_mask']), on(inp['context']))
        out, flags_ = dyn.launch(prep, on(t), on(z))
        torch.cuda.synchronize()
        assert prep['need'] > 0
        return Ran({'eps_hat': out, 'nan_flags': flags_},
                   [('workspace', prep['ws'], prep['need']), ('eps_hat', out, 4 * out.numel()), ('nan_flags', flags_, 4 * B)])
    got = check_contract(monkeypatch, run)
    assert not bool(got['nan_flags'].any()) and torch.isfinite(got['eps_hat']).all()


# ---- g. the linker-size predictor ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn', [False, True], ids=['plain', 'batch_norm'])
def test_size_gnn_inference(monkeypatch, bn):
    in_nf, out_nf, L = 9, 33, 3
    sizes = [5, 64, 33, 17]
    data = SG.to_dev(SG.random_batch(sizes, [0, 0, 4, 2], in_nf, seed=sum(sizes)))

    def run():
        clf, _ = SG.make_classifier(in_nf, out_nf, L, seed=11, bn=bn)
        logits = clf.gnn.predict_logits(data['one_hot'], data['positions'], data['fragment_mask'], data['edge_mask'])
        torch.cuda.synchronize()
        return Ran({'logits': logits}, [('logits', logits, 4 * len(sizes) * out_nf)])
    assert torch.isfinite(check_contract(monkeypatch, run)['logits']).all()


def test_size_gnn_training_forward_and_backward(monkeypatch):
    """``dl_size_train_forward`` + ``dl_size_train_backward`` (the smallest case of test_gpu_size_train.py, BatchNorm on): logits,
    loss, every gradient and the running statistics; the per-call workspace is found by its size."""
    from difflinker_amd import _lib
    sizes, linkers, L, bn, _ = ST.CASES['bn1_ragged']
    data = size_batch(sizes, linkers, ST.IN_NF, seed=sum(sizes), scale=0.9, chain=True)
    B, N = data['positions'].shape[:2]

    def run():
        clf, _ = ST.make_clf(L, bn, seed=700 + L)
        logits, loss, grads = ST.hip_run(clf, data)
        torch.cuda.synchronize()
        need = int(_lib.load().dl_size_train_workspace_bytes(ctypes.byref(clf.gnn._train_args(B, N))))
        out = {'logits': logits, 'loss': loss}
        out.update({'grad.' + k: v for k, v in grads.items()})
        out.update({'buffer.' + k: v for k, v in clf.gnn.named_buffers()})
        n_params = sum(p.numel() for p in clf.gnn.parameters())
        return Ran(out, sizes=[('workspace', need, 1), ('grad_params', 4 * n_params, 1)])
    got = check_contract(monkeypatch, run)
    assert all(torch.isfinite(v).all() for v in got.values())


# ---- h. post-processing ------------------------------------------------------------------------------------------------------
def _bond_batch():
    sizes = [24, 2, 13, 1, 20, 7]
    return MT.chains(len(sizes), 24, sizes, 8, seed=3), sizes


def _written_bonds(found):
    """The bond list with the rows the API leaves unwritten (from n_bonds on) masked out."""
    cap = found.bonds.shape[1]
    written = torch.arange(cap, device=found.bonds.device)[None, :, None] < found.n_bonds[:, None, None]
    return torch.where(written, found.bonds, torch.full_like(found.bonds, -7))


def test_perceive_bonds(monkeypatch):
    """``dl_perceive_bonds``: everything but the tail of the bond list is written whatever the buffers held - ``valence`` 0 and
    ``component`` -1 from the atom count on included (difflinker_hip.h); once more with a capacity that overflows."""
    from difflinker_amd.molecule_builder import perceive_bonds
    (one_hot, x, mask), sizes = _bond_batch()
    B, N = mask.shape[:2]
    unwritten = []                                                   # the list of the one-atom molecule: no bond, nothing written

    def run():
        out, buffers = {}, []
        for tag, cap in (('default', None), ('cut', 3)):
            found = perceive_bonds(on(one_hot), on(x), on(mask), False, capacity=cap)
            torch.cuda.synchronize()
            unwritten.append(found.bonds[3].cpu())
            for name in ('n_bonds', 'valence', 'n_components', 'component', 'status'):
                out[f'{tag}.{name}'] = getattr(found, name)
                buffers.append((f'{tag}.{name}', getattr(found, name), 4 * getattr(found, name).numel()))
            out[f'{tag}.bonds'] = _written_bonds(found)
            buffers.append((f'{tag}.bonds', found.bonds, 4 * found.bonds.numel()))
        return Ran(out, buffers)
    got = check_contract(monkeypatch, run)
    assert got['default.status'].tolist() == [0] * B and got['cut.status'].ne(0).any()
    assert got['default.n_bonds'].tolist()[3] == 0 and int(got['default.n_bonds'].max()) < 4 * N
    # the poison really is in device memory when the kernel starts, and the tail really is left alone: what the API calls
    # unwritten still holds the pattern (runs: un-patched, then the four patterns, two launches each)
    assert len(unwritten) == 2 + 2 * len(POISON_PATTERNS)
    for k, pattern in enumerate(POISON_PATTERNS):
        word = pattern - (1 << 32) if pattern >> 31 else pattern
        for tail in unwritten[2 + 2 * k:4 + 2 * k]:
            assert tail.numel() and bool((tail == word).all()), f'{pattern:#010x}'
    for b, n in enumerate(sizes):
        assert got['default.component'][b, n:].tolist() == [-1] * (N - n) and got['default.valence'][b, n:].tolist() == [0] * (N - n)


def test_molecule_keys(monkeypatch):
    """``dl_molecule_keys`` (through ``analyze``), without and with a drop mask: every output is written in full."""
    from difflinker_amd.metrics import analyze
    (one_hot, x, mask), sizes = _bond_batch()
    B, N = mask.shape[:2]
    drop = mask.clone()
    drop[:, ::3] = 0                                                 # two atoms in three are "pocket"

    def run():
        out, buffers = {}, []
        for tag, dm in (('all', None), ('dropped', drop)):
            got = analyze(on(one_hot), on(x), on(mask), False, drop_mask=on(dm))
            torch.cuda.synchronize()
            for name in ('n_atoms', 'n_over', 'n_components', 'n_bonds', 'key', 'colour', 'status'):
                v = getattr(got, name)
                out[f'{tag}.{name}'] = v
                buffers.append((f'{tag}.{name}', v, v.element_size() * v.numel()))
            out[f'{tag}.bonds'] = _written_bonds(got.bonds)
        return Ran(out, buffers)
    got = check_contract(monkeypatch, run)
    assert got['all.status'].tolist() == [0] * B and got['all.n_atoms'].tolist() == sizes
    for b, n in enumerate(sizes):
        assert got['all.colour'][b, n:].tolist() == [0] * (N - n)


def test_best_rmsd(monkeypatch):
    """``dl_best_rmsd`` on the pairs of test_gpu_rmsd.py, the flagged ones among them (NaN / -1 / their bit: defined too)."""
    cases = RM.build_cases()
    seven = RM.point_sets()['generic'].astype('float32')
    nan_a = seven.copy()
    nan_a[4, 1] = float('nan')
    ident = [list(range(7))]
    extra = [(RM.BAD_AT['no_map'], 7, seven, seven, []), (RM.BAD_AT['nan'], 7, nan_a, seven, ident),
             (RM.BAD_AT['too_large'], RM.N_MAX + 1, seven, seven, ident)]
    pairs = len(cases) + len(extra)

    def run():
        rmsd, best, status = RM.launch(cases, RM.N_MAX, extra)
        return Ran({'rmsd': rmsd, 'best': best, 'status': status}, sizes=[('rmsd, best, status', 4 * pairs, 3)])
    got = check_contract(monkeypatch, run)
    assert int(got['status'].ne(0).sum()) == 3 and int(got['rmsd'].isnan().sum()) == 3 and int((got['best'] == -1).sum()) == 3


# ---- e. the backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ragged', 'sub3_ctx3_centering'])
def test_backward_twice_on_one_model(monkeypatch, case):
    """e. ``dl_egnn_backward_fc`` twice on the same ``Dynamics``: the second call finds the first call's scratch (per-molecule
    partials, the saved activations), so a partial sum that accumulates instead of overwriting shows there."""
    from difflinker_amd import _lib, egnn
    sizes, linkers, nf, ctx, L, S, per_mol_t, centering, trained = TR.CASES[case]
    b, context = TR.batch(sizes, linkers, nf, ctx, seed=7)
    B, N = b['positions'].shape[:2]
    gen = torch.Generator().manual_seed(3)
    z = torch.cat([b['positions'], b['one_hot'] / 4], -1) + 0.5 * torch.randn(B, N, 3 + nf, generator=gen) * b['linker_mask']
    t = torch.rand(B, 1, generator=gen) if per_mol_t else torch.tensor([0.37])
    G = torch.randn(B, N, 3 + nf, generator=gen)
    args = (t, z, b['atom_mask'], None if centering else b['linker_mask'], b['edge_mask'], context, G)

    def run():
        dyn = TR.make_dyn(nf, ctx, L, S, wseed=40 + L + S, trained=trained, centering=centering)
        first = dyn.parameter_grad(*(on(v) for v in args))
        torch.cuda.synchronize()
        ws = dyn._bwd_ws
        second = dyn.parameter_grad(*(on(v) for v in args))
        torch.cuda.synchronize()
        assert dyn._bwd_ws is ws, 'the second call reuses the first call\'s workspace'
        need = int(_lib.load().dl_egnn_backward_fc_workspace_bytes(ctypes.byref(egnn.backward_args(dyn, B, N))))
        assert need > 0
        names = [n for n, _ in dyn.named_parameters()]
        out = {f'first.{k}': v for k, v in zip(names, first)}
        out.update({f'second.{k}': v for k, v in zip(names, second)})
        n_params = sum(p.numel() for p in dyn.parameters())
        return Ran(out, [('workspace', ws, need), ('grad_params', first[0], 4 * n_params), ('grad_params again', second[0], 4 * n_params)])
    got = check_contract(monkeypatch, run)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        if k.startswith('first.'):
            assert torch.equal(v, got['second.' + k[6:]]), f'{k[6:]}: the second call on the used workspace gives other bits'


# ---- d. the fused chain, route 'one' (one compute unit per molecule, one launch) ----------------------------------------------
CHAIN_T, KEEP = 20, 2          # T = 20: the smallest at which EDM considers the hand-over plan


def chain_closure(make, sizes, linkers, nf, route, split=None, inpainting=False, T=CHAIN_T):
    """Make the closure of a chain case (shared with tests/test_gpu_streams.py): ``build()`` makes a fresh EDM and returns it with
    ``sample(place, place_bank)``: ``EDM.sample_chain`` from a fixed noise bank and once more with Philox draws, the inputs put on
    the device through ``place`` (the bank through ``place_bank``; None: handed over on the host).  Returns both chains and the
    flag / step arrays the fused launches reported (none on the host-driven loops, where no exception means no flag)."""
    inp, _, _ = P.ragged_inputs(sizes, linkers, nf, seed=172)
    B, N = inp['x'].shape[:2]
    if inpainting:
        g0 = torch.Generator().manual_seed(173)
        bank = (torch.randn(1 + 2 * T + 2, B, N, 3, generator=g0), torch.randn(1 + 2 * T + 2, B, N, nf, generator=g0))
    else:
        bank = edm_oracle.NoiseBank.generate(T, B, N, 3, nf, seed=173).stacked()

    def build():
        edm = make(T)
        if split is not None:
            edm.split_chain = split

        def sample(place=on, place_bank=None):
            g = {k: place(v) for k, v in inp.items()}
            if inpainting:
                args = (g['x'], g['h'], g['node_mask'], g['edge_mask'], g['fragment_mask'], g['linker_mask'], g['context'])
            else:
                args = (g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'], g['context'])
            noise = bank if place_bank is None else tuple(place_bank(v) for v in bank)
            reported = []
            raise_on = edm._raise_on_chain_flags
            edm._raise_on_chain_flags = lambda f, s: (reported.append((f.clone(), s.clone())), raise_on(f, s))[1]
            out = {}
            for source in ('bank', 'philox'):
                edm.last_route = None
                if source == 'philox':
                    edm.noise_source, edm.noise_seed = 'philox', 9
                try:
                    out[f'chain.{source}'] = edm.sample_chain(*args, keep_frames=KEEP, noise_bank=noise if source == 'bank' else None)
                    torch.cuda.synchronize()
                finally:
                    assert edm.last_route == route, (edm.last_route, route)
            for k, (f, s) in enumerate(reported):
                out[f'nan_flags.{k}'], out[f'nan_step.{k}'] = f, s
            return out
        return edm, sample
    return build


def chain_case(monkeypatch, make, sizes, linkers, nf, route, split=None, inpainting=False, expect=(), T=CHAIN_T):
    """Check a chain case: ``expect(edm)`` names the workspaces the route must have used as ``[(key of product_workspaces, least
    bytes)]``."""
    build = chain_closure(make, sizes, linkers, nf, route, split, inpainting, T)

    def run():
        edm, sample = build()
        out = sample()
        held = product_workspaces(edm.dynamics)
        want = list(expect(edm)) if callable(expect) else list(expect)
        assert held and want
        buffers = [(name, ws, 1) for name, ws in held.items()]
        for name, least in want:
            assert name in held, (name, sorted(held))
            buffers.append((name, held[name], least))
        return Ran(out, buffers)
    got = check_contract(monkeypatch, run)
    assert all(torch.isfinite(v).all() for k, v in got.items() if k.startswith('chain.'))
    assert not any(bool(v.any()) for k, v in got.items() if k.startswith('nan_flags.'))
    return got


def _fc_edm(L, seed, team=1, precision='f16x3', flags=None):
    def make(T):
        dyn, _, _ = J._model(precision, seed, L, flags)
        dyn.team = team
        return J._edm(dyn, J.NF, T)
    return make


def _ws_bytes(B, team):
    from difflinker_amd import _lib
    return int(_lib.load().dl_workspace_bytes(int(B), int(team)))


def test_chain_in_one_launch(monkeypatch):
    """d. route 'one': ``dl_sample_chain_fc`` on one compute unit per molecule (``split_chain`` off)."""
    chain_case(monkeypatch, _fc_edm(2, 301), J.SIZES, J.LINKERS, J.NF, 'one', split=False,
               expect=[('0._fc_ws', _ws_bytes(len(J.SIZES), 1))])


# ---- a. the forward on teams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
@pytest.mark.parametrize('case', list(FWD_SIZES))
@pytest.mark.parametrize('team', [2, 4, 8])
def test_forward_on_teams(monkeypatch, team, case, precision):
    """a. ``dl_egnn_forward_fc_team`` with teams of 2, 4 and 8 compute units: the exchange rows and arrival words of the
    workspace, the flags the members OR their bits into."""
    forward_case(monkeypatch, lambda: P.make_dynamics(8, 1, 2, seed=14, precision=precision)[0], *FWD_SIZES[case], 8, team)


@pytest.mark.parametrize('team', [2, 8])
def test_forward_on_teams_f16x2_and_with_attention_tanh_and_mean(monkeypatch, team):
    forward_case(monkeypatch, lambda: P.make_dynamics(8, 1, 2, seed=14, precision='f16x2')[0], *FWD_SIZES['lds-limit'], 8, team)
    forward_case(monkeypatch, lambda: F.make(8, 1, 2, 210, ALL_FLAGS, 'f16x3', 1.0)[0], *FWD_SIZES['lds-limit'], 8, team)


# ---- f. the loss, e. its backward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['fc', 'pocket'])
def test_loss_rows_and_terms(monkeypatch, tag):
    """f. ``EDM.forward``: prologue (``z_t``, ``t``, gamma), the denoiser with the product's default team size, epilogue rows;
    fixed ``t_int`` with 0 and T among them, fixed noise (the golden cases of test_gpu_edm_loss.py)."""
    edm0, g = LS.golden_case(tag)
    B, T = g['x'].shape[0], int(edm0.T)
    del edm0
    assert B >= 3

    def run():
        edm, _ = LS.golden_case(tag)
        t_int = torch.tensor(([0, T, T // 2, 1, T - 1] * B)[:B], device=LS.DEV)
        with torch.no_grad():
            rows, t_dev = edm._loss_rows(g['x'], g['h'], g['node_mask'], g['fragment_mask'], g['linker_mask'], g['edge_mask'],
                                         g['context'], t_int, (g['noise_x'], g['noise_h']), 0)
            terms = edm._reduce_loss_rows(rows, t_dev)
        torch.cuda.synchronize()
        out = {'rows': rows, 't_int': t_dev}
        out.update(dict(zip(LS.NAMES, terms)))
        held = product_workspaces(edm.dynamics)
        assert held, 'the denoiser of the loss works in a cached workspace'
        return Ran(out, [('rows', rows, 4 * rows.numel())] + [(name, ws, 1) for name, ws in held.items()])
    got = check_contract(monkeypatch, run)
    assert torch.isfinite(got['rows']).all() and got['t_int'].tolist()[:2] == [0, T]


def test_training_forward_and_loss_backward(monkeypatch):
    """e. ``EDM.training_forward(...)[4].backward()``: the 7 terms and every parameter gradient (``dl_edm_loss_grad`` +
    ``dl_egnn_backward_fc`` behind the forward's kernels)."""
    nf = 8
    g, ctx = TR.edm_inputs([11, 16, 9, 13], [4, 5, 3, 4], nf, seed=6)
    B, N = g['positions'].shape[:2]
    t_int = torch.tensor([0, 120, 260, 500], device=TR.DEV)
    gen = torch.Generator().manual_seed(2)
    noise = (torch.randn(B, N, 3, generator=gen).to(TR.DEV), torch.randn(B, N, nf, generator=gen).to(TR.DEV))

    def run():
        edm = TR.make_edm(nf, 1, 1, 2, 33)
        edm.dynamics.zero_grad()
        terms = edm.training_forward(*TR.edm_args(g, ctx), t_int=t_int, noise=noise)
        terms[4].backward()
        torch.cuda.synchronize()
        out = dict(zip(LS.NAMES, terms))
        out.update({'grad.' + k: p.grad for k, p in edm.dynamics.named_parameters()})
        held = product_workspaces(edm.dynamics)
        assert '0._bwd_ws' in held and '0._fc_ws' in held
        return Ran(out, [(name, ws, 1) for name, ws in held.items()])
    got = check_contract(monkeypatch, run)
    assert all(torch.isfinite(torch.as_tensor(v)).all() for v in got.values())


# ---- d. the fused chain: teams beside the main launch, the two hand-overs, the split by size, inpainting ------------------------
def test_chain_with_overflow_teams(monkeypatch):
    """d. route 'overflow_teams': (compute units + 3) molecules of about 10 atoms; the three beyond one per compute unit are
    sampled by teams of four in a launch on the side stream, whose workspace and flag arrays are the side launch's own."""
    from difflinker_amd import _lib
    cus = torch.cuda.get_device_properties(P.dev()).multi_processor_count
    B = cus + 3
    sizes = torch.randint(4, 13, (B,), generator=torch.Generator().manual_seed(5)).tolist()
    linkers = [max(1, s // 4) for s in sizes]
    index = P.dev().index

    def expect(edm):
        assert edm.overflow_teams and int(_lib.load().dl_team_max(3)) >= 4
        return [('0._fc_ws', _ws_bytes(cus, 1)), (f"side{(index, 'teams')}", _ws_bytes(3, 4))]
    chain_case(monkeypatch, _fc_edm(1, 71, team='auto'), sizes, linkers, J.NF, 'overflow_teams', expect=expect)


def test_chain_in_two_launches(monkeypatch):
    """d. route 'two_launch': four molecules resume from ``z_state`` on teams of two behind the first launch (a batch whose
    join_plan is None by itself: too few finished molecules to help)."""
    from difflinker_amd import edm as edm_mod
    sizes, linkers = J.SIZES[:6], J.LINKERS[:6]
    cus = torch.cuda.get_device_properties(P.dev()).multi_processor_count
    plan = edm_mod.split_plan(sizes, linkers, CHAIN_T + 1, cus, 2, 2)
    assert plan is not None and edm_mod.join_plan(sizes, linkers, CHAIN_T + 1, cus, 2, 2) is None
    chain_case(monkeypatch, _fc_edm(2, 171), sizes, linkers, J.NF, 'two_launch', split=True,
               expect=[('0._fc_ws', _ws_bytes(len(sizes), 1)), (f"side{(P.dev().index, 'teams')}", _ws_bytes(len(plan[1]), 2))])


@pytest.mark.parametrize('variant', ['f16x3', 'fp32', 'attention-tanh-mean'])
def test_chain_with_the_join_hand_over(monkeypatch, variant):
    """d. route 'join': ``dl_sample_chain_fc_join``, six teams formed inside one launch; exchange buffers, arrival and join words
    of the join workspace, ``z_state``."""
    from difflinker_amd import _lib, edm as edm_mod
    cus = torch.cuda.get_device_properties(P.dev()).multi_processor_count
    plan = edm_mod.join_plan(J.SIZES, J.LINKERS, CHAIN_T + 1, cus, 2, 2)
    assert plan is not None
    need = int(_lib.load().dl_join_workspace_bytes(len(plan[1])))
    make = _fc_edm(2, 361, flags=ALL_FLAGS) if variant == 'attention-tanh-mean' else _fc_edm(2, 301, precision=variant)
    chain_case(monkeypatch, make, J.SIZES, J.LINKERS, J.NF, 'join', split=True,
               expect=[('0._fc_ws', _ws_bytes(len(J.SIZES), 1)),
                       (f"side{(P.dev().index, 'join', torch.cuda.current_stream(P.dev()).cuda_stream)}", need)])


def test_chain_split_by_size(monkeypatch):
    """d. small, 56..110-atom and bigger molecules in one batch: the fused chain on teams for the first two classes (its last
    part's route is 'one': a team launch has no hand-over), the host-driven loop over the HBM-resident kernels for the third."""
    def make(T):
        dyn, _, _ = P.make_dynamics(J.NF, 1, 1, seed=33)
        dyn.team = 'auto'
        return J._edm(dyn, J.NF, T)
    chain_case(monkeypatch, make, [20, 70, 35, 120, 12, 56], [4, 9, 5, 8, 3, 6], J.NF, 'one',
               expect=[('0._fc_ws', 1), ('0._large_ws', 1)])


def _inpainting_edm(T):
    from difflinker_amd import Dynamics, InpaintingEDM
    nf, L = J.NF, 1
    dyn = Dynamics(n_dims=3, in_node_nf=nf, context_node_nf=1, hidden_nf=128, n_layers=L, norm_constant=1e-6,
                   normalization='batch_norm', centering=True)
    dyn.load_state_dict(seeded_state_dict(nf + 2, 128, L, 81), strict=True)
    edm = InpaintingEDM(dyn.to(P.dev()), in_node_nf=nf, n_dims=3, timesteps=500, noise_schedule='polynomial_2',
                        noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10]).to(P.dev())
    edm.T = T
    return edm


def test_inpainting_chain(monkeypatch):
    """d. ``InpaintingEDM.sample_chain``: the host-driven loop (denoiser on teams + the fused tail per step); it launches no
    fused chain, so ``last_route`` stays None."""
    chain_case(monkeypatch, _inpainting_edm, [12, 33, 10], [4, 6, 3], J.NF, None, inpainting=True, expect=[('0._fc_ws', 1)])
