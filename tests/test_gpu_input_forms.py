"""The input contract of every Python entry point ("What a tensor argument may look like"): A CALL'S RESULT IS A
FUNCTION OF THE VALUES OF ITS TENSOR ARGUMENTS ALONE - NOT OF THEIR STRIDES, THEIR STORAGE OFFSET OR THEIR (EXACT) DTYPE - AND NO
CALL WRITES TO ITS ARGUMENTS.  A wrapper turns tensors into raw pointers and from then on the kernel assumes dense fp32 / int32 /
int8 rows at that address; every other GPU test hands over freshly made, dense, zero-offset tensors of the canonical dtype.

Every part-A case of tests/test_gpu_streams.py (``BUILDERS[case](monkeypatch)`` returns ``run(place)``, which puts every input
on the device through ``place``) runs once with ``place`` = the canonical form and once per other form of tests/input_forms.py
(strided, sliced, wide, squeezed), on fresh objects.  The outputs must have the same names, dtypes, shapes and BITS; every placed
buffer - the poison in the gaps and around a slice included - must be bit-identical to the copy taken before the call; no
warning of the product.  ``NOT_APPLICABLE`` and ``REFUSES`` (input_forms.py) bound what a case may do instead.

Four stream cases ('aromatic', 'fragment-cuts', 'multi-cuts', 'pocket-select') call the C entry point with raw pointers, as
'forward-c-abi' does; the C ABI is dense by definition, so here the SAME batches go through the Python wrappers those entry
points have (``OVERRIDES``), and every key of ``DRIVES`` but 'forward-c-abi' still runs under every form.  Added: ``fingerprints``
and ``tanimoto_nearest`` (not in ``DRIVES``), ``training_forward`` and ``parameter_grad`` of both denoisers called directly, a
``Bonds`` whose members are re-formed one kind at a time into every wrapper that takes one (it never passes through ``place`` in
the stream cases), and a stride-0 ``t``.

LOADS WIDER THAN 4 BYTES FROM A CALLER'S POINTER (re-read in csrc/ before the ``sliced`` form - a pointer aligned to its item
size and nothing more - first ran; workspaces, packed weights, the Python layer's own converted copies and LDS not counted):
  * ``dl_tanimoto_nearest``: ``a_bits`` and ``b_bits`` as ``uint4`` (fingerprint.hip, ``tanimoto_kernel``).  The C entry point
    refuses a pointer that is not 16-byte aligned (``DL_ERR_BAD_ARG``, stated in the header); ``metrics.tanimoto_nearest``
    hands it an aligned copy (one ``clone()``) when ``data_ptr() % 16 != 0``;
  * ``dl_pocket_select``: ``ligand_x`` as ``double`` (pocket.hip) - 8 bytes, the item size of the float64 tensor it comes from,
    so every view of one is aligned;
  * ``dl_molecule_keys`` WRITES 64-bit ``key`` / ``colour`` and ``dl_tanimoto_nearest`` ``sum_q20``: outputs the wrappers allocate.
Every other ``float4`` / ``uint4`` / ``float2`` access, LDS-DMA and buffer load in csrc/ is on packed weight images, on
workspaces (the 4-float coordinate rows ``X`` / ``X0`` of egnn_sparse.hip and egnn_backward_sparse.hip, the team rows and
partials of egnn_fc.hip, the activations that ``mm64`` / ``mmT`` of size_gnn_train.hip multiply with the flat parameter copy) or
on LDS (egnn_backward.hip, rmsd.hip, clash.hip); the kernels read ``xh``, masks, noise, bond lists and counts one element at a time."""
import warnings

import numpy as np
import pytest
import torch

import input_forms as IF
import test_gpu_aromatic as AR
import test_gpu_fingerprint as FP
import test_gpu_fragment as FR
import test_gpu_multicut as MC
import test_gpu_parity as P
import test_gpu_pocket_train as PT
import test_gpu_scratch as S
import test_gpu_streams as GS
import test_gpu_train as TR
from input_forms import NOT_APPLICABLE, REFUSES, UNDER_TEST
from test_gpu_scratch import assert_same
from test_gpu_streams import on_host

pytestmark = pytest.mark.gpu


def _fields(got):
    return {name: getattr(got, name) for name in got._fields if torch.is_tensor(getattr(got, name))}


# ---- the stream cases that go to the C entry point: the same batches through the Python wrappers ----------------------------------
def _aromatic(mp):
    from difflinker_amd.molecule_builder import Bonds, refine_bond_orders
    batch = AR.pack([AR.mol(AR.ar.hand_molecule(name)) for name in sorted(AR.ar.HAND)] + [AR.mol(([], [], []))], 16,
                    rng=np.random.default_rng(0))

    def run(place):
        found = Bonds(place(batch['n_in'], torch.int32), place(batch['bonds'], torch.int32), None, None, None,
                      place(batch['status'], torch.int32))
        refined, aromatic = refine_bond_orders(found, place(batch['one_hot']), place(batch['x']), place(batch['mask']), False,
                                               place(batch['drop']), place(batch['mark']))
        out = {'aromatic.' + k: v for k, v in _fields(aromatic).items()}
        out.update(bonds=refined.bonds, valence=refined.valence)       # (the whole list: the order of every entry is written)
        return out
    return run


def _cuts(wrapper, batch, capacity, **rule):
    def make(mp):
        from difflinker_amd import fragment

        def run(place):
            return _fields(getattr(fragment, wrapper)(
                place(batch['one_hot']), place(batch['mask']), place(batch['bonds'], torch.int32), place(batch['n_in'], torch.int32),
                charge=place(batch['charge'], torch.int32), status=place(batch['status'], torch.int32), is_geom=False,
                capacity=capacity, **rule))
        return run
    return make


def _pocket_select(mp):
    from difflinker_amd.pocket import select_pockets
    case = GS._pocket_case()
    names = ('protein_x', 'protein_group', 'protein_offset', 'pair_protein', 'ligand_x', 'ligand_mask')
    dtypes = (torch.float32, torch.int32, torch.int32, torch.int32, torch.float64, torch.float32)
    return lambda place: _fields(select_pockets(*(place(case[k], d) for k, d in zip(names, dtypes)), capacity=300))


OVERRIDES = {
    'aromatic': _aromatic,
    'fragment-cuts': lambda mp: _cuts('fragment_cuts', FR.hand_batch()[1], 8)(mp),
    'multi-cuts': lambda mp: _cuts('multi_cuts', MC.random_batch(MC.RANDOM_CASES[1][0]), MC.RANDOM_CASES[1][2],
                                   **MC.RANDOM_CASES[1][1])(mp),
    'pocket-select': _pocket_select,
}


# ---- fingerprints and their similarity: not in DRIVES -------------------------------------------------------------------------------
def _fingerprints(mp):
    """``metrics.fingerprints`` on the mixed batch of test_gpu_fingerprint.py (the call of its wrapper test)."""
    from difflinker_amd.metrics import fingerprints
    from difflinker_amd.molecule_builder import Bonds
    batch = FP.build_mixed()[1]

    def run(place):
        found = Bonds(place(batch['n_in'], torch.int32), place(batch['bonds'], torch.int32), None, None, None,
                      place(batch['status'], torch.int32))
        return _fields(fingerprints(place(batch['one_hot']), place(batch['mask']), found, place(batch['drop']),
                                    place(batch['centre']), radius=3, n_bits=1024))
    return run


def _tanimoto(mp):
    """``metrics.tanimoto_nearest`` on the seven groups of test_gpu_fingerprint.py, W = 32."""
    from difflinker_amd.metrics import tanimoto_nearest
    a, b, a_off, b_off = FP.grouped_case(np.random.default_rng(300), 32)
    return lambda place: _fields(tanimoto_nearest(place(a.view(np.int32), torch.int32), place(b.view(np.int32), torch.int32),
                                                  place(np.asarray(a_off), torch.int32), place(np.asarray(b_off), torch.int32)))


def _clashes_shared(mp):
    """``analyze_clashes`` with everything it takes: the batch of the 'clashes' stream case, a shared ``protein`` list of 257
    atoms (test_gpu_clash.test_shared_target_list) and the caller's own ``thresholds`` table."""
    from difflinker_amd import const
    from difflinker_amd.metrics import analyze_clashes
    x, one_hot, qm, tm = GS._clash_batch()
    rng = np.random.default_rng(257)
    px = (50.0 + rng.uniform(0, 20.0, size=(257, 3))).astype(np.float32)
    pt = rng.integers(0, one_hot.shape[2], size=257).astype(np.int32)
    table = const.clash_threshold_table(True)
    return lambda place: _fields(analyze_clashes(place(one_hot), place(x), place(qm), place(tm),
                                                 protein=(place(px), place(pt, torch.int32)), thresholds=place(table)))


def _grads(dyn, a, G):
    out = {'training_forward': dyn.training_forward(*a)}
    out.update({'grad.' + k: g for (k, _), g in zip(dyn.named_parameters(), dyn.parameter_grad(*a, G))})
    return out


def _parameter_grad(mp):
    """``Dynamics.training_forward`` and ``Dynamics.parameter_grad`` called directly (in the 'train-*' cases ``t``, ``xh`` and
    ``grad_out`` are made inside ``EDM.training_forward``): the 'ragged' case of test_gpu_train.py."""
    sizes, linkers, nf, ctx, L, sub = TR.CASES['ragged'][:6]
    b, context = TR.batch(sizes, linkers, nf, ctx, seed=7)
    B, N = b['positions'].shape[:2]
    gen = torch.Generator().manual_seed(3)
    z = torch.cat([b['positions'], b['one_hot'] / 4], -1) + 0.5 * torch.randn(B, N, 3 + nf, generator=gen) * b['linker_mask']
    t, G = torch.rand(B, 1, generator=gen), torch.randn(B, N, 3 + nf, generator=gen)
    dyn = TR.make_dyn(nf, ctx, L, sub, wseed=40 + L + sub)
    return lambda place: _grads(dyn, [place(v) for v in (t, z, b['atom_mask'], b['linker_mask'], b['edge_mask'], context)], place(G))


def _parameter_grad_pocket(mp):
    """The same of ``DynamicsWithPockets``: the smallest case of test_gpu_pocket_train.py."""
    dyn, inp, z, t, G = PT.case_inputs('far_pocket_atom')
    return lambda place: _grads(dyn, [place(v) for v in (t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'],
                                                         inp['context'])], place(G))


ADDED = {'fingerprints': _fingerprints, 'tanimoto': _tanimoto, 'clashes-shared': _clashes_shared, 'parameter-grad': _parameter_grad,
         'parameter-grad-pocket': _parameter_grad_pocket}
CASES = [case for case in GS.DRIVES if case not in NOT_APPLICABLE] + list(ADDED)


def builder(case):
    return OVERRIDES.get(case) or ADDED.get(case) or GS.BUILDERS[case]


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
def check_input_form(make, case, form):
    """``make()`` builds the case's objects and returns ``run(place)``.  Returns the baseline's outputs."""
    dev = P.dev()
    refused = {k: piece for (c, f, _), (at, piece) in REFUSES.items() if (c, f) == (case, form) for k in at}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        rec = GS.Recorder(dev)
        base = on_host(make()(rec.place))                                # 1. canonical, fresh objects
        torch.cuda.synchronize()
        assert rec.seen, 'a case places the inputs its entry point reads'
        if refused:                                                      # the docstring fixes the dtype: a ValueError that names it
            placer = IF.FormPlace(dev, rec.seen, form, case, GS.host)
            with pytest.raises(ValueError, match='|'.join(sorted(set(refused.values())))):
                make()(placer.place)
            torch.cuda.synchronize()
            placer.assert_untouched()
        placer = IF.FormPlace(dev, rec.seen, form, case, GS.host, canonical_at=refused)
        got = on_host(make()(placer.place))                              # 2. the form, fresh objects
        torch.cuda.synchronize()
    assert placer.k == len(rec.seen), 'the second run placed fewer inputs than the first'
    assert len(rec.seen) == sum(IF.PLACES[case][1].values()), f'{case} placed {len(rec.seen)} inputs, PLACES says {IF.PLACES[case][1]}'
    changed = sum(1 for t, h in zip(placer.placed, rec.seen)
                  if t.dtype != h.dtype or t.shape != h.shape or not t.is_contiguous() or t.storage_offset())
    print(f'[input forms] {case} under {form}: {len(rec.seen)} placed inputs, {changed} of them in another form')
    ours = GS.product_warnings(caught)
    assert not ours, ours                                                # 5.
    assert_same(got, base, f'{case} under {form} against canonical')     # 3.
    placer.assert_untouched()                                            # 4.
    return base, changed


@pytest.mark.parametrize('form', UNDER_TEST)
@pytest.mark.parametrize('case', CASES)
def test_entry_point_takes_the_form(monkeypatch, case, form):
    base, changed = check_input_form(lambda: builder(case)(monkeypatch), case, form)
    if form != 'squeezed' or case in IF.SQUEEZE:
        assert changed, 'the form changed no input: the case tests nothing'
    assert any(torch.is_tensor(v) and v.numel() for v in base.values())


def test_the_callers_threshold_table_is_used():
    """The values behind the 'clashes-shared' case: the default table handed over as ``thresholds`` gives the default's bits, and
    a table of zeros - no pair clashes - is really read."""
    from difflinker_amd import const
    from difflinker_amd.metrics import analyze_clashes
    dev = P.dev()
    x, one_hot, qm, tm = (torch.from_numpy(v).to(dev) for v in GS._clash_batch())
    table = const.clash_threshold_table(True).to(dev)
    default = on_host(_fields(analyze_clashes(one_hot, x, qm, tm)))
    assert_same(on_host(_fields(analyze_clashes(one_hot, x, qm, tm, thresholds=table))), default, 'the default table, handed over')
    none = analyze_clashes(one_hot, x, qm, tm, thresholds=torch.zeros_like(table))
    assert int(default['n_clashes'].sum()) > 0 and int(none.n_clashes.sum()) == 0


def test_the_c_abi_case_is_the_only_one_left_out():
    assert set(CASES) == (set(GS.DRIVES) - NOT_APPLICABLE) | set(ADDED) and NOT_APPLICABLE <= set(GS.DRIVES)
    assert all(case in CASES for case, _, _ in REFUSES)


def test_the_poison_is_what_a_dense_reader_sees():
    """The control of the forms on the device: reading ``numel`` dense elements at ``data_ptr()`` - what a kernel does - gives
    the values for the canonical form and for the sliced one (whose pointer is aligned to 4 bytes only, between two poisoned
    elements) and something else for the strided and the wide one."""
    dev = P.dev()
    h = torch.arange(1, 25, dtype=torch.float32).reshape(2, 4, 3)
    for form in ('canonical', 'strided', 'sliced', 'wide'):
        t = IF.BY_NAME[form](h, dev)
        buf = IF.buffer_of(t)
        offset = (t.data_ptr() - buf.data_ptr()) // 4
        dense = buf.reshape(-1).view(torch.float32)[offset:offset + h.numel()].cpu()
        assert torch.equal(t.cpu().to(torch.float32), h)
        assert torch.equal(dense, h.reshape(-1)) == (form in ('canonical', 'sliced')), form
        if form == 'sliced':
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            assert buf[0].isnan() and buf[-1].isnan() and buf.numel() == h.numel() + 2
        if form == 'strided':
            assert dense[1::2].isnan().all()


# ---- a Bonds of the caller's own --------------------------------------------------------------------------------------------------------
COUNTS = ('n_bonds', 'status', 'valence', 'n_components')
REFORMS = ('bonds-capacity-slice', 'bonds-int64', 'counts-strided', 'counts-sliced', 'counts-int64')


@pytest.fixture(scope='module')
def perceived():
    """``perceive_bonds`` on the batch of test_gpu_scratch.py, once: the inputs on the device and the canonical ``Bonds``."""
    from difflinker_amd.molecule_builder import perceive_bonds
    (one_hot, x, mask), _ = S._bond_batch()
    one_hot, x, mask = (v.to(P.dev()) for v in (one_hot, x, mask))
    found = perceive_bonds(one_hot, x, mask, False)
    torch.cuda.synchronize()
    assert int(found.n_bonds.max()) > 8 and found.status.tolist() == [0] * found.status.numel()
    return one_hot, x, mask, found


def reformed(found, how):
    """``found`` with members re-formed; returns it with the ``(buffer, bit copy)`` pairs of the new members."""
    dev, keep, new = found.bonds.device, [], {}

    def held(t):
        keep.append((IF.buffer_of(t), IF.as_bytes(IF.buffer_of(t)).clone()))
        return t
    if how == 'bonds-capacity-slice':                                    # a list cut to a smaller capacity: wider[:, :capacity]
        h = found.bonds.cpu()
        B, cap = h.shape[:2]
        wider = IF.poison_(torch.empty((B, 2 * cap, 3), dtype=h.dtype))
        wider[:, :cap] = h
        new['bonds'] = held(wider.to(dev)[:, :cap])
        assert not new['bonds'].is_contiguous()
    elif how == 'bonds-int64':                                           # what torch.tensor(rows) makes
        new['bonds'] = held(found.bonds.cpu().to(torch.int64).to(dev))
    else:
        form = {'counts-strided': IF.strided, 'counts-sliced': IF.sliced, 'counts-int64': IF.wide}[how]
        for name in COUNTS:
            new[name] = held(form(getattr(found, name).cpu(), dev))
    for name, t in new.items():
        assert torch.equal(t.cpu().long(), getattr(found, name).cpu().long())
    return found._replace(**new), keep


def _with_bonds(got, found):
    out = _fields(got)
    if hasattr(got, 'bonds') and not torch.is_tensor(got.bonds):
        assert got.bonds is found, 'the Bonds inside the result is the caller\'s object'
    return out


def _call_keys(found, one_hot, x, mask):
    from difflinker_amd.metrics import molecule_keys
    return _with_bonds(molecule_keys(one_hot, mask, found, False), found)


def _call_rings(found, one_hot, x, mask):
    from difflinker_amd.metrics import ring_scores
    return _with_bonds(ring_scores(mask, found), found)


def _call_fingerprints(found, one_hot, x, mask):
    from difflinker_amd.metrics import fingerprints
    return _fields(fingerprints(one_hot, mask, found, radius=2, n_bits=512))


def _call_refine(found, one_hot, x, mask):
    from difflinker_amd.molecule_builder import refine_bond_orders
    refined, aromatic = refine_bond_orders(found, one_hot, x, mask, False)
    out = {'aromatic.' + k: v for k, v in _fields(aromatic).items()}
    out.update(bonds=S._written_bonds(refined), valence=refined.valence)
    return out


def _call_cuts(found, one_hot, x, mask):
    from difflinker_amd.fragment import fragment_cuts
    return _fields(fragment_cuts(one_hot, mask, found.bonds, found.n_bonds, is_geom=False, capacity=8, status=found.status,
                                 min_linker=1, min_fragment=1, min_path_atoms=1, linker_leq_frags=False))


def _call_multicuts(found, one_hot, x, mask):
    from difflinker_amd.fragment import multi_cuts
    return _fields(multi_cuts(one_hot, mask, found.bonds, found.n_bonds, is_geom=False, capacity=8, status=found.status,
                              min_linker=1, min_fragment=1, max_atoms=256, min_rings=0))


TAKES_BONDS = {'molecule_keys': _call_keys, 'ring_scores': _call_rings, 'fingerprints': _call_fingerprints,
               'refine_bond_orders': _call_refine, 'fragment_cuts': _call_cuts, 'multi_cuts': _call_multicuts}


@pytest.mark.parametrize('how', REFORMS)
@pytest.mark.parametrize('wrapper', list(TAKES_BONDS))
def test_a_bonds_of_the_callers_own(perceived, wrapper, how):
    """``found`` as a caller may have built it - the list a capacity slice of a longer one or int64 (``torch.tensor(rows)``), the
    counts strided, sliced or int64 - gives the bits of the ``Bonds`` ``perceive_bonds`` returned, and is left as it was."""
    one_hot, x, mask, found = perceived
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        base = on_host(TAKES_BONDS[wrapper](found, one_hot, x, mask))
        mine, keep = reformed(found, how)
        got = on_host(TAKES_BONDS[wrapper](mine, one_hot, x, mask))
        torch.cuda.synchronize()
    ours = GS.product_warnings(caught)
    assert not ours, ours
    assert_same(got, base, f'{wrapper} on {how} against the canonical Bonds')
    for k, (buf, copy) in enumerate(keep):
        assert torch.equal(IF.as_bytes(buf), copy), f'{wrapper} wrote to re-formed member {k} of {how} or around it'
    assert int(base['n_bonds'].sum() if 'n_bonds' in base else base['n_on'].sum() if 'n_on' in base else base['valence'].sum()) > 0


# ---- a stride-0 input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes, linkers', [([33], [5]), ([20, 33, 9], [4, 6, 2])], ids=['[33]', '[20,33,9]'])
def test_an_expanded_t(sizes, linkers):
    """``t = torch.tensor([[0.37]]).expand(B, 1)`` - every stride 0 - into ``Dynamics.forward`` and ``Dynamics.parameter_grad``
    gives the bits of the same values dense, and still holds them afterwards."""
    dev = P.dev()
    nf = GS.NF
    inp, z, _ = P.ragged_inputs(sizes, linkers, nf, seed=11)
    B = z.shape[0]
    G = torch.randn(z.shape, generator=torch.Generator().manual_seed(5))
    one = torch.tensor([[0.37]], device=dev)
    a = [v.to(dev) for v in (z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'])]

    def run(t):
        dyn = TR.make_dyn(nf, 1, 2, 2, wseed=44)
        out = {'forward': dyn.forward(t, *a)}
        out.update({'grad.' + k: g for (k, _), g in zip(dyn.named_parameters(), dyn.parameter_grad(t, *a, G.to(dev)))})
        return on_host(out)
    expanded = one.expand(B, 1)
    assert expanded.stride(0) == 0 or B == 1
    base, got = run(torch.full((B, 1), 0.37, device=dev)), run(expanded)
    torch.cuda.synchronize()
    assert_same(got, base, 'an expanded t against a dense one')
    assert float(one) == float(torch.tensor(0.37)) and torch.isfinite(base['forward']).all()
