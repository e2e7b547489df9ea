"""The completeness guard of tests/test_gpu_input_forms.py, and the forms and the ``Bonds`` normaliser themselves on CPU tensors.
Runs without a GPU: a public wrapper cannot gain a tensor parameter, and the GPU suite cannot lose a case or gain an exemption,
without a test failing here."""
import importlib
import inspect

import pytest
import torch

import input_forms as IF
import test_gpu_input_forms as GF
import test_gpu_streams as GS

CPU = torch.device('cpu')
SAMPLES = {
    'positions': torch.randn(3, 5, 3, generator=torch.Generator().manual_seed(0)),
    'mask3': (torch.arange(15).reshape(3, 5, 1) % 3 != 0).float(),
    'mask2': (torch.arange(15).reshape(3, 5) % 2).float(),
    'counts': torch.tensor([4, 0, 7], dtype=torch.int32),
    'edge': torch.tensor([0, -1, -2, 0], dtype=torch.int8),
    'maps': torch.arange(12, dtype=torch.int16),
    'ligand': torch.randn(2, 4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)),
    't_int': torch.tensor([[3], [0], [9]]),
    'one': torch.tensor([[0.37]]),
    'none': torch.zeros(0, 3),
}


def dense_read(t):
    """What a kernel reads at ``data_ptr()``: ``numel`` dense elements of the tensor's own dtype."""
    buf = IF.buffer_of(t)
    first = (t.data_ptr() - buf.data_ptr()) // t.element_size()
    return buf.reshape(-1)[first:first + t.numel()]


def is_poison(t):
    if t.numel() == 0:
        return True
    return bool((IF.as_bytes(t.contiguous()) == (0xFF if t.is_floating_point() else 0x7F)).all())


@pytest.mark.parametrize('name', list(SAMPLES))
@pytest.mark.parametrize('form', ['canonical', 'strided', 'sliced', 'wide'])
def test_a_form_keeps_the_values_and_is_what_it_says(form, name):
    h = SAMPLES[name]
    t = IF.BY_NAME[form](h, CPU)
    assert t.shape == h.shape and torch.equal(t.to(torch.float64), h.to(torch.float64))
    plain = h.numel() <= 1
    if form == 'canonical' or (form == 'strided' and plain) or (form == 'sliced' and h.numel() == 0):
        assert t.dtype == h.dtype and t.is_contiguous() and t.storage_offset() == 0 and IF.buffer_of(t) is t
    elif form == 'strided':
        assert t.dtype == h.dtype and not t.is_contiguous() and t.storage_offset() == 0
        assert t.stride() == tuple(2 * s for s in h.contiguous().stride()[:-1]) + (2,)
        buf = IF.buffer_of(t)
        assert buf.shape == h.shape[:-1] + (2 * h.shape[-1],) and is_poison(buf[..., 1::2]), 'the gaps are poison'
        assert not torch.equal(dense_read(t).to(torch.float64), h.reshape(-1).to(torch.float64)), 'a dense reader sees poison'
    elif form == 'sliced':
        buf = IF.buffer_of(t)
        assert t.dtype == h.dtype and t.is_contiguous() and t.storage_offset() == 1 and buf.shape == (h.numel() + 2,)
        assert t.data_ptr() - buf.data_ptr() == h.element_size()
        assert is_poison(buf[:1]) and is_poison(buf[-1:]), 'the first and the last element are poison'
    else:
        want = {torch.float32: torch.float64, torch.int8: torch.int64, torch.int16: torch.int64, torch.int32: torch.int64}
        if name in ('mask3', 'mask2'):
            assert t.dtype == torch.bool
        elif name == 'none':
            assert t.dtype == torch.float64, 'an empty tensor is no mask'
        else:
            assert t.dtype == want.get(h.dtype, h.dtype)
        assert t.is_contiguous() and t.storage_offset() == 0


def test_wide_leaves_the_widest_types_alone():
    assert IF.wide(SAMPLES['ligand'], CPU).dtype == torch.float64 and IF.wide(SAMPLES['t_int'], CPU).dtype == torch.int64
    assert IF.wide(torch.tensor([True, False]), CPU).dtype == torch.bool


def test_the_other_shapes():
    seen = [SAMPLES['one'], SAMPLES['positions'], SAMPLES['mask3'], SAMPLES['mask3'], torch.zeros(3 * 5 * 5, 1), SAMPLES['mask3']]
    got = [IF.squeezed(h, 'forward[33]', k, seen) for k, h in enumerate(seen)]
    assert [tuple(g.shape) for g in got] == [(1,), (3, 5, 3), (3, 5), (3, 5), (3, 5, 5), (3, 5, 1)]
    assert all(torch.equal(g.reshape(-1), h.reshape(-1)) for g, h in zip(got, seen))
    assert IF.squeezed(SAMPLES['mask3'], 'chain-one', 2, seen) is SAMPLES['mask3'], 'a case without a second documented shape'
    assert IF.other_mask_shape(SAMPLES['mask2']).shape == (3, 5, 1) and IF.other_column_shape(torch.zeros(4)).shape == (4, 1)
    loss = [SAMPLES['positions'], SAMPLES['t_int'].reshape(-1)]
    assert IF.squeezed(loss[1], 'loss-fc', 1, loss).shape == (3, 1) and IF.squeezed(loss[0], 'loss-fc', 0, loss) is loss[0]
    assert IF.squeezed(torch.zeros(15, dtype=torch.int64), 'train-pocket', 1, loss).shape == (15,), 'the batch-index vector'
    assert IF.squeezed(SAMPLES['one'], 'forward-pocket', -6 + 6, seen).shape == (1,), 'positions may count from the end'
    assert IF.squeezed(SAMPLES['mask2'], 'rings', 0, []).shape == (3, 5, 1) and IF.squeezed(SAMPLES['positions'], 'rings', 1, []) is \
        SAMPLES['positions']
    assert set(IF.SQUEEZE) <= set(GF.CASES)


def test_the_placer_keeps_a_copy_and_sees_a_write():
    seen = [SAMPLES['positions'], SAMPLES['counts']]
    for form in ('strided', 'sliced', 'wide'):
        placer = IF.FormPlace(CPU, seen, form, 'bonds', GS.host)
        placed = [placer.place(h) for h in seen]
        placer.assert_untouched()
        IF.buffer_of(placed[1]).reshape(-1)[-1] += 1                    # the last element: poison in two of the forms
        with pytest.raises(AssertionError, match='wrote to its input 1'):
            placer.assert_untouched()
    with pytest.raises(AssertionError, match='input 0 differs'):
        IF.FormPlace(CPU, seen, 'wide', 'bonds', GS.host).place(SAMPLES['positions'] + 1)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def test_the_exemptions_are_the_stated_ones():
    assert GF.NOT_APPLICABLE is IF.NOT_APPLICABLE and GF.REFUSES is IF.REFUSES
    assert IF.NOT_APPLICABLE == {'forward-c-abi'}
    assert set(IF.REFUSES) == {('rmsd', 'wide', 'maps'), ('tanimoto', 'wide', 'a_bits'), ('tanimoto', 'wide', 'b_bits')}
    from difflinker_amd import metrics
    for (case, form, parameter), (_, piece) in IF.REFUSES.items():
        wrapper = {'rmsd': metrics.best_rmsd, 'tanimoto': metrics.tanimoto_nearest}[case]
        assert parameter in inspect.signature(wrapper).parameters
        assert piece in inspect.getsource(wrapper), 'the message the wrapper raises'
    assert 'int16' in metrics.pack_maps.__doc__ and 'pack_maps' in metrics.best_rmsd.__doc__, 'the docstring fixes the dtype'
    assert 'int32 words' in metrics.tanimoto_nearest.__doc__


def test_every_case_runs_under_every_form():
    assert set(GF.CASES) == (set(GS.DRIVES) - IF.NOT_APPLICABLE) | set(GF.ADDED)
    assert set(GF.ADDED) == {'fingerprints', 'tanimoto', 'clashes-shared', 'parameter-grad', 'parameter-grad-pocket'}
    assert len(GF.CASES) == len(set(GF.CASES))
    assert set(GF.OVERRIDES) == {'aromatic', 'fragment-cuts', 'multi-cuts', 'pocket-select'} and set(GF.OVERRIDES) <= set(GS.DRIVES)
    assert IF.UNDER_TEST == ('strided', 'sliced', 'wide', 'squeezed')
    marks = {m.args[0]: m.args[1] for m in GF.test_entry_point_takes_the_form.pytestmark if m.name == 'parametrize'}
    assert list(marks['case']) == GF.CASES and tuple(marks['form']) == IF.UNDER_TEST
    assert set(GF.TAKES_BONDS) == {'molecule_keys', 'ring_scores', 'fingerprints', 'refine_bond_orders', 'fragment_cuts', 'multi_cuts'}
    assert set(GF.REFORMS) == {'bonds-capacity-slice', 'bonds-int64', 'counts-strided', 'counts-sliced', 'counts-int64'}
    assert set(IF.ADDED_CASES) == set(GF.ADDED) | {'stride-0[33]', 'stride-0[20,33,9]', 'found'}


def wrapper_of(path):
    module, *names = path.split('.')
    obj = importlib.import_module('difflinker_amd.' + module)
    for name in names:
        obj = getattr(obj, name)
    return obj


WRAPPERS = ('egnn.Dynamics.forward', 'egnn.Dynamics.parameter_grad', 'egnn.Dynamics.training_forward',
            'egnn.DynamicsWithPockets.forward', 'egnn.DynamicsWithPockets.parameter_grad', 'egnn.DynamicsWithPockets.training_forward',
            'edm.EDM.forward', 'edm.EDM.training_forward', 'edm.EDM.sample_chain', 'edm.InpaintingEDM.sample_chain',
            'edm.EDM._sampler_step', 'linker_size.SizeGNN.predict_logits', 'linker_size.SizeClassifier.training_forward',
            'molecule_builder.perceive_bonds', 'molecule_builder.refine_bond_orders', 'metrics.molecule_keys', 'metrics.best_rmsd',
            'metrics.analyze_clashes', 'metrics.analyze_shapes', 'metrics.ring_scores', 'metrics.fingerprints',
            'metrics.tanimoto_nearest', 'fragment.fragment_cuts', 'fragment.multi_cuts', 'pocket.select_pockets')


def test_the_coverage_table_names_the_public_wrappers():
    assert set(IF.COVERS) == set(WRAPPERS)


@pytest.mark.parametrize('path', WRAPPERS)
def test_every_parameter_is_covered_or_no_tensor(path):
    """The wrapper's signature is exactly its row of ``COVERS`` (a case feeds the parameter a formed tensor) plus its own entry of
    ``NOT_A_TENSOR``: a new parameter fails here until it is in one of them.  A row may only name a case that reaches the
    wrapper and places that parameter (``PLACES``, whose counts the GPU suite holds against what the case really placed)."""
    names = set(inspect.signature(wrapper_of(path)).parameters)
    table, plain = IF.COVERS[path], IF.NOT_A_TENSOR[path]
    assert not set(table) & plain
    assert set(table) | plain == names, f'{path}: {sorted(names ^ (set(table) | plain))}'
    for parameter, case in table.items():
        if case == 'found':
            assert parameter == 'found' and path in IF.TAKE_FOUND
            continue
        reached, placed = IF.PLACES[case]
        assert path in reached, f'{path}.{parameter}: the case {case} does not call it'
        assert placed.get(parameter, 0) >= 1, f'{path}.{parameter}: the case {case} places no such input'


def test_the_placing_table_is_the_suites():
    assert set(IF.PLACES) == set(GF.CASES) and set(IF.NOT_A_TENSOR) == set(IF.COVERS)
    for case, (reached, placed) in IF.PLACES.items():
        names = set().union(*(inspect.signature(wrapper_of(path)).parameters for path in reached))
        assert set(placed) <= names and all(n >= 1 for n in placed.values()), f'{case}: {sorted(set(placed) - names)}'
    assert all(p in inspect.signature(wrapper_of(path)).parameters for path in IF.TAKE_FOUND for p in ['found'])
    assert set(GF.TAKES_BONDS) >= {path.split('.')[-1] for path in IF.TAKE_FOUND}


def test_misaligned_fingerprint_rows_are_copied_once():
    """``tanimoto_nearest`` hands the kernel, which reads 16 bytes at a time, an aligned copy of a row slice."""
    from difflinker_amd.metrics import _aligned_rows
    rows = torch.arange(4 * 16 + 4, dtype=torch.int32)
    aligned = rows[(-rows.data_ptr() % 16) // 4:][:64].view(4, 16)
    assert aligned.data_ptr() % 16 == 0 and _aligned_rows(aligned) is aligned
    for shift in (1, 2, 3):
        part = rows[(-rows.data_ptr() % 16) // 4 + shift:][:48].view(3, 16)
        got = _aligned_rows(part)
        assert part.data_ptr() % 16 == 4 * shift and got.data_ptr() % 16 == 0 and torch.equal(got, part) and got is not part


# ---- the Bonds normaliser --------------------------------------------------------------------------------------------------------------
def a_bonds(B=3, capacity=4, N=5):
    from difflinker_amd.molecule_builder import Bonds
    g = torch.Generator().manual_seed(2)
    i32 = lambda *shape: torch.randint(0, 5, shape, generator=g, dtype=torch.int32)     # noqa: E731
    return Bonds(i32(B), i32(B, capacity, 3), i32(B, N), i32(B), i32(B, N), i32(B))


def test_members_on_the_host_are_refused():
    from difflinker_amd import _lib
    from difflinker_amd.molecule_builder import normalize_bonds
    with pytest.raises(_lib.HipLibraryError, match='ring_scores runs on the HIP device only.*n_bonds on cpu'):
        normalize_bonds(a_bonds(), 3, CPU, 'ring_scores')


def test_a_canonical_bonds_is_not_copied():
    from difflinker_amd.molecule_builder import _canonical_members
    found = a_bonds()
    got = _canonical_members(found, 3, CPU)
    for name in found._fields:
        assert getattr(got, name).data_ptr() == getattr(found, name).data_ptr(), name
    assert got.bonds.data_ptr() == found.bonds.data_ptr()
    hand = found._replace(valence=None, n_components=None, component=None)     # what the tests build by hand
    got = _canonical_members(hand, 3, CPU)
    assert got.valence is None and got.component is None and got.status.data_ptr() == hand.status.data_ptr()


@pytest.mark.parametrize('how', ['int64', 'strided', 'sliced', 'capacity-slice'])
def test_the_normaliser_makes_dense_int32(how):
    from difflinker_amd.molecule_builder import _KERNEL_READS, _canonical_members
    found = a_bonds()
    if how == 'capacity-slice':
        wider = IF.poison_(torch.empty((3, 8, 3), dtype=torch.int32))
        wider[:, :4] = found.bonds
        mine = found._replace(bonds=wider[:, :4])
    else:
        form = {'int64': IF.wide, 'strided': IF.strided, 'sliced': IF.sliced}[how]
        mine = found._replace(**{name: form(getattr(found, name), CPU) for name in found._fields})
    before = [IF.as_bytes(IF.buffer_of(t)).clone() for t in mine]
    got = _canonical_members(mine, 3, CPU)
    assert got.component is mine.component, 'no kernel reads it: left as it is'
    for name in _KERNEL_READS:
        t = getattr(got, name)
        assert t.dtype == torch.int32 and t.is_contiguous() and torch.equal(t, getattr(found, name)), name
        dense = t.reshape(-1)
        assert torch.equal(torch.as_strided(t, dense.shape, (1,)), getattr(found, name).reshape(-1)), 'what a kernel reads'
    assert all(torch.equal(IF.as_bytes(IF.buffer_of(t)), b) for t, b in zip(mine, before)), 'the caller\'s members are left alone'


def test_wrong_shapes_name_the_member():
    from difflinker_amd.molecule_builder import _canonical_members
    found = a_bonds()
    for name, bad in (('bonds', found.bonds[:, :, :2]), ('bonds', found.bonds[:2]), ('bonds', found.bonds.reshape(3, 12)),
                      ('n_bonds', found.n_bonds[:2]), ('status', torch.tensor(0, dtype=torch.int32)),
                      ('valence', found.valence[:2]), ('n_components', torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match=f'shapes disagree: {name} '):
            _canonical_members(found._replace(**{name: bad}), 3, CPU)
    odd = found._replace(component=found.component[:2])                  # not the kernels' business
    assert _canonical_members(odd, 3, CPU).component is odd.component
