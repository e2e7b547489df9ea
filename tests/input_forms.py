"""The forms a caller's tensor may take, for tests/test_gpu_input_forms.py, and the tables of that suite (held against the code
on the CPU by tests/test_input_forms_host.py).  Nothing here touches a GPU at import.

Every wrapper turns tensors into raw pointers (``t.data_ptr()``) and from then on the kernel reads dense fp32 / int32 / int8 rows
at that address.  A FORM is a function ``form(host_tensor, device) -> device_tensor`` that hands the same VALUES over in another
layout or dtype.  Every form preserves every value exactly, and whatever a reader that assumes the dense canonical layout would
touch instead of the values is poison: 0xFF bytes (NaN) in floats, 0x7F bytes in integers (``test_gpu_streams.poison_``).

  canonical   dense, zero offset, the dtype the case asked for
  strided     the same shape and dtype as a view ``buffer[..., ::2]`` of a buffer whose last dimension is doubled (1-D: ``[::2]``);
              the gaps hold poison.  Tensors of at most one element stay as they are
  sliced      the contiguous view ``buffer[1:1 + numel].view(shape)`` of a flat buffer of ``numel + 2`` elements whose first and
              last are poison: the storage offset is one element, ``data_ptr()`` is aligned to the item size and nothing more
              - a row slice ``batch[1:]``.  Empty tensors stay as they are
  wide        float32 -> float64; int8 / int16 / int32 -> int64; a float tensor whose values are all 0 or 1 (masks, one-hot
              rows) -> bool.  A tensor that is float64, int64 or bool already stays
  squeezed    where the wrapper's docstring allows two shapes, the other one (``SQUEEZE``); everything else canonical

``buffer_of(t)`` is the whole allocation behind a form's tensor, poison included: the suite keeps a bit copy of it and holds the
buffer against the copy after the call - no wrapper writes to its inputs or around them."""
import torch

FORMS = ('canonical', 'strided', 'sliced', 'wide', 'squeezed')
UNDER_TEST = FORMS[1:]

# ---- what a case may do instead of matching the canonical run's bits -------------------------------------------------------------
# this case hands raw pointers to the C entry point with ctypes; the C ABI takes dense arrays by definition
NOT_APPLICABLE = {'forward-c-abi'}
# (case, form, parameter) -> (the positions of the parameter among the case's placed inputs, a piece of the message): the
# wrapper's docstring fixes the dtype and the right outcome is a ValueError that names it, before any launch.  The case then
# runs once more with these parameters canonical and everything else in the form
REFUSES = {
    ('rmsd', 'wide', 'maps'): ((3,), '16-bit'),                          # best_rmsd: the table of pack_maps is int16
    ('tanimoto', 'wide', 'a_bits'): ((0,), 'int32 words'),               # tanimoto_nearest: Fingerprints.bits are int32 words
    ('tanimoto', 'wide', 'b_bits'): ((1,), 'int32 words'),
}


def poison_(t):
    if t.numel():
        t.view(torch.uint8).fill_(0xFF if t.is_floating_point() else 0x7F)
    return t


def buffer_of(t):
    """The allocation a form's tensor is a view of (the tensor itself when it is no view)."""
    return t if t._base is None else t._base


def canonical(h, device):
    return h.contiguous().to(device)


def strided(h, device):
    if h.numel() <= 1:
        return canonical(h, device)
    wide_shape = tuple(h.shape[:-1]) + (2 * h.shape[-1],)
    buf = poison_(torch.empty(wide_shape, dtype=h.dtype))
    buf[..., ::2] = h
    return buf.to(device)[..., ::2]


def sliced(h, device):
    if h.numel() == 0:
        return canonical(h, device)
    buf = poison_(torch.empty(h.numel() + 2, dtype=h.dtype))
    buf[1:1 + h.numel()] = h.reshape(-1)
    return buf.to(device)[1:1 + h.numel()].view(h.shape)


def wide_dtype(h):
    if h.dtype == torch.float32:
        return torch.bool if h.numel() and bool(((h == 0) | (h == 1)).all()) else torch.float64
    if h.dtype in (torch.int8, torch.int16, torch.int32, torch.uint8):
        return torch.int64
    return h.dtype


def wide(h, device):
    return h.to(wide_dtype(h)).contiguous().to(device)


# ---- the other shape of a parameter whose docstring allows two ---------------------------------------------------------------------
def _is_mask(h):
    return h.is_floating_point() and h.numel() > 0 and bool(((h == 0) | (h == 1)).all())


def other_mask_shape(h):
    """``[B,N]`` for ``[B,N,1]`` and back."""
    if h.dim() == 3 and h.shape[2] == 1:
        return h.reshape(h.shape[:2])
    assert h.dim() == 2, tuple(h.shape)
    return h.reshape(h.shape + (1,))


def other_column_shape(h):
    """``[B]`` for ``[B,1]`` and back (``t``, ``t_int``)."""
    if h.dim() == 2 and h.shape[1] == 1:
        return h.reshape(-1)
    assert h.dim() == 1, tuple(h.shape)
    return h.reshape(-1, 1)


def squeezed_at(h, op, seen):
    """The placed input ``h`` under ``op`` of ``SQUEEZE``; ``seen`` are all placed inputs of the case (for the batch's shape)."""
    if op == 'mask':
        return other_mask_shape(h)
    if op == 'column':
        return other_column_shape(h)
    if op[0] == 'edge':                                                  # [B*N*N,1] -> [B,N,N], B and N from the mask at op[1]
        B, N = seen[op[1]].shape[:2]
        assert h.numel() == B * N * N, (tuple(h.shape), B, N)
        return h.reshape(B, N, N)
    raise KeyError(op)


_FORWARD = {0: 'column', 2: 'mask', 3: 'mask', 4: ('edge', 2), 6: 'column', 8: 'mask', 9: 'mask', 10: ('edge', 2)}
# case -> {position among the placed inputs (negative: from the end): op}, or 'masks': every placed float tensor ``[B,N]`` /
# ``[B,N,1]`` of zeros and ones, or 't_int': every placed int64 tensor with one element per molecule (B from the first placed
# tensor of three dimensions).  A case that is not here has no parameter with two documented shapes: it runs canonical
SQUEEZE = {
    # Dynamics.forward / _launch_forward: t, xh, node_mask, linker_mask, edge_mask, context - twice
    'forward[33]': _FORWARD, 'forward[55,32,31,2,40]': _FORWARD, 'forward-team-of-4[20,33,9]': _FORWARD,
    'forward-teams[58,61]': _FORWARD, 'forward-hbm[116,10]': _FORWARD,
    # DynamicsWithPockets: t, xh into launch, then the four masks into forward (edge_mask is the batch-index vector: one shape)
    'forward-pocket': {0: 'column', 2: 'mask', 3: 'mask'},
    # EDM.forward / training_forward: t_int [B] or [B,1], the one placed int64 tensor with an element per molecule
    'loss-fc': 't_int', 'loss-pocket': 't_int', 'train-fc': 't_int', 'train-pocket': 't_int',
    'bonds': {2: 'mask'},                                                # perceive_bonds(one_hot, x, node_mask)
    'molecule-keys': {2: 'mask', 3: 'mask'},                             # analyze(one_hot, x, node_mask, drop_mask=)
    'clashes': 'masks', 'shapes': 'masks', 'rings': 'masks', 'aromatic': 'masks', 'fragment-cuts': 'masks', 'multi-cuts': 'masks',
    'fingerprints': 'masks', 'clashes-shared': 'masks',
}


def squeezed(h, case, k, seen):
    """The ``k``-th placed input of ``case`` in its other documented shape, on the host (``h`` itself where it has none)."""
    table = SQUEEZE.get(case)
    if table is None:
        return h
    if table == 'masks':
        two = h.dim() == 2 or (h.dim() == 3 and h.shape[2] == 1)
        return other_mask_shape(h) if two and _is_mask(h) else h
    if table == 't_int':
        B = next(v.shape[0] for v in seen if v.dim() == 3)
        return other_column_shape(h) if h.dtype == torch.int64 and h.numel() == B and h.dim() <= 2 else h
    op = table.get(k, table.get(k - len(seen)))
    return h if op is None else squeezed_at(h, op, seen)


BY_NAME = {'canonical': canonical, 'strided': strided, 'sliced': sliced, 'wide': wide}


class FormPlace:
    """``place`` of the run under test: builds the canonical host tensor exactly as ``test_gpu_streams.Recorder.place`` does
    (``host``), holds it against the baseline run's, and hands out its form.  ``keep`` holds, per placed input, the whole buffer
    behind it and a bit copy of that buffer; ``assert_untouched`` compares them after the call."""

    def __init__(self, device, seen, form, case, host, canonical_at=()):
        self.device, self.seen, self.form, self.case, self.host = device, seen, form, case, host
        self.canonical_at, self.k, self.keep, self.placed = set(canonical_at), 0, [], []

    def place(self, v, dtype=None):
        if v is None:
            return None
        h, k = self.host(v, dtype), self.k
        want = self.seen[k]
        assert h.dtype == want.dtype and h.shape == want.shape and torch.equal(as_bytes(h), as_bytes(want)), f'input {k} differs'
        self.k += 1
        if k in self.canonical_at or k - len(self.seen) in self.canonical_at:
            t = canonical(h, self.device)
        elif self.form == 'squeezed':
            t = canonical(squeezed(h, self.case, k, self.seen), self.device)
        else:
            t = BY_NAME[self.form](h, self.device)
        a, b = t.cpu().reshape(-1).to(torch.float64), h.reshape(-1).to(torch.float64)
        assert a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all()), f'input {k}: the form changes a value'
        self.placed.append(t)
        self.keep.append((buffer_of(t), as_bytes(buffer_of(t)).clone()))
        return t

    def assert_untouched(self):
        """After ``torch.cuda.synchronize()``: every placed buffer, the poison around the values included, is what it was."""
        for k, (buf, copy) in enumerate(self.keep):
            assert torch.equal(as_bytes(buf), copy), f'{self.case} under {self.form}: the call wrote to its input {k} or around it'


def as_bytes(t):
    """A dense tensor's bytes (NaN equals NaN)."""
    t = t.detach()
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


# ---- the coverage table of tests/test_input_forms_host.py ----------------------------------------------------------------------------
# public wrapper -> {tensor parameter: the case of tests/test_gpu_input_forms.py that feeds it a formed tensor}
_DENOISER = dict(t='forward[33]', xh='forward[33]', node_mask='forward[33]', linker_mask='forward[33]', edge_mask='forward[33]',
                 context='forward[33]')
_POCKET_DENOISER = {k: 'forward-pocket' for k in _DENOISER}
_LOSS = dict(x='loss-fc', h='loss-fc', node_mask='loss-fc', fragment_mask='loss-fc', linker_mask='loss-fc', edge_mask='loss-fc',
             context='loss-fc', t_int='loss-fc', noise='loss-fc')
_CHAIN = dict(x='chain-one', h='chain-one', node_mask='chain-one', fragment_mask='chain-one', linker_mask='chain-one',
              edge_mask='chain-one', context='chain-one', noise_bank='chain-one')
_FOUND = 'found'                                                         # the re-formed ``Bonds`` cases
COVERS = {
    'egnn.Dynamics.forward': _DENOISER,
    'egnn.Dynamics.parameter_grad': dict({k: 'parameter-grad' for k in _DENOISER}, grad_out='parameter-grad'),
    'egnn.Dynamics.training_forward': {k: 'parameter-grad' for k in _DENOISER},
    'egnn.DynamicsWithPockets.forward': _POCKET_DENOISER,
    'egnn.DynamicsWithPockets.parameter_grad': dict({k: 'parameter-grad-pocket' for k in _DENOISER},
                                                    grad_out='parameter-grad-pocket'),
    'egnn.DynamicsWithPockets.training_forward': {k: 'parameter-grad-pocket' for k in _DENOISER},
    'edm.EDM.forward': _LOSS,
    'edm.EDM.training_forward': {k: 'train-fc' for k in _LOSS},
    'edm.EDM.sample_chain': _CHAIN,
    'edm.InpaintingEDM.sample_chain': {k: 'chain-inpainting' for k in _CHAIN},
    'edm.EDM._sampler_step': dict(z_t='sampler-step', eps_hat='sampler-step', noise='sampler-step', fragment_mask='sampler-step',
                                  linker_mask='sampler-step'),
    'linker_size.SizeGNN.predict_logits': dict(one_hot='size-predict', positions='size-predict', fragment_mask='size-predict',
                                               edge_mask='size-predict'),
    'linker_size.SizeClassifier.training_forward': dict(data='size-train'),
    'molecule_builder.perceive_bonds': dict(one_hot='bonds', x='bonds', node_mask='bonds'),
    'molecule_builder.refine_bond_orders': dict(found=_FOUND, one_hot='aromatic', x='aromatic', node_mask='aromatic',
                                                drop_mask='aromatic', mark_mask='aromatic'),
    'metrics.molecule_keys': dict(one_hot='molecule-keys', node_mask='molecule-keys', found=_FOUND, drop_mask='molecule-keys'),
    'metrics.best_rmsd': dict(xa='rmsd', xb='rmsd', n_atoms='rmsd', maps='rmsd', offsets='rmsd'),
    'metrics.analyze_clashes': dict(one_hot='clashes', x='clashes', query_mask='clashes', target_mask='clashes',
                                    protein='clashes-shared', thresholds='clashes-shared'),
    'metrics.analyze_shapes': dict(one_hot_a='shapes', x_a='shapes', mask_a='shapes', one_hot_b='shapes', x_b='shapes',
                                   mask_b='shapes'),
    'metrics.ring_scores': dict(node_mask='rings', found=_FOUND, drop_mask='rings', mark_mask='rings'),
    'metrics.fingerprints': dict(one_hot='fingerprints', node_mask='fingerprints', found=_FOUND, drop_mask='fingerprints',
                                 centre_mask='fingerprints'),
    'metrics.tanimoto_nearest': dict(a_bits='tanimoto', b_bits='tanimoto', a_offsets='tanimoto', b_offsets='tanimoto'),
    'fragment.fragment_cuts': dict(one_hot='fragment-cuts', node_mask='fragment-cuts', bonds='fragment-cuts',
                                   n_bonds='fragment-cuts', charge='fragment-cuts', status='fragment-cuts'),
    'fragment.multi_cuts': dict(one_hot='multi-cuts', node_mask='multi-cuts', bonds='multi-cuts', n_bonds='multi-cuts',
                                charge='multi-cuts', status='multi-cuts'),
    'pocket.select_pockets': dict(protein_x='pocket-select', protein_group='pocket-select', protein_offset='pocket-select',
                                  pair_protein='pocket-select', ligand_x='pocket-select', ligand_mask='pocket-select'),
}
# per wrapper, its parameters that are no tensors (flags, rule constants, capacities, a coefficient struct): with the row of
# ``COVERS`` they are the wrapper's whole signature
NOT_A_TENSOR = {
    'egnn.Dynamics.forward': {'self'}, 'egnn.Dynamics.parameter_grad': {'self'}, 'egnn.Dynamics.training_forward': {'self'},
    'egnn.DynamicsWithPockets.forward': {'self'}, 'egnn.DynamicsWithPockets.parameter_grad': {'self'},
    'egnn.DynamicsWithPockets.training_forward': {'self'},
    'edm.EDM.forward': {'self', 'mol_offset'}, 'edm.EDM.training_forward': {'self', 'mol_offset'},
    'edm.EDM.sample_chain': {'self', 'keep_frames', 'mol_offset'},
    'edm.InpaintingEDM.sample_chain': {'self', 'keep_frames', 'mol_offset'},
    'edm.EDM._sampler_step': {'self', 'coef'},
    'linker_size.SizeGNN.predict_logits': {'self'}, 'linker_size.SizeClassifier.training_forward': {'self'},
    'molecule_builder.perceive_bonds': {'is_geom', 'margins', 'capacity'},
    'molecule_builder.refine_bond_orders': {'is_geom', 'planarity', 'substituent'},
    'metrics.molecule_keys': {'is_geom'}, 'metrics.best_rmsd': set(),
    'metrics.analyze_clashes': {'is_geom', 'scale', 'tolerance', 'contact_cutoff'},
    'metrics.analyze_shapes': {'is_geom', 'scale', 'step'},
    'metrics.ring_scores': set(), 'metrics.fingerprints': {'radius', 'n_bits'},
    'metrics.tanimoto_nearest': {'exclude_diagonal', 'want_sum'},
    'fragment.fragment_cuts': {'is_geom', 'capacity', 'min_linker', 'min_fragment', 'min_path_atoms', 'linker_leq_frags'},
    'fragment.multi_cuts': {'is_geom', 'capacity', 'min_cuts', 'max_cuts', 'min_linker', 'min_fragment', 'max_atoms', 'min_rings'},
    'pocket.select_pockets': {'cutoff', 'capacity', 'max_atoms'},
}

# case -> (the wrappers its inputs reach, {parameter: how many tensors the case puts on the device through ``place`` for it}).
# The GPU suite holds the sum against the number of inputs the case really placed, and the host guard holds every row of
# ``COVERS`` against this table: a row may only name a case that reaches the wrapper and places that parameter.
_SIX = dict(t=1, xh=1, node_mask=1, linker_mask=1, edge_mask=1, context=1)
_TWICE = {k: 2 for k in _SIX}                                            # once into _launch_forward, once into forward
_SEVEN = dict(x=1, h=1, node_mask=1, fragment_mask=1, linker_mask=1, edge_mask=1, context=1)
_CUTS = dict(one_hot=1, node_mask=1, bonds=1, n_bonds=1, charge=1, status=1)
_FC, _PK = 'egnn.Dynamics.', 'egnn.DynamicsWithPockets.'
PLACES = {
    'forward[33]': ((_FC + 'forward',), _TWICE), 'forward[55,32,31,2,40]': ((_FC + 'forward',), _TWICE),
    'forward-team-of-4[20,33,9]': ((_FC + 'forward',), _TWICE), 'forward-teams[58,61]': ((_FC + 'forward',), _TWICE),
    'forward-hbm[116,10]': ((_FC + 'forward',), _TWICE),
    'forward-pocket': ((_PK + 'forward',), _SIX),
    'chain-one': (('edm.EDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-join': (('edm.EDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-two-launch': (('edm.EDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-overflow-teams': (('edm.EDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-host-loop-pocket': (('edm.EDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-inpainting': (('edm.InpaintingEDM.sample_chain',), dict(_SEVEN, noise_bank=2)),
    'chain-philox': (('edm.EDM.sample_chain',), _SEVEN),
    'philox-bank': (('edm.EDM._philox_draw',), dict(mol_index=1)),
    'sampler-step': (('edm.EDM._sampler_step',), dict(z_t=1, eps_hat=1, noise=1, fragment_mask=1, linker_mask=1)),
    'loss-fc': (('edm.EDM.forward',), dict(_SEVEN, t_int=1, noise=2)),
    'loss-pocket': (('edm.EDM.forward',), dict(_SEVEN, t_int=1, noise=2)),
    'train-fc': (('edm.EDM.training_forward',), dict(_SEVEN, t_int=1, noise=2)),
    'train-pocket': (('edm.EDM.training_forward',), dict(_SEVEN, t_int=1, noise=2)),
    'size-predict': (('linker_size.SizeGNN.predict_logits',), dict(one_hot=1, positions=1, fragment_mask=1, edge_mask=1)),
    'size-train': (('linker_size.SizeClassifier.training_forward',), dict(data=7)),
    'bonds': (('molecule_builder.perceive_bonds',), dict(one_hot=1, x=1, node_mask=1)),
    'aromatic': (('molecule_builder.refine_bond_orders',), dict(found=3, one_hot=1, x=1, node_mask=1, drop_mask=1, mark_mask=1)),
    'molecule-keys': (('metrics.analyze', 'metrics.molecule_keys'), dict(one_hot=1, x=1, node_mask=1, drop_mask=1)),
    'rmsd': (('metrics.best_rmsd',), dict(xa=1, xb=1, n_atoms=1, maps=1, offsets=1)),
    'clashes': (('metrics.analyze_clashes',), dict(one_hot=1, x=1, query_mask=1, target_mask=1)),
    'clashes-shared': (('metrics.analyze_clashes',), dict(one_hot=1, x=1, query_mask=1, target_mask=1, protein=2, thresholds=1)),
    'shapes': (('metrics.analyze_shapes',), dict(one_hot_a=1, x_a=1, mask_a=1, one_hot_b=1, x_b=1, mask_b=1)),
    'rings': (('metrics.ring_scores',), dict(node_mask=1, found=3, drop_mask=1, mark_mask=1)),
    'fragment-cuts': (('fragment.fragment_cuts',), _CUTS), 'multi-cuts': (('fragment.multi_cuts',), _CUTS),
    'pocket-select': (('pocket.select_pockets',), dict(protein_x=1, protein_group=1, protein_offset=1, pair_protein=1, ligand_x=1,
                                                       ligand_mask=1)),
    'fingerprints': (('metrics.fingerprints',), dict(one_hot=1, node_mask=1, found=3, drop_mask=1, centre_mask=1)),
    'tanimoto': (('metrics.tanimoto_nearest',), dict(a_bits=1, b_bits=1, a_offsets=1, b_offsets=1)),
    'parameter-grad': ((_FC + 'training_forward', _FC + 'parameter_grad'), dict(_SIX, grad_out=1)),
    'parameter-grad-pocket': ((_PK + 'training_forward', _PK + 'parameter_grad'), dict(_SIX, grad_out=1)),
}
# the re-formed ``Bonds`` (test_a_bonds_of_the_callers_own): the wrappers that take one
TAKE_FOUND = ('metrics.molecule_keys', 'metrics.ring_scores', 'metrics.fingerprints', 'molecule_builder.refine_bond_orders')
# the cases the GPU suite adds to the stream table's
ADDED_CASES = ('fingerprints', 'tanimoto', 'clashes-shared', 'parameter-grad', 'parameter-grad-pocket', 'stride-0[33]',
               'stride-0[20,33,9]', _FOUND)
