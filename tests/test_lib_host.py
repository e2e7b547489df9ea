"""CPU tests of ``difflinker_amd._lib``'s one launch path: the table of the struct-taking entry points, the prototypes
``_open`` declares from it, and the refusal of host tensors."""
import ctypes

import pytest
import torch

# every entry point whose prototype is ``int32 f(const STRUCT*)``: the stream is the struct's last field
STREAM_IN_STRUCT = ['dl_interaction_types', 'dl_interaction_scores', 'dl_fingerprints', 'dl_tanimoto_nearest',
                    'dl_pharmacophore_features', 'dl_feature_match', 'dl_add_hydrogens', 'dl_pose_checks']
# every entry point whose prototype is ``int32 f(const STRUCT*, void* stream)``: the analysis ones, then loss, backward, size-train
STREAM_AS_ARGUMENT = ['dl_perceive_bonds', 'dl_molecule_keys', 'dl_best_rmsd', 'dl_clash_scores', 'dl_shape_scores',
                      'dl_ring_scores', 'dl_fragment_cuts', 'dl_fragment_multicuts', 'dl_aromatic_rings', 'dl_pocket_select',
                      'dl_edm_loss_prologue', 'dl_edm_loss_epilogue', 'dl_egnn_backward_fc', 'dl_size_train_forward',
                      'dl_size_train_backward']


def test_the_table_declares_every_struct_taking_entry_point():
    import __graft_entry__ as g
    g.build()
    from difflinker_amd import _lib
    lib = _lib.load()
    assert set(_lib.STRUCT_ENTRY_POINTS) == set(STREAM_IN_STRUCT) | set(STREAM_AS_ARGUMENT)
    assert len(STREAM_IN_STRUCT) == 8 and len(STREAM_AS_ARGUMENT) == 15 and not set(STREAM_IN_STRUCT) & set(STREAM_AS_ARGUMENT)
    assert set(_lib.STRUCT_ENTRY_POINTS) <= set(_lib.EXPORTS)
    for name, struct in _lib.STRUCT_ENTRY_POINTS.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32, name
        fields = [field for field, _ in struct._fields_]
        if 'stream' in fields:
            assert name in STREAM_IN_STRUCT and fields[-1] == 'stream' and fields.count('stream') == 1, name
            assert dict(struct._fields_)['stream'] is ctypes.c_void_p, name
            assert fn.argtypes == [ctypes.POINTER(struct)], name
        else:
            assert name in STREAM_AS_ARGUMENT, name
            assert fn.argtypes == [ctypes.POINTER(struct), ctypes.c_void_p], name


def test_host_tensors_are_refused_by_name():
    from difflinker_amd import _lib
    x, mask = torch.zeros(2, 3), torch.ones(2)
    with pytest.raises(_lib.HipLibraryError, match=r'^some_wrapper runs on the HIP device only \(no CPU fallback\): got ') as e:
        _lib.require_device('some_wrapper', x=x, drop_mask=None, node_mask=mask)
    assert 'x on cpu' in str(e.value) and 'node_mask on cpu' in str(e.value) and 'drop_mask' not in str(e.value)
    _lib.require_device('some_wrapper', drop_mask=None)          # nothing given: nothing to refuse


def test_the_cast_makes_dense_tensors_and_passes_none():
    from difflinker_amd import _lib
    assert _lib.dense(None, torch.device('cpu'), torch.float32) is None
    wide = torch.arange(12, dtype=torch.int64).reshape(3, 4)[:, ::2]
    got = _lib.dense(wide, torch.device('cpu'), torch.int32)
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, wide.to(torch.int32))
    same = torch.zeros(4, dtype=torch.float32)
    assert _lib.dense(same, same.device, torch.float32) is same, 'a dense tensor is not copied'
    assert _lib.ptr(None) is None and _lib.ptr(same).value == same.data_ptr()
