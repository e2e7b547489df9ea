"""Host-side contract of pocket training: the scope check, the C ABI's new names and the argument checks of
``dl_egnn_backward_pocket``, all of which answer before any device work (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

from difflinker_amd import DynamicsWithPockets, _lib, egnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2             # dl_status of include/difflinker_hip.h
NEW = ('dl_egnn_backward_pocket_workspace_bytes', 'dl_egnn_backward_pocket')


def pocket_dyn(graph_type='FC-10A-4A', **kw):
    args = dict(n_dims=3, in_node_nf=9, context_node_nf=2, hidden_nf=128, n_layers=1, inv_sublayers=2, norm_constant=1e-6,
                normalization_factor=100, graph_type=graph_type)
    args.update(kw)
    return DynamicsWithPockets(**args)


@pytest.mark.parametrize('graph_type', ['FC-4A', 'FC-10A-4A'])
def test_check_trainable_accepts_the_fc_pocket_graphs(graph_type):
    egnn.check_trainable(pocket_dyn(graph_type))


@pytest.mark.parametrize('kw', [dict(graph_type='4A'), dict(attention=True), dict(tanh=True), dict(aggregation_method='mean'),
                                dict(sin_embedding=True), dict(hidden_nf=64)], ids=lambda kw: next(iter(kw)))
def test_check_trainable_refuses_the_rest(kw):
    with pytest.raises(NotImplementedError):
        egnn.check_trainable(pocket_dyn(**kw))


def test_cpu_tensors_raise():
    dyn = pocket_dyn()
    B, N = 1, 6
    z, nm = torch.zeros(B, N, 12), torch.ones(B, N, 1)
    ctx = torch.cat([nm, torch.zeros(B, N, 1)], -1)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        dyn.parameter_grad(torch.zeros(B, 1), z, nm, torch.zeros(B, N, 1), torch.zeros(B * N), ctx, torch.zeros(B, N, 12))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        dyn.training_forward(torch.zeros(B, 1), z, nm, torch.zeros(B, N, 1), torch.zeros(B * N), ctx)


def test_exports_and_header():
    assert _lib.ABI_VERSION == 7 and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    at = _lib.EXPORTS.index('dl_egnn_backward_fc')
    assert _lib.EXPORTS[at + 1:at + 3] == NEW
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
    lib = _lib.load()
    assert lib.dl_abi_version() == 7
    for name in NEW:
        assert hasattr(lib, name)


def args_for(B=2, N=40, **kw):
    a = egnn.backward_args(pocket_dyn(), B, N)
    for k, v in kw.items():
        setattr(a, k, v)
    a.n_params = int(_lib.load().dl_egnn_backward_fc_num_params(ctypes.byref(a)))
    return a


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    call = lambda a, g=2: int(lib.dl_egnn_backward_pocket(ctypes.byref(a), g, None))      # noqa: E731
    assert int(lib.dl_egnn_backward_pocket(None, 2, None)) == BAD_ARG
    a = args_for()
    assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(a), 2)) > 0
    assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(a), 0)) > 0       # '4A': the C entry point takes it
    assert call(a) == BAD_ARG                                                 # null pointers
    assert call(a, 3) == BAD_ARG and call(a, -1) == BAD_ARG       # no such graph
    assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(a), 3)) == 0
    a.n_params += 1
    assert call(a) == BAD_ARG
    for kw in (dict(hidden_nf=64), dict(inv_sublayers=5), dict(context_node_nf=1), dict(n_layers=0)):
        b = egnn.backward_args(pocket_dyn(), 2, 40)
        for k, v in kw.items():
            setattr(b, k, v)
        assert call(b) == UNSUPPORTED, kw
        assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(b), 2)) == 0
    assert call(args_for(N=0)) == BAD_ARG and call(args_for(B=-1)) == BAD_ARG
    wide = args_for(B=1, N=egnn.POCKET_BACKWARD_MAX_ATOMS + 1)
    assert call(wide) == _lib.DL_ERR_TOO_MANY_ATOMS
    assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(wide), 2)) == 0
    assert call(args_for(B=1, N=1024)) == BAD_ARG                             # 1024 padded atoms: in range (null pointers)
    assert int(lib.dl_egnn_backward_pocket_workspace_bytes(ctypes.byref(args_for(B=1, N=1024)), 2)) > 0


def test_empty_batch_is_ok():
    lib = _lib.load()
    a = args_for(B=0)
    assert int(lib.dl_egnn_backward_pocket(ctypes.byref(a), 2, None)) == _lib.DL_OK
