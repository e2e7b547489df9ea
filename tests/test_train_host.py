"""Training entry points without a GPU: the new C entries are exported and argument-checked, the ABI version is unchanged,
the optimiser has the reference's settings, out-of-scope denoisers raise, CPU tensors raise, the CLI parses."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dl_edm_loss_grad', 'dl_egnn_backward_fc_num_params', 'dl_egnn_backward_fc_workspace_bytes',
       'dl_egnn_backward_max_atoms', 'dl_egnn_backward_fc')


def test_new_exports_declared_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and f'{name}(' in header
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7


def test_new_entries_check_arguments():
    from difflinker_amd import _lib
    lib = _lib.load()
    assert lib.dl_egnn_backward_fc(None, None) == -1
    assert lib.dl_edm_loss_grad(None, None, None, None) == -1
    assert lib.dl_egnn_backward_fc_workspace_bytes(None) == 0
    assert lib.dl_egnn_backward_fc_num_params(None) == -1
    assert lib.dl_egnn_backward_max_atoms() >= 110
    a = _lib.DLBackwardArgs(B=2, N=10, in_node_nf=8, context_node_nf=1, condition_time=1, hidden_nf=128, n_layers=2,
                            inv_sublayers=2, normalization_factor=100.0)
    from difflinker_amd import Dynamics
    dyn = Dynamics(n_dims=3, in_node_nf=8, context_node_nf=1, hidden_nf=128, n_layers=2, inv_sublayers=2)
    assert lib.dl_egnn_backward_fc_num_params(ctypes.byref(a)) == sum(p.numel() for p in dyn.parameters())
    assert lib.dl_egnn_backward_fc_workspace_bytes(ctypes.byref(a)) > 0
    a.n_params = 5                                            # wrong layout, null pointers: refused before any device work
    assert lib.dl_egnn_backward_fc(ctypes.byref(a), None) == -1
    a.n_params = lib.dl_egnn_backward_fc_num_params(ctypes.byref(a))
    assert lib.dl_egnn_backward_fc(ctypes.byref(a), None) == -1
    a.hidden_nf = 64
    assert lib.dl_egnn_backward_fc(ctypes.byref(a), None) == -2
    a.hidden_nf, a.N = 128, lib.dl_egnn_backward_max_atoms() + 1
    assert lib.dl_egnn_backward_fc_workspace_bytes(ctypes.byref(a)) == 0


def _ddpm(**kw):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import GLUE_HPARAMS
    from difflinker_amd import DDPM
    hp = dict(GLUE_HPARAMS)
    hp.update(kw)
    return DDPM(**hp)


def test_configure_optimizers_reference_settings():
    m = _ddpm(lr=3e-4)
    opt = m.configure_optimizers()
    assert type(opt) is torch.optim.AdamW
    grp = opt.param_groups[0]
    assert grp['lr'] == 3e-4 and grp['amsgrad'] is True and grp['weight_decay'] == 1e-12
    assert [id(p) for p in grp['params']] == [id(p) for p in m.edm.parameters()]


@pytest.mark.parametrize('kw', [dict(attention=True), dict(tanh=True), dict(aggregation_method='mean'),
                                dict(sin_embedding=True), dict(hidden_nf=64),
                                dict(train_data_prefix='MOAD_train.full', context_node_nf=2, graph_type='4A')])
def test_out_of_scope_training_raises(kw):
    from difflinker_amd.egnn import check_trainable
    m = _ddpm(**kw)
    with pytest.raises(NotImplementedError):
        check_trainable(m.edm.dynamics)
    x = torch.zeros(1, 4, 3)
    with pytest.raises(NotImplementedError):
        m.edm.training_forward(x, torch.zeros(1, 4, 8), torch.ones(1, 4, 1), torch.ones(1, 4, 1), torch.zeros(1, 4, 1),
                               torch.zeros(16, 1, dtype=torch.int8), torch.zeros(1, 4, 1))


def test_training_on_cpu_tensors_raises():
    from difflinker_amd import _lib
    m = _ddpm()
    b = 1
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        m.edm.training_forward(torch.zeros(b, 4, 3), torch.zeros(b, 4, 8), torch.ones(b, 4, 1), torch.ones(b, 4, 1),
                               torch.zeros(b, 4, 1), torch.zeros(16, 1, dtype=torch.int8), torch.zeros(b, 4, 1))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        m.edm.dynamics.training_forward(torch.zeros(b, 1), torch.zeros(b, 4, 11), torch.ones(b, 4, 1), torch.ones(b, 4, 1),
                                        torch.zeros(16, 1, dtype=torch.int8), torch.zeros(b, 4, 1))


def test_existing_forward_still_refuses_grad_mode():
    m = _ddpm()
    with pytest.raises(NotImplementedError, match='training=True'):
        m.forward({}, training=True)


def test_random_rotation_is_a_rotation():
    from difflinker_amd import utils
    torch.manual_seed(0)
    x = torch.randn(4, 6, 3)
    y = utils.random_rotation(x)
    assert torch.allclose(x.norm(dim=2), y.norm(dim=2), atol=1e-5)
    assert not torch.allclose(x, y)


def test_train_cli_help():
    proc = subprocess.run([sys.executable, '-m', 'difflinker_amd.train', '--help'], cwd=ROOT, capture_output=True,
                          text=True, timeout=120)
    assert proc.returncode == 0 and '--max_steps' in proc.stdout
