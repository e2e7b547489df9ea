"""Size-predictor training without a GPU: the new C entries are exported and argument-checked, the ABI version is
unchanged, CPU tensors raise, the balanced loss weights follow N / (C n_c), the CLI parses and refuses the other tasks."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dl_size_train_num_params', 'dl_size_train_workspace_bytes', 'dl_size_train_forward', 'dl_size_train_backward')


def test_new_exports_declared_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and f'{name}(' in header
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7


def _args(**kw):
    from difflinker_amd import _lib
    a = dict(B=2, N=10, in_node_nf=8, hidden_nf=128, out_node_nf=10, n_layers=2, batch_norm=1)
    a.update(kw)
    return _lib.DLSizeTrainArgs(**a)


@pytest.mark.parametrize('bn', [0, 1])
def test_num_params_matches_module(bn):
    from difflinker_amd import _lib
    from difflinker_amd.linker_size import SizeGNN
    lib = _lib.load()
    for L in (1, 3):
        gnn = SizeGNN(8, 128, 10, L, 'batch_norm' if bn else None)
        a = _args(n_layers=L, batch_norm=bn)
        assert lib.dl_size_train_num_params(ctypes.byref(a)) == sum(p.numel() for p in gnn.parameters())
        assert lib.dl_size_train_workspace_bytes(ctypes.byref(a)) > 0


def test_entries_refuse_bad_arguments():
    from difflinker_amd import _lib
    lib = _lib.load()
    assert lib.dl_size_train_forward(None, None) == -1
    assert lib.dl_size_train_backward(None, None) == -1
    assert lib.dl_size_train_num_params(None) == -1
    assert lib.dl_size_train_workspace_bytes(None) == 0
    a = _args()
    assert lib.dl_size_train_forward(ctypes.byref(a), None) == -1          # wrong n_params (0)
    a.n_params = lib.dl_size_train_num_params(ctypes.byref(a))
    assert lib.dl_size_train_forward(ctypes.byref(a), None) == -1          # null pointers, no workspace
    assert lib.dl_size_train_backward(ctypes.byref(a), None) == -1
    a.n_params += 1
    assert lib.dl_size_train_backward(ctypes.byref(a), None) == -1
    for kw in (dict(hidden_nf=256), dict(n_layers=0), dict(batch_norm=2), dict(in_node_nf=17), dict(out_node_nf=65)):
        b = _args(**kw)
        assert lib.dl_size_train_num_params(ctypes.byref(b)) == -1
        assert lib.dl_size_train_workspace_bytes(ctypes.byref(b)) == 0
        assert lib.dl_size_train_forward(ctypes.byref(b), None) == -2
    one = _args(B=1, N=1)                                                   # BatchNorm over one row: refused
    one.n_params = lib.dl_size_train_num_params(ctypes.byref(one))
    assert lib.dl_size_train_forward(ctypes.byref(one), None) == -1
    # a workspace one byte short is refused before anything reads it
    a = _args()
    a.n_params = lib.dl_size_train_num_params(ctypes.byref(a))
    a.workspace, a.workspace_bytes = 16, lib.dl_size_train_workspace_bytes(ctypes.byref(a)) - 1
    a.params = 16
    assert lib.dl_size_train_forward(ctypes.byref(a), None) == -1


def test_training_on_cpu_tensors_raises():
    from difflinker_amd import _lib
    from difflinker_amd.linker_size import SizeClassifier
    clf = SizeClassifier(in_node_nf=8, hidden_nf=128, out_node_nf=10, n_layers=2, normalization='batch_norm')
    data = {'one_hot': torch.zeros(2, 4, 8), 'positions': torch.zeros(2, 4, 3), 'fragment_mask': torch.ones(2, 4, 1),
            'linker_mask': torch.zeros(2, 4, 1), 'edge_mask': torch.zeros(32, 1)}
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        clf.training_forward(data)


def test_train_mode_forward_still_refuses_and_points_to_training_forward():
    from difflinker_amd.linker_size import SizeClassifier
    clf = SizeClassifier(in_node_nf=8, hidden_nf=128, out_node_nf=10, n_layers=1, normalization='batch_norm').train()
    with pytest.raises(NotImplementedError, match='training_forward'):
        clf.gnn._host_tensors()


def test_configure_optimizers_reference_settings():
    from difflinker_amd.linker_size import SizeClassifier
    clf = SizeClassifier(in_node_nf=8, hidden_nf=128, out_node_nf=10, n_layers=2, lr=2e-3)
    opt = clf.configure_optimizers()
    grp = opt.param_groups[0]
    assert type(opt) is torch.optim.AdamW and grp['lr'] == 2e-3 and grp['amsgrad'] is True
    assert grp['weight_decay'] == 1e-12
    assert [id(p) for p in grp['params']] == [id(p) for p in clf.gnn.parameters()]


def test_balanced_loss_weights_reproduce_the_zinc_table():
    """The ZINC training set's class counts (sizes 3..12): the reference's table is N / (C n_c) of them."""
    from difflinker_amd.linker_size import balanced_loss_weights
    counts = [126274, 94716, 85604, 77990, 33663, 13527, 5399, 1269, 161, 7]
    assert sum(counts) == 438610
    w = balanced_loss_weights(counts)
    assert w[0] == pytest.approx(3.47347831e-01, rel=1e-8)
    assert w[-1] == pytest.approx(43861 / 7, rel=1e-12) and w[-1] == pytest.approx(6265.85714, rel=1e-8)
    assert all(wc * len(counts) * c == pytest.approx(438610) for wc, c in zip(w, counts))
    assert balanced_loss_weights([3, 0, 1]) == [4 / 9, 0.0, 4 / 3]


def test_cli_other_tasks_raise(tmp_path):
    from difflinker_amd import train_size_gnn
    for task in ('regression', 'ordinal'):
        with pytest.raises(NotImplementedError):
            train_size_gnn.main(['--task', task, '--data', str(tmp_path), '--checkpoints', str(tmp_path / 'ck')])


def test_cli_help():
    proc = subprocess.run([sys.executable, '-m', 'difflinker_amd.train_size_gnn', '--help'], cwd=ROOT, capture_output=True,
                          text=True, timeout=120)
    assert proc.returncode == 0
    for opt in ('--max_steps', '--loss_weights', '--normalization', '--resume', '--val_every'):
        assert opt in proc.stdout
