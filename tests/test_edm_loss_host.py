"""CPU tests of the loss / VLB evaluation (EDM.forward): C ABI, the refusals, the evaluate command line, and the host-side
batch reductions against the reference's formulas (src/edm.py:64-121)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edm(T=10, inpainting=False):
    from difflinker_amd import Dynamics, EDM, InpaintingEDM
    dyn = Dynamics(n_dims=3, in_node_nf=9, context_node_nf=1, hidden_nf=128, n_layers=1, norm_constant=1e-6,
                   centering=inpainting)
    return (InpaintingEDM if inpainting else EDM)(dyn, in_node_nf=9, n_dims=3, timesteps=T, noise_schedule='polynomial_2',
                                                  noise_precision=1e-5, loss_type='l2', norm_values=[1, 4, 10])


def _inputs(B=2, N=5):
    nm = torch.ones(B, N, 1)
    fm = torch.zeros(B, N, 1)
    fm[:, :3] = 1
    return (torch.randn(B, N, 3), torch.nn.functional.one_hot(torch.randint(0, 9, (B, N)), 9).float(), nm, fm, nm - fm,
            torch.ones(B * N * N, 1, dtype=torch.int8), fm)


def test_loss_entry_points_exported_declared_and_checked():
    import __graft_entry__ as g
    g.build()
    from difflinker_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    for name in ('dl_edm_loss_prologue', 'dl_edm_loss_epilogue'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r'\b' + name + r'\s*\(', header)
        # argument checks come before any device work: a missing pointer is DL_ERR_BAD_ARG on any machine
        assert getattr(lib, name)(None, None) == -1
        assert getattr(lib, name)(ctypes.byref(_lib.DLLossArgs(B=1, N=4, nf=9, T=10, timesteps=10)), None) == -1
    assert lib.dl_abi_version() == _lib.ABI_VERSION == 7
    assert ctypes.sizeof(_lib.DLLossArgs) == 160                    # dl_loss_args (LP64)
    assert re.search(r'#define DL_LOSS_ROW (\d+)', header).group(1) == str(_lib.LOSS_ROW)


def test_forward_with_grad_refuses():
    edm = _edm()
    with pytest.raises(NotImplementedError, match='no_grad'):
        edm(*_inputs())


def test_forward_on_cpu_tensors_has_no_fallback():
    from difflinker_amd import _lib
    for inpainting in (False, True):
        with torch.no_grad(), pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
            _edm(inpainting=inpainting)(*_inputs())


def test_ddpm_forward_training_refuses():
    from difflinker_amd import DDPM
    from helpers import GLUE_HPARAMS
    m = DDPM(**GLUE_HPARAMS)
    with pytest.raises(NotImplementedError):
        m.forward({}, training=True)
    with pytest.raises(NotImplementedError):
        m.setup('test')


def test_evaluate_cli_help():
    proc = subprocess.run([sys.executable, '-m', 'difflinker_amd.evaluate', '--help'], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    for flag in ('--checkpoint', '--data', '--prefix', '--batch_size', '--noise_source', '--seed', '--device'):
        assert flag in proc.stdout


def _reference_reductions(rows, t_int, T, nf, norm0, inpainting):
    """The reference's batch reductions of the per-molecule terms, restated from edm.py:64-121 (fp32 tensors)."""
    error_t, noise, kl, log_px, log_ph, log_const, snr_w, n = rows.unbind(1)
    dim = (n - 1) * 3 if inpainting else n * 3
    delta_log_px = (-dim * np.log(norm0)).mean()
    t_is_zero = (t_int.reshape(-1, 1) == 0).squeeze().float()
    t_is_not_zero = 1 - t_is_zero
    l2_loss = (error_t / ((3 + nf) * n)).mean()
    loss_term_t = ((T * 0.5 * snr_w * error_t) * t_is_not_zero).sum() / t_is_not_zero.sum()
    noise_t = (noise * t_is_not_zero).sum() / t_is_not_zero.sum()
    if t_is_zero.sum() > 0:
        loss_term_0 = ((-(log_px + log_ph) + -log_const) * t_is_zero).sum() / t_is_zero.sum()
        noise_0 = (noise * t_is_zero).sum() / t_is_zero.sum()
    else:
        loss_term_0, noise_0 = 0., 0.
    return delta_log_px, kl.mean(), loss_term_t, loss_term_0, l2_loss, noise_t, noise_0


@pytest.mark.parametrize('inpainting', [False, True])
@pytest.mark.parametrize('t_int', [[0, 3, 10, 0, 7], [0, 0, 0, 0, 0], [1, 2, 3, 4, 5], [0]])
def test_host_batch_reductions_match_the_reference(t_int, inpainting):
    from difflinker_amd import _lib
    g = torch.Generator().manual_seed(len(t_int) + 7 * inpainting)
    B = len(t_int)
    rows = torch.randn((B, _lib.LOSS_ROW), generator=g)
    rows[:, 7] = torch.randint(2, 30, (B,), generator=g).float()
    edm = _edm(inpainting=inpainting)
    edm.norm_values = [1.7, 4, 10]
    t = torch.tensor(t_int, dtype=torch.int32)
    got = edm._reduce_loss_rows(rows, t)
    want = _reference_reductions(rows, t, edm.T, 9, 1.7, inpainting)
    for a, b in zip(got, want):
        if isinstance(b, float):
            assert isinstance(a, float) and a == b
        elif torch.isnan(b):
            assert torch.isnan(a)
        else:
            assert torch.allclose(a, b, rtol=1e-6, atol=0), (a, b)


def test_aggregate_metric_is_the_mean_over_steps():
    from difflinker_amd import DDPM
    outs = [{'loss': torch.tensor(1.0)}, {'loss': 2.0}, {'loss': torch.tensor(6.0)}]
    assert float(DDPM.aggregate_metric(outs, 'loss')) == 3.0
