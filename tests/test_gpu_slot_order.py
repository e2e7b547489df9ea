"""Pair loops with the short last chunks gathered into the last waves (difflinker_amd/csrc/slot_order.h; the map itself is walked
for every size on the CPU, tests/test_slot_order_host.py).

A receiver's n senders are cut into g chunks of q; where the last chunk holds r < q of them, the slots of the last chunks come
behind all the others and the waves they fill run r steps.  Sizes whose plans changed, and controls whose plans did not:

  n         q, g, r      |  n         q, g, r
  37/38/39  7, 6, 2/3/4  |  36        6, 6, 6      (control)
  43        9, 5, 7      |  42        7, 6, 7      (control)
  46        10, 5, 6     |  45        9, 5, 9      (control)
  48/49     10, 5, 8/9   |  50        10, 5, 10    (control)
  coordinate pass, 12 linker receivers of 46 senders: 3, 16, 1; 10 of 47: 2, 24, 1
  teams of two: 46 atoms, 23 receivers: 5, 10, 1; 47 atoms, 24 / 23 receivers: 5, 10, 2
  team of four: 50 atoms, 13 receivers: 3, 17, 2

* every forward against the oracle at the suite's forward bars (``P.FWD_TOLS``; f16x2: the bars of tests/test_gpu_f16x2.py),
  bitwise repeatable, padded rows exactly zero;
* in the test-hooks build ``dl_debug_slot_order(1)`` numbers the slots receiver by receiver again: the same forwards, a
  T = 6 chain and a T = 24 chain through the join launch (the shortest chains EDM hands over have T = 20) must come out bit for bit the same in both orders - every (receiver, chunk) partial adds
  the same senders in the same order and the partials are added in the same order, only the lane that computes one differs."""
import pytest
import torch

import test_gpu_join as J
import test_gpu_parity as P
from oracle import edm_oracle, egnn_oracle
from test_gpu_f16x2 import H_TOL as F16X2_H_TOL, V_TOL as F16X2_V_TOL

pytestmark = pytest.mark.gpu

NF, L = 9, 2
PLAIN, ATTENTION = None, dict(attention=True)
# (sizes, linkers, team, precision, flags)
CASES = [
    ((37, 38, 39), (5, 7, 9), 1, 'f16x3', PLAIN),
    ((43, 46, 48, 49), (6, 12, 8, 9), 1, 'f16x3', PLAIN),
    ((36, 42, 45, 50), (6, 7, 8, 8), 1, 'f16x3', PLAIN),               # controls: r = q, today's plan
    ((46, 47), (12, 10), 1, 'f16x3', PLAIN),                            # coordinate plans with r = 1
    ((46, 47), (12, 10), 2, 'f16x3', PLAIN),
    ((50, 46, 47), (8, 12, 10), 4, 'f16x3', PLAIN),
    ((46, 47), (12, 10), 2, 'fp32', PLAIN),
    ((37, 38, 39), (5, 7, 9), 1, 'f16x2', PLAIN),
    ((43, 46, 48, 49), (6, 12, 8, 9), 1, 'f16x3', ATTENTION),
]
IDS = [f'{"-".join(map(str, c[0]))}-team{c[2]}-{c[3]}{"-attention" if c[4] else ""}' for c in CASES]

_shared = {}


def _model(precision, flags):
    """A two-block denoiser with seeded weights (one seed per hyper-parameter set), built in whichever library is loaded."""
    dyn, sd, cfg = J._model(precision, 1201 + (7 if flags else 0), L, flags, nf=NF)
    return dyn, sd, cfg


def _inputs_and_reference(sizes, linkers, flags):
    """Inputs and the oracle's forward of a case: computed once, shared by the tests (and by the precisions) and never written to."""
    key = (sizes, linkers, bool(flags))
    if key not in _shared:
        _, sd, cfg = _model('f16x3', flags)
        inp, z, t = P.ragged_inputs(list(sizes), list(linkers), NF, seed=1210 + sum(sizes))
        ref = egnn_oracle.dynamics_forward(sd, cfg, t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'])
        _shared[key] = (inp, z, t, ref)
    return _shared[key]


@pytest.mark.parametrize('sizes,linkers,team,precision,flags', CASES, ids=IDS)
def test_forward_with_short_chunks_last_against_the_oracle(sizes, linkers, team, precision, flags):
    inp, z, t, ref = _inputs_and_reference(sizes, linkers, flags)
    dyn, _, _ = _model(precision, flags)
    dyn.team = team
    out = P.run_hip_forward(dyn, inp, z, t)
    ev, eh = P.report(f'slot order sizes={sizes} linkers={linkers} team={team} {precision} attention={bool(flags)}', out, ref, z)
    if precision == 'f16x2':
        assert ev <= F16X2_V_TOL and eh <= F16X2_H_TOL
    else:
        assert ev <= P.FWD_TOLS[precision] and eh <= P.FWD_TOLS[precision]
    assert float((out * (1 - inp['node_mask'].float())).abs().max()) == 0.0, 'padded rows must be exactly zero'
    assert float(ref[..., :3].abs().max()) > 1e-4, 'the coordinate head must act in this case'
    assert torch.equal(out, P.run_hip_forward(dyn, inp, z, t)), 'bitwise repeatable'


def _set_order(lib, receiver_major):
    assert lib.dl_debug_slot_order(1 if receiver_major else 0) == 0


def test_both_slot_orders_give_the_same_bits():
    """The test-hooks library: the forwards above, a T = 6 chain of test_gpu_join's 12 molecules and their T = 24 chain through the
    join launch, once in the product's order and once receiver by receiver."""
    from difflinker_amd import _lib
    assert not hasattr(_lib.load(), 'dl_debug_slot_order'), 'the product library must not export the test hook'
    with _lib.test_hooks() as lib:
        try:
            for (sizes, linkers, team, precision, flags), tag in zip(CASES, IDS):
                inp, z, t, _ = _inputs_and_reference(sizes, linkers, flags)
                dyn, _, _ = _model(precision, flags)
                dyn.team = team
                _set_order(lib, False)
                new = P.run_hip_forward(dyn, inp, z, t)
                _set_order(lib, True)
                old = P.run_hip_forward(dyn, inp, z, t)
                assert torch.isfinite(new).all() and torch.equal(new, old), tag

            # chains of test_gpu_join's 12 molecules.  EDM hands a chain over inside one launch from T = 20 on, so the six-step
            # chain runs as one launch (one compute unit per molecule throughout) and the 24-step chain of test_gpu_join takes
            # the join launch (its four big molecules finish on teams of two); _run asserts the route
            dyn, sd, cfg = P.make_dynamics(J.NF, 1, 1, seed=1251)
            dyn.team = 1
            inp, _, _ = P.ragged_inputs(J.SIZES, J.LINKERS, J.NF, seed=1252)
            B, N = inp['x'].shape[:2]
            g = {k: v.to(P.dev()) for k, v in inp.items()}
            for T, route in ((6, 'one'), (J.T, 'join')):
                edm = J._edm(dyn, J.NF, T)
                bank = edm_oracle.NoiseBank.generate(T, B, N, 3, J.NF, seed=1253)
                _set_order(lib, False)
                new = J._run(edm, g, True, bank.stacked(), keep=3, route=route)
                _set_order(lib, True)
                old = J._run(edm, g, True, bank.stacked(), keep=3, route=route)
                assert torch.isfinite(new).all() and torch.equal(new, old), f'chain T = {T}, route {route}'
        finally:
            lib.dl_debug_slot_order(0)
