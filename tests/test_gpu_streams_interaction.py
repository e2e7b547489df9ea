"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.analyze_interactions`` (both launches of ``csrc/interaction.hip``):
the inputs hold poison until copies queued on a side stream behind a delay have written them, the outputs are read on that
stream, and they equal the default stream's bits and the reference's.  Then two calls on two streams at once.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: the control of that module needs a side stream that does not share the default stream's queue, and streams taken
before it move it."""
import numpy as np
import pytest
import torch

import test_gpu_interaction as TI
import test_gpu_streams as GS
from test_gpu_interaction import mixed  # noqa: F401  (the module's fixture: the mixed batch and its reference)
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def shared_list(M=300):
    rng = np.random.default_rng(6)
    px = (18.0 + rng.uniform(0, 11.0, size=(M, 3))).astype(np.float32)
    pxs = (rng.choice(TI.NF, size=M) | (rng.integers(0, 8, size=M) << 4)).astype(np.int32)
    return px, pxs


def test_both_launches_on_a_side_stream(monkeypatch, delay, mixed):  # noqa: F811
    m, protein = mixed, shared_list()
    make = GS._through_dev(TI, lambda: TI.analyze(m['x'], m['one_hot'], m['qm'], m['lig'], m['tm'], protein=protein))
    base = GS.check_stream_contract(lambda: make(monkeypatch), delay)
    want = TI.reference(m['x'], m['one_hot'], m['qm'], m['lig'], m['tm'], protein=protein)
    assert torch.equal(base['xs_type'], torch.from_numpy(want['xs_type'].copy()))
    TI.assert_scores(base, want, 'the baseline')
    assert int(base['n_pairs'].min()) > 500


def test_two_streams_at_once(mixed):  # noqa: F811
    m = mixed
    rng = np.random.default_rng(8)
    other = TI.stack([TI.big(rng, 700, 300, 200) for _ in range(3)])
    base, other_base = TI.analyze(m['x'], m['one_hot'], m['qm'], m['lig'], m['tm']), TI.analyze(*other)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = TI.analyze(*other)
    with torch.cuda.stream(s2):
        b = TI.analyze(m['x'], m['one_hot'], m['qm'], m['lig'], m['tm'])
    s1.synchronize()
    s2.synchronize()
    TI.assert_same_bits(a, other_base, 'stream 1 of two')
    TI.assert_same_bits(b, base, 'stream 2 of two')
    assert int(a.n_pairs.min()) > 1000
