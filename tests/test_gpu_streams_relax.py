"""Part A of ``tests/test_gpu_streams.py`` for ``molecule_builder.relax`` (``dl_relax_molecules``, whose stream is the last field
of its structure): the inputs hold poison until copies queued on a side stream behind a delay have written them, the outputs are
read on that stream, and they equal the default stream's bits and the reference's.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import pytest
import torch

import relax_ref as rr
import test_gpu_relax as TR
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_relax_on_a_side_stream(delay):  # noqa: F811
    batch = rr.batch_of(TR.hand_molecules(), 12, seed=1, status=[2 * (b % 2) for b in range(len(TR.hand_molecules()))])
    tensor = lambda a, dtype=torch.float32: torch.as_tensor(a).to(dtype)      # noqa: E731

    def call(place):
        return dict(zip(rr.FIELDS, TR.public(batch, lambda a, dtype=torch.float32: place(tensor(a, dtype)), steps=20)))

    call(lambda t: t.to(TR.DEV))                                             # the tables are on the device before the harness starts
    torch.cuda.synchronize()
    base = GS.check_stream_contract(lambda: call, delay)
    want = rr.reference(batch, steps=20)
    for name in rr.FIELDS:
        assert base[name].numpy().tobytes() == want[name].tobytes(), name
    assert want['steps_done'].max() == 20 and (want['status'] == 2).any()
