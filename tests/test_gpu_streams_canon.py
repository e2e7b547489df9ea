"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.canonical_ranks`` (``dl_canonical_ranks``, whose stream is the last field
of its structure): the inputs hold poison until copies queued on a side stream behind a delay have written them, the outputs are
read on that stream, and they equal the default stream's bits and the reference's.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import pytest
import torch

import test_gpu_canon as TC
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_canonical_ranks_on_a_side_stream(delay):  # noqa: F811
    molecules, batch = TC.small_batch()

    def call(place):
        return TC.launch(batch, place=place)

    base = GS.check_stream_contract(lambda: call, delay)
    want = TC.reference(molecules, 16)
    for name in TC.FIELDS:
        assert base[name].tolist() == want[name], name
    assert int(base['n_leaves'][0]) == 48 and bool((base['status'] == 2).any())
    assert torch.equal(base['rank'][0].sort().values[8:], torch.arange(8, dtype=torch.int32))
