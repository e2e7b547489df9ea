"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.stereo`` (``dl_stereo_perceive``, whose stream is the last field of its
structure): the inputs hold poison until copies queued on a side stream behind a delay have written them, the outputs are read
on that stream, and they equal the default stream's bits and the restatement's.  Then two launches on two streams at once.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import ctypes

import pytest
import torch

import stereo_ref as sr
import test_gpu_stereo as TS
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_stereo_on_a_side_stream(delay):  # noqa: F811
    batch = TS.batch_of(sr.random_molecules(TS.SEEDS[0], 16), 40, seed=19)

    def call(place):
        return TS.through_python(batch, place=place, host=False)

    base = GS.check_stream_contract(lambda: call, delay)
    want = TS.reference(batch)
    for name in sr.FIELDS:
        assert base[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    assert int(want['counts'][:, 0].sum()) > 0


def test_two_streams_at_once():
    from difflinker_amd import _lib
    molecules = sr.random_molecules(TS.SEEDS[1], 32)
    first, second = TS.batch_of(molecules[:16], 40, seed=19), TS.batch_of(molecules[16:], 40, seed=20)
    want = [TS.reference(first), TS.reference(second)]
    streams = [torch.cuda.Stream(device=TS.DEV), torch.cuda.Stream(device=TS.DEV)]
    prepared = [TS.arguments(first), TS.arguments(second)]
    torch.cuda.synchronize()
    for (args, out, held), stream in zip(prepared, streams):
        args.stream = stream.cuda_stream
        _lib.check(_lib.load().dl_stereo_perceive(ctypes.byref(args)), 'dl_stereo_perceive')
    torch.cuda.synchronize()
    for (args, out, held), expected in zip(prepared, want):
        assert all(out[name].cpu().numpy().tobytes() == expected[name].tobytes() for name in sr.FIELDS)
