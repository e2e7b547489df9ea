"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.match_patterns`` (``dl_substructure_match``, whose stream is the last
field of its structure): the inputs hold poison until copies queued on a side stream behind a delay have written them, the
outputs are read on that stream, and they equal the default stream's bits and the reference's.  Then two calls on two streams
at once.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import pytest
import torch

import substructure_cases as sc
import test_gpu_streams as GS
import test_gpu_substructure as TS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_match_patterns_on_a_side_stream(delay):  # noqa: F811
    molecules, patterns, batch = TS.small_batch()

    def call(place):
        return TS.launch(batch, patterns, place=place)

    base = GS.check_stream_contract(lambda: call, delay)
    want = TS.reference(molecules, 16, patterns)
    for name in TS.FIELDS:
        assert base[name].tolist() == want[name], name
    assert int(base['n_hits'].sum()) > 8 and int(base['n_hits_marked'].sum()) > 0 and bool((base['status'] == 2).any())


def test_two_streams_at_once():
    molecules, patterns, batch = TS.small_batch()
    random_molecules, smarts = sc.random_batch()
    other_patterns = TS.compiled(smarts)
    other = TS.batch_of([TS.molecule(*m) for m in random_molecules], 24)
    base, other_base = TS.launch(batch, patterns), TS.launch(other, other_patterns)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = TS.launch(other, other_patterns)
    with torch.cuda.stream(s2):
        b = TS.launch(batch, patterns)
    s1.synchronize()
    s2.synchronize()
    for name in TS.FIELDS:
        assert torch.equal(a[name], other_base[name]) and torch.equal(b[name], base[name]), name
    assert int(a['n_hits'].sum()) > 500
