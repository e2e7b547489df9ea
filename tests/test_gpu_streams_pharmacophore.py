"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.pharmacophore_features`` and ``metrics.feature_match``: the inputs hold
poison until copies queued on a side stream behind a delay have written them, the outputs are read on that stream, and they
equal the default stream's bits and the reference's.

In a file of its own that is collected AFTER ``test_gpu_streams.py``: torch hands out its side streams round-robin from a pool
and the HIP runtime spreads them over a few hardware queues, so which queue a test's side stream gets depends on how many
streams the tests before it took.  The control of that module (``test_the_delay_outlasts_a_launch_on_the_wrong_stream``) needs a
side stream that does not share the default stream's queue; two more streams taken before it moved it onto that queue, and it
failed.  Taken after it, they move nothing it depends on."""
import pytest
import torch

import pharmacophore_ref as pr
import test_gpu_pharmacophore as TP
import test_gpu_streams as GS
from test_gpu_pharmacophore import fuzz  # noqa: F401  (the module's fixture: the fuzz batch and its reference)
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_features_on_a_side_stream(monkeypatch, delay, fuzz):  # noqa: F811
    from difflinker_amd import metrics
    batch = fuzz['batch']

    def call():
        return metrics.pharmacophore_features(
            TP.dev(batch['one_hot']), TP.dev(batch['x']), TP.dev(batch['node_mask']), TP.bonds_of(batch),
            TP.dev(batch['bond_aromatic'], torch.int32), True, TP.dev(fuzz['drop']), TP.dev(fuzz['mark']), capacity=fuzz['Fcap'])
    make = GS._through_dev(TP, call)
    base = GS.check_stream_contract(lambda: make(monkeypatch), delay)
    TP.assert_exact({k: v.numpy() for k, v in base.items()}, fuzz['a'], pr.FIELDS, 'the baseline')


def test_the_match_on_a_side_stream(monkeypatch, delay, fuzz):  # noqa: F811
    from difflinker_amd import metrics

    def call():
        kind = lambda name: torch.float32 if name == 'position' else torch.int32      # noqa: E731
        a, b = (metrics.Features(**{name: TP.dev(side[name], kind(name)) for name in pr.FIELDS}) for side in (fuzz['a'], fuzz['b']))
        return metrics.feature_match(a, b)
    make = GS._through_dev(TP, call)
    base = GS.check_stream_contract(lambda: make(monkeypatch), delay)
    TP.assert_exact({k: v.numpy() for k, v in base.items()}, TP.reference_match(fuzz['a'], fuzz['b']), pr.MATCH_FIELDS, 'the baseline')
