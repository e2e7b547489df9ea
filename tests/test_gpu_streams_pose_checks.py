"""Part A of ``tests/test_gpu_streams.py`` for ``metrics.pose_checks`` (``dl_pose_checks``, whose stream is the last field of
its structure): the inputs hold poison until copies queued on a side stream behind a delay have written them, the outputs are
read on that stream, and they equal the default stream's bits and the reference's.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import numpy as np
import pytest
import torch

import pose_checks_ref as pr
import test_gpu_pose_checks as TP
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_pose_checks_on_a_side_stream(delay):  # noqa: F811
    from difflinker_amd.metrics import pose_checks
    from difflinker_amd.molecule_builder import Bonds
    molecules = [dict(pr.hand_molecule(name), marked=[0]) for name in TP.NAMES]
    batch = TP.batch_of(molecules, 12, status=[2 * (b % 2) for b in range(len(molecules))])
    tensor = lambda name, dtype: torch.as_tensor(batch[name]).to(dtype)      # noqa: E731

    def call(place):
        found = Bonds(place(tensor('n_bonds_in', torch.int32)), place(tensor('bonds', torch.int32)), None, None, None,
                      place(tensor('status_in', torch.int32)))
        counts, flags, status = pose_checks(
            place(tensor('one_hot', torch.float32)), place(tensor('x', torch.float32)), place(tensor('node_mask', torch.float32)),
            found, False, drop_mask=place(tensor('drop_mask', torch.float32)), mark_mask=place(tensor('mark_mask', torch.float32)),
            atom_planar=place(tensor('atom_planar', torch.int32)))
        return {'counts': counts, 'atom_flags': flags, 'status': status}

    call(lambda t: t.to(TP.DEV))                                             # the tables are on the device before the harness starts
    torch.cuda.synchronize()
    base = GS.check_stream_contract(lambda: call, delay)
    want = TP.reference(batch)
    for name in pr.FIELDS:
        assert np.array_equal(base[name].numpy(), want[name]), name
    assert want['counts'][:, 0, [pr.SHORT, pr.LONG, pr.BAD_ANGLES, pr.CLASHES]].sum() > 10 and want['counts'][:, 1].any()
