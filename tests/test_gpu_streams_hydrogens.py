"""Part A of ``tests/test_gpu_streams.py`` for ``molecule_builder.add_hydrogens`` (``dl_add_hydrogens``, whose stream is the
last field of its structure): the inputs hold poison until copies queued on a side stream behind a delay have written them,
the outputs are read on that stream, and they equal the default stream's bits and the reference's.

In a file of its own that is collected AFTER ``test_gpu_streams.py``, for the reason ``test_gpu_streams_pharmacophore.py``
gives: a side stream taken before that module's control moves the control's own stream onto the default stream's hardware
queue.  Taken after it, it moves nothing the control depends on."""
import numpy as np
import pytest
import torch

import hydrogens_ref as hr
import test_gpu_hydrogens as TH
import test_gpu_streams as GS
from test_gpu_streams import delay  # noqa: F401  (the module's fixture: the calibrated delay of the stream harness)

pytestmark = pytest.mark.gpu


def test_hydrogens_on_a_side_stream(delay):  # noqa: F811
    from difflinker_amd.molecule_builder import Bonds, add_hydrogens
    molecules = [hr.hand_molecule(name) for name in TH.NAMES]
    batch = TH.pack(molecules, 12, rng=np.random.default_rng(0))
    tensor = lambda name, dtype: torch.as_tensor(batch[name]).to(dtype)      # noqa: E731

    def make():
        def run(place):
            found = Bonds(place(tensor('n_in', torch.int32)), place(tensor('bonds', torch.int32)), None, None, None,
                          place(tensor('status', torch.int32)))
            got = add_hydrogens(found, place(tensor('one_hot', torch.float32)), place(tensor('x', torch.float32)),
                                place(tensor('mask', torch.float32)), False, drop_mask=place(tensor('drop', torch.float32)),
                                atom_planar=place(tensor('planar', torch.int32)))
            return {name: getattr(got, name) for name in got._fields}
        return run
    add_hydrogens(Bonds(*(None if v is None else v.to(TH.DEV) for v in (tensor('n_in', torch.int32), tensor('bonds', torch.int32),
                                                                       None, None, None, tensor('status', torch.int32)))),
                  tensor('one_hot', torch.float32).to(TH.DEV), tensor('x', torch.float32).to(TH.DEV),
                  tensor('mask', torch.float32).to(TH.DEV), False)      # the tables are on the device before the harness starts
    torch.cuda.synchronize()
    base = GS.check_stream_contract(make, delay)
    want = TH.reference(batch)
    listed = np.arange(48)[None, :] < want['n_h'][:, None]
    assert np.array_equal(base['n_h'].numpy(), want['n_h']) and np.array_equal(base['h_count'].numpy(), want['h_count'])
    assert np.array_equal(base['status'].numpy(), want['status']) and want['n_h'].sum() > 40
    assert np.array_equal(base['parent'].numpy()[listed], want['h_parent'][listed])
    assert np.abs(base['x'].numpy()[listed] - want['h_x'][listed]).max() <= TH.BAR
