"""A completeness guard for tests/test_gpu_streams.py that runs without a GPU: every ``dl_*`` function of the API header whose
last parameter is ``void* stream`` is driven by at least one case of part A (``DRIVES``), and every case has a builder.  A new
entry point then cannot land without a stream case.  This parses the header only."""
import os
import re

import test_gpu_streams as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    found = []
    for name, params in re.findall(r'\b(dl_\w+)\s*\(([^;{}()]*)\)\s*;', text):
        last = params.split(',')[-1].split()
        if last[-1:] == ['stream'] and ''.join(last[:-1]) == 'void*':
            found.append(name)
    return found


def test_the_header_is_parsed():
    found = stream_entry_points()
    assert len(found) == len(set(found)) >= 27
    for name in ('dl_egnn_forward_fc', 'dl_sample_chain_fc_join', 'dl_egnn_backward_pocket', 'dl_size_train_backward',
                 'dl_philox_fill', 'dl_pocket_select', 'dl_aromatic_rings'):
        assert name in found, name
    assert 'dl_workspace_bytes' not in found and 'dl_model_create' not in found


def test_every_entry_point_with_a_stream_has_a_stream_case():
    driven = {name for names in GS.DRIVES.values() for name in names}
    missing = [name for name in stream_entry_points() if name not in driven]
    assert not missing, f'no case of tests/test_gpu_streams.py drives {missing}'
    unknown = sorted(driven - set(stream_entry_points()))
    assert not unknown, f'DRIVES names {unknown}, which the header does not declare with a stream'


def test_every_case_of_the_table_has_a_builder():
    assert set(GS.DRIVES) == set(GS.BUILDERS)
    assert all(names and isinstance(names, tuple) for names in GS.DRIVES.values())
