"""``metrics.stereo``, ``metrics.stereo_codes`` and the isomeric strings on the GPU under every transform of ``frame_cases``:
unchanged under proper signed permutations, rotations, shifts and renumberings (classes and labels go with the atoms),
hands exchanged under mirrors.  The cases and their clearance are those of ``stereo_frame_cases``."""
import numpy as np
import pytest
import torch

import stereo_frame_cases as sf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def gpu_run(batch):
    from difflinker_amd import metrics
    from difflinker_amd.molecule_builder import Bonds
    t = lambda a, dtype=torch.float32: torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype)      # noqa: E731
    one_hot, mask, drop = t(batch['one_hot']), t(batch['node_mask']), t(batch['drop_mask'])
    found = Bonds(t(batch['n_bonds_in'], torch.int32), t(batch['bonds'], torch.int32), None, None, None, t(batch['status_in'], torch.int32))
    result = metrics.stereo(one_hot, t(batch['x']), mask, found, True, drop, t(batch['mark_mask']), t(batch['atom_planar'], torch.int32),
                            t(batch['bond_aromatic'], torch.int32))
    codes = metrics.stereo_codes(result, one_hot, mask, found, drop)
    strings = metrics.isomeric_smiles_to_host(result, codes, one_hot, mask, found, drop)
    host = {name: v.cpu().numpy() for name, v in {**result, **codes}.items()}
    out = []
    for b in range(len(strings)):
        n, n_in = len(batch['rows'][b]), int(batch['n_bonds_in'][b])
        out.append(dict(atom_class=host['atom_class'][b][:n].tolist(), atom_stereo=host['atom_stereo'][b][:n].tolist(),
                        bond_stereo=host['bond_stereo'][b][:n_in].tolist(), counts=host['counts'][b].tolist(),
                        stereo_code=int(host['stereo_code'][b]) & 0xFFFFFFFFFFFFFFFF,
                        mirror_code=int(host['mirror_code'][b]) & 0xFFFFFFFFFFFFFFFF, isomeric_smiles=strings[b],
                        stereo_rank=host['stereo_rank'][b][:n].tolist()))
    return out


@pytest.fixture(scope='module')
def base():
    batch, _ = sf.batch_under('identity')
    got = gpu_run(batch)
    assert got == sf.host_run(batch), 'the GPU path and the restatement agree on the cases themselves'
    return got


@pytest.mark.parametrize('name', sf.TRANSFORMS[1:])
def test_the_gpu_under(name, base):
    batch, molecules = sf.batch_under(name)
    sf.compare(name, base, gpu_run(batch), molecules)
