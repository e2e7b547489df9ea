"""The restatement ``stereo_ref`` under every transform of ``frame_cases`` (the host twin of ``test_gpu_stereo_frames.py``),
and the clearance of the chosen cases."""
import pytest

import stereo_frame_cases as sf


@pytest.fixture(scope='module')
def base():
    return sf.host_run(sf.batch_under('identity')[0])


def test_every_case_clears_its_thresholds_under_every_transform():
    least = [sf.cleared(m) for m in sf.cases()]
    assert len(least) == len(sf.HAND) + len(sf.RANDOM) and min(least) >= sf.CLEARANCE, least


def test_the_cases_hold_both_hands_both_sides_and_the_undecided(base):
    labels = [s for r in base for s in r['atom_stereo']]
    bonds = [s for r in base for s in r['bond_stereo']]
    assert labels.count(1) >= 3 and labels.count(2) >= 3 and bonds.count(1) >= 2 and bonds.count(2) >= 2
    assert any('@' in r['isomeric_smiles'] for r in base) and any('/' in r['isomeric_smiles'] for r in base)
    assert sum(r['stereo_code'] != r['mirror_code'] for r in base) >= 4


@pytest.mark.parametrize('name', sf.TRANSFORMS[1:])
def test_the_restatement_under(name, base):
    batch, molecules = sf.batch_under(name)
    sf.compare(name, base, sf.host_run(batch), molecules)
