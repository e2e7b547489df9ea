"""The clash score without a GPU: the radii and the threshold table, the new C entry (exported where the header says, argument
checked, ABI unchanged), ``compute_clashes`` on hand-written records, the numpy restatement ``clash_ref`` on a case worked by
hand, and the drivers' flag."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import clash_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radii_and_threshold_table():
    from difflinker_amd import const
    assert const.VDW_RADII == (1.70, 1.52, 1.55, 1.47, 1.80, 1.75, 1.85, 1.98, 1.80), 'Bondi, in GEOM index order'
    assert [const.GEOM_IDX2ATOM[k] for k in range(9)] == ['C', 'O', 'N', 'F', 'S', 'Cl', 'Br', 'I', 'P']
    geom, zinc = const.clash_threshold_table(True), const.clash_threshold_table(False)
    assert geom.shape == (9, 9) and zinc.shape == (8, 8) and geom.dtype == torch.float32
    assert torch.equal(geom[:8, :8], zinc) and torch.equal(geom, geom.T)
    assert geom[0, 0].item() == np.float32(2.55), 'C-C at the default: 0.75 * 3.4, rounded to fp32 once'
    for a in range(9):
        for b in range(9):
            want = np.float32(0.75 * (const.VDW_RADII[a] + const.VDW_RADII[b]) - 0.0)
            assert geom[a, b].item() == want, (a, b)
    plain = const.clash_threshold_table(True, scale=1.0)
    assert plain[0, 1].item() == np.float32(1.70 + 1.52) and plain[7, 7].item() == np.float32(1.98 + 1.98)
    shifted = const.clash_threshold_table(True, scale=1.0, tolerance=0.4)
    assert shifted[2, 4].item() == np.float32(1.0 * (1.55 + 1.80) - 0.4)
    assert (const.clash_threshold_table(True, scale=0.5, tolerance=5.0) < 0).all(), 'the table itself may go negative'


def test_non_positive_threshold_never_clashes():
    x = np.zeros((1, 2, 3), dtype=np.float32)                          # two atoms on top of each other: d2 = 0
    one_hot = np.eye(2, dtype=np.float32)[None]
    masks = dict(query_mask=[[1, 0]], target_mask=[[0, 1]])
    for t, want in ((0.0, 0), (-1.0, 0), (float('nan'), 0), (1e-30, 0), (0.5, 1), (float('inf'), 1)):
        got = clash_ref.clash_scores(x, one_hot, threshold=np.full((2, 2), t), **masks)
        assert got['n_clashes'][0] == want and got['n_contacts'][0] == 1 and got['min_dist2'][0] == 0, t


def test_reference_on_a_case_worked_by_hand():
    """``clash_ref``'s docstring: queries C (0,0,0) and O (10,0,0), targets N (2,0,0) and C (0,3,0), thresholds 2.5, cut-off 4.
    The rows are interleaved with a padding row that holds NaN, and the last row is set in both masks: a query only."""
    nan = float('nan')
    x = np.array([[[0, 0, 0], [2, 0, 0], [nan, nan, nan], [10, 0, 0], [0, 3, 0], [50, 50, 50]]], dtype=np.float32)
    types = [0, 2, 0, 1, 0, 0]
    one_hot = np.eye(3, dtype=np.float32)[types][None]
    first = dict(query_mask=[[1, 0, 0, 1, 0, 0]], target_mask=[[0, 1, 0, 0, 1, 0]])
    got = clash_ref.clash_scores(x, one_hot, threshold=np.full((3, 3), 2.5), **first)
    assert (got['n_query'][0], got['n_target'][0], got['status'][0]) == (2, 2, 0)
    assert (got['n_clashes'][0], got['n_clash_atoms'][0], got['n_contacts'][0], got['min_dist2'][0]) == (1, 1, 2, 4.0)
    assert got['atom_clashes'][0].tolist() == [1, 0, 0, 0, 0, 0]
    assert got['atom_min_dist2'][0].tolist() == [4.0, math.inf, math.inf, 64.0, math.inf, math.inf]
    both = clash_ref.clash_scores(x, one_hot, threshold=np.full((3, 3), 2.5), query_mask=[[1, 0, 0, 1, 0, 1]],
                                  target_mask=[[0, 1, 0, 0, 1, 1]])
    assert (both['n_query'][0], both['n_target'][0], both['n_clashes'][0]) == (3, 2, 1), 'a row in both masks is a query only'
    # the table is [query type][target type]: only C (query) against N (target) may clash
    directed = np.zeros((3, 3), dtype=np.float32)
    directed[0, 2] = 2.5
    assert clash_ref.clash_scores(x, one_hot, threshold=directed, **first)['n_clashes'][0] == 1
    assert clash_ref.clash_scores(x, one_hot, threshold=directed.T, **first)['n_clashes'][0] == 0
    # the shared list: the same two targets given once more, a type outside the table skipped, a NaN flagging the molecule
    shared = dict(protein_x=[[2, 0, 0], [0, 3, 0], [0, 0, 0]], protein_type=[2, 0, 3])
    got = clash_ref.clash_scores(x, one_hot, threshold=np.full((3, 3), 2.5), **first, **shared)
    assert (got['n_target'][0], got['n_clashes'][0], got['n_contacts'][0], got['status'][0]) == (4, 2, 4, clash_ref.BAD_TYPE)
    shared['protein_x'][0][1] = nan
    got = clash_ref.clash_scores(x, one_hot, threshold=np.full((3, 3), 2.5), **first, **shared)
    assert got['status'][0] == clash_ref.BAD_TYPE | clash_ref.NONFINITE and math.isnan(got['min_dist2'][0])
    assert (got['n_query'][0], got['n_target'][0], got['n_clashes'][0], got['n_contacts'][0]) == (0, 0, 0, 0)
    assert np.isnan(got['atom_min_dist2'][0][[0, 3]]).all() and np.isinf(got['atom_min_dist2'][0][[1, 2, 4, 5]]).all()
    # first largest entry, as the bond kernel reads a one-hot row
    assert clash_ref.first_maximum([[0, 1, 1], [2, 2, 2], [0, 0, 3], [-1, -2, -3]]).tolist() == [1, 0, 2, 0]


def test_export_declared_checked_and_abi_unchanged():
    from difflinker_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'difflinker_hip.h')).read()
    lib = _lib.load()
    assert 'int32_t dl_clash_scores(const dl_clash_args* args, void* stream);' in header and hasattr(lib, 'dl_clash_scores')
    at = _lib.EXPORTS.index('dl_molecule_keys')
    assert _lib.EXPORTS[at + 1] == 'dl_clash_scores' and _lib.EXPORTS[-1] == 'dl_best_rmsd', 'right after dl_molecule_keys'
    assert ' *   dl_clash_scores ' in header.split('#ifndef DIFFLINKER_HIP_H')[0], 'listed in the opening comment'
    assert _lib.ABI_VERSION == 7 and lib.dl_abi_version() == 7 and '#define DL_ABI_VERSION 7' in header
    for name, bit in (('DL_CLASH_NONFINITE', 1), ('DL_CLASH_TOO_LARGE', 2), ('DL_CLASH_BAD_TYPE', 4)):
        assert f'#define {name} {bit} ' in header and getattr(_lib, name) == bit
    assert (clash_ref.NONFINITE, clash_ref.TOO_LARGE, clash_ref.BAD_TYPE) == (1, 2, 4)
    # the struct's fields in the header's order
    body = header.split('typedef struct dl_clash_args {')[1].split('} dl_clash_args;')[0]
    declared = [part.strip(' *') for line in body.splitlines() if ';' in line
                for part in line.split(';')[0].split(None, 1 + line.strip().startswith('const'))[-1].split(',')]
    assert declared == [name for name, _ in _lib.DLClashArgs._fields_]
    # no GPU here: every refusal below comes back as DL_ERR_BAD_ARG (-1) before any device work
    assert lib.dl_clash_scores(None, None) == -1
    one = ctypes.c_void_p(16)                    # never dereferenced
    required = ('x', 'one_hot', 'query_mask', 'threshold', 'n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts',
                'min_dist2', 'status', 'atom_clashes', 'atom_min_dist2')
    ok = dict(B=2, N=8, nf=9, M=3, contact_cutoff=4.0, target_mask=one, target_x=one, target_type=one,
              **{k: one for k in required})
    refusals = [dict(B=-1), dict(N=0), dict(nf=0), dict(nf=17), dict(M=-1), dict(target_x=None), dict(target_type=None)]
    for bad in refusals + [{k: None} for k in required]:
        assert lib.dl_clash_scores(ctypes.byref(_lib.DLClashArgs(**dict(ok, **bad))), None) == -1, bad
    empty = _lib.DLClashArgs(B=0, N=8, nf=9)
    assert lib.dl_clash_scores(ctypes.byref(empty), None) == _lib.DL_OK, 'an empty batch is DL_OK without a launch'
    for field, value in (('N', 0), ('nf', 17), ('M', -1)):
        worse = _lib.DLClashArgs(B=0, N=8, nf=9)
        setattr(worse, field, value)
        assert lib.dl_clash_scores(ctypes.byref(worse), None) == -1, 'the sizes are checked before the empty batch'


def record(n_query=4, n_target=30, n_clashes=0, n_clash_atoms=0, n_contacts=0, min_distance=3.0, status=0):
    from difflinker_amd.metrics import ClashRecord
    return ClashRecord(n_query, n_target, n_clashes, n_clash_atoms, n_contacts, min_distance, status, [0] * n_query,
                       [min_distance] * n_query)


def test_compute_clashes_on_hand_written_records():
    from difflinker_amd.metrics import CLASH_NAMES, CLASH_TRUE_NAMES, compute_clashes
    pred = [record(n_clashes=3, n_clash_atoms=2, n_contacts=10, min_distance=1.5),
            record(n_query=6, n_contacts=4, min_distance=3.5),
            record(n_query=0, n_target=0, min_distance=math.inf),                        # no pair: out of the mean distance
            record(n_query=0, n_target=0, min_distance=math.nan, status=1),              # flagged: out of everything
            record(n_clashes=1, n_clash_atoms=1, n_contacts=1, min_distance=math.nan, status=2)]
    got = compute_clashes(pred)
    assert tuple(got) == CLASH_NAMES
    assert got == {'clash_molecules': 3, 'clash_flagged': 2, 'clash_free': 2 / 3, 'clashes_per_molecule': 1.0,
                   'clash_atoms_share': 2 / 10, 'contacts_per_molecule': 14 / 3, 'min_distance': 2.5}
    bad_type_only = compute_clashes([record(status=4, n_clashes=2, n_clash_atoms=1)])
    assert bad_type_only['clash_molecules'] == 1 and bad_type_only['clash_flagged'] == 0, 'a skipped atom does not void the rest'
    true = [record(n_clashes=1), record(n_clashes=2), record(), record(n_clashes=7), record(status=1)]
    with_true = compute_clashes(pred, true)
    assert tuple(with_true) == CLASH_NAMES + CLASH_TRUE_NAMES and {k: with_true[k] for k in CLASH_NAMES} == got
    assert with_true['true_clashes_per_molecule'] == 1.0 and with_true['true_clash_free'] == 1 / 3
    assert with_true['clash_excess'] == ((3 - 1) + (0 - 2) + 0) / 3
    nothing = compute_clashes([])
    assert nothing == {'clash_molecules': 0, 'clash_flagged': 0, 'clash_free': 0.0, 'clashes_per_molecule': 0.0,
                       'clash_atoms_share': 0.0, 'contacts_per_molecule': 0.0, 'min_distance': None}
    assert compute_clashes([record(n_query=0, n_target=0, min_distance=math.inf)])['min_distance'] is None
    with pytest.raises(ValueError):
        compute_clashes(pred, true[:2])


def test_cpu_tensors_raise():
    from difflinker_amd import _lib
    from difflinker_amd.metrics import analyze_clashes
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_clashes(torch.zeros(1, 4, 9), torch.zeros(1, 4, 3), torch.ones(1, 4))


def test_generate_clashes_needs_a_protein(tmp_path):
    """Raised before the model is loaded: the checkpoint named here does not exist."""
    from difflinker_amd import generate
    argv = ['--fragments', 'frag.sdf', '--model', str(tmp_path / 'missing.ckpt'), '--linker_size', '5',
            '--output', str(tmp_path / 'out'), '--clashes']
    with pytest.raises(ValueError, match='--pocket or --protein'):
        generate.main(argv)
    assert not (tmp_path / 'out').exists()
    with pytest.raises(ValueError, match='pocket or a protein'):
        generate.generate('frag.sdf', str(tmp_path / 'missing.ckpt'), str(tmp_path / 'out'), 1, 5, '5', clashes=True)


def test_drivers_parse_the_clashes_flag(monkeypatch, capsys):
    from difflinker_amd import generate, sample, train
    seen = []
    monkeypatch.setattr(sample, 'sample', lambda *a, **kw: seen.append(kw))
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p', '--clashes'])
    sample.main(['--checkpoint', 'c.ckpt', '--samples', 's', '--prefix', 'p'])
    assert seen == [{'clashes': True}, {}], 'without the flag the call is what it was'
    calls = []
    monkeypatch.setattr(generate, 'generate_with_pocket', lambda *a, **kw: calls.append(kw) or [])
    monkeypatch.setattr(generate, 'generate_with_protein', lambda *a, **kw: calls.append(kw) or [])
    common = ['--fragments', 'f.sdf', '--model', 'm.ckpt', '--linker_size', '5']
    generate.main(common + ['--pocket', 'p.pdb', '--clashes'])
    generate.main(common + ['--protein', 'p.pdb', '--clashes'])
    generate.main(common + ['--pocket', 'p.pdb'])
    assert [kw.get('clashes') for kw in calls] == [True, True, None]
    with pytest.raises(SystemExit):
        train.main(['--help'])
    assert '--clashes' in capsys.readouterr().out
    from difflinker_amd.lightning import DDPM
    import inspect
    assert 'self.clash_metrics = False' in inspect.getsource(DDPM.__init__)


def test_protein_atoms_helper():
    """All atoms of the file whose element is in the vocabulary, in file order, in the file's own frame."""
    from difflinker_amd import const
    from difflinker_amd.io import _walk_pdb, get_protein_atoms
    folder = os.path.join(ROOT, 'tests', 'golden', 'io', 'case_studies')
    path = next(os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.endswith('.pdb'))
    atoms = _walk_pdb(path)
    positions, types = get_protein_atoms(path)
    known = [a for a in atoms if a.element.capitalize() in const.GEOM_ATOM2IDX]
    assert len(known) == len(types) > 0 and positions.shape == (len(types), 3) and types.dtype == np.int32
    assert types.tolist() == [const.GEOM_ATOM2IDX[a.element.capitalize()] for a in known]
    assert positions.tolist() == [a.coord for a in known]
