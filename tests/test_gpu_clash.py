"""``dl_clash_scores`` (csrc/clash.hip) on the GPU against its numpy-float32 restatement ``clash_ref``: every output EXACTLY,
the integers and the bits of the squared distances - the rule fixes every rounding, so there is no tolerance anywhere but
where coordinates went through a text file.  One mixed batch with the sizes at which the mapping changes (wave and workgroup
strides on the target side, the lane-group widths and the four-queries-per-thread path on the query side), the shared target
list, flagged molecules between good ones, and the public path through ``generate_with_pocket`` / ``generate_with_protein``."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import clash_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, 'golden', 'io', 'case_studies')
NF = 9
INT_FIELDS = ('n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts', 'status', 'atom_clashes')
FLOAT_FIELDS = ('min_dist2', 'atom_min_dist2')

# (query atoms, in-batch targets): target counts 0, 1, 63, 64, 65, 255, 256, 257, 600 (wave and workgroup strides of the tile);
# query counts 0, 1, 2, 64, 65, 110, and 128, 129, 256, 257, 600 - where the lane groups go from 4 to 2 to 1 and where a thread
# starts to hold more than one query
SIZES = [(0, 0), (1, 1), (2, 63), (64, 64), (65, 65), (110, 255), (1, 256), (2, 257), (110, 600), (0, 65), (64, 0),
         (128, 70), (129, 70), (256, 70), (257, 70), (600, 300)]
N_ROWS = 1000


def molecule(rng, n, nq, nt, both=0, box=20.0):
    """Rows in random order: ``nq`` queries, ``nt`` targets, ``both`` rows set in both masks, the rest padding that holds finite
    garbage.  All nine elements on both sides, coordinates in a box offset by 50 A."""
    x = (50.0 + rng.uniform(0, box, size=(n, 3))).astype(np.float32)
    one_hot = np.eye(NF, dtype=np.float32)[rng.integers(0, NF, size=n)]
    rows = rng.permutation(n)
    qm, tm = np.zeros(n, np.float32), np.zeros(n, np.float32)
    qm[rows[:nq + both]] = 1
    tm[rows[nq:nq + both + nt]] = 1
    return x, one_hot, qm, tm


def stack(mols):
    return tuple(np.stack(part) for part in zip(*mols))


@pytest.fixture(scope='module')
def mixed():
    from difflinker_amd import const
    rng = np.random.default_rng(2024)
    mols = [molecule(rng, N_ROWS, nq, nt) for nq, nt in SIZES]
    mols.append(molecule(rng, N_ROWS, 40, 100, both=5))                 # rows set in both masks: queries only
    # a molecule whose only clash is between its LAST query row and its LAST target row: queries and targets 100 A apart
    x, one_hot, qm, tm = molecule(rng, N_ROWS, 70, 300)
    x[tm != 0] += 100.0
    last_q, last_t = np.nonzero(qm)[0][-1], np.nonzero(tm)[0][-1]
    x[last_q] = np.float32([300.0, 300.0, 300.0])                       # away from every other atom of the molecule
    x[last_t] = np.float32([301.0, 300.0, 300.0])
    mols.append((x, one_hot, qm, tm))
    x, one_hot, qm, tm = stack(mols)
    threshold = const.clash_threshold_table(True).numpy()
    want = clash_ref.clash_scores(x, one_hot, qm, threshold, tm)
    for part in (x, one_hot, qm, tm, threshold, *want.values()):
        part.setflags(write=False)
    return dict(x=x, one_hot=one_hot, qm=qm, tm=tm, threshold=threshold, want=want)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda:0')


def score(x, one_hot, qm, tm=None, protein=None, **kw):
    from difflinker_amd.metrics import analyze_clashes
    shared = None if protein is None else (dev(np.asarray(protein[0]).reshape(-1, 3)), dev(protein[1], torch.int32))
    return analyze_clashes(dev(one_hot), dev(x), dev(qm), None if tm is None else dev(tm), protein=shared, **kw)


def assert_exact(got, want, what=''):
    for name in INT_FIELDS:
        assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), (what, name)
    for name in FLOAT_FIELDS:
        bits = getattr(got, name).cpu().numpy().view(np.int32)
        both_nan = np.isnan(getattr(got, name).cpu().numpy()) & np.isnan(want[name])
        assert np.array_equal(np.where(both_nan, 0, bits), np.where(both_nan, 0, want[name].view(np.int32))), (what, name)


def launch_prefilled(x, one_hot, qm, tm, threshold, cutoff=4.0):
    """The C entry on output buffers that hold 0x7f bytes (fp32 3.4e38, a huge int32): what ``analyze_clashes`` does, with the
    outputs in the test's hands."""
    from difflinker_amd import _lib
    B, N, nf = one_hot.shape
    stale = lambda *shape: torch.full(shape, 0x7f, dtype=torch.uint8, device='cuda:0')      # noqa: E731
    names = ('n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts', 'min_dist2', 'status')
    out = {name: stale(B, 4) for name in names}
    out.update(atom_clashes=stale(B, N, 4), atom_min_dist2=stale(B, N, 4))
    ins = dict(x=dev(x), one_hot=dev(one_hot), query_mask=dev(qm), target_mask=dev(tm), threshold=dev(threshold))
    args = _lib.DLClashArgs(B=B, N=N, nf=nf, M=0, contact_cutoff=cutoff, **{k: v.data_ptr() for k, v in ins.items()},
                            **{k: v.data_ptr() for k, v in out.items()})
    _lib.check(_lib.load().dl_clash_scores(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'clash')
    torch.cuda.synchronize()
    view = lambda name: out[name].view(torch.float32 if name in FLOAT_FIELDS else torch.int32).squeeze(-1)   # noqa: E731
    return {name: view(name) for name in out}


def test_mixed_batch_exact_and_independent_of_stale_memory(mixed):
    m = mixed
    first = score(m['x'], m['one_hot'], m['qm'], m['tm'])
    assert_exact(first, m['want'], 'mixed batch')
    assert int(first.status.abs().sum()) == 0 and int(first.n_clashes.sum()) > 1000, 'the batch does hold clashes'
    last = len(SIZES) + 1
    assert int(first.n_clashes[last]) == 1 and int(first.n_clash_atoms[last]) == 1 and float(first.min_dist2[last]) == 1.0
    again = score(m['x'], m['one_hot'], m['qm'], m['tm'])
    # once more with every padding row of every input NaN and every output pre-filled
    padding = (m['qm'] == 0) & (m['tm'] == 0)
    x, one_hot = m['x'].copy(), m['one_hot'].copy()
    x[padding] = np.nan
    one_hot[padding] = np.nan
    stale = launch_prefilled(x, one_hot, m['qm'], m['tm'], m['threshold'])
    for name in INT_FIELDS + FLOAT_FIELDS:
        assert torch.equal(getattr(first, name), getattr(again, name)), name
        assert torch.equal(getattr(first, name), stale[name]), name


def test_strict_comparison():
    """Thresholds all 2.0: atoms exactly 2.0 apart do not clash (4 < 4 is false); with the target one fp32 step closer they do."""
    x = np.zeros((2, 2, 3), dtype=np.float32)
    x[0, 1, 0] = 2.0
    x[1, 1, 0] = np.nextafter(np.float32(2.0), np.float32(0.0))
    one_hot = np.eye(NF, dtype=np.float32)[[[0, 3], [0, 3]]]
    qm, tm = np.float32([[1, 0], [1, 0]]), np.float32([[0, 1], [0, 1]])
    threshold = np.full((NF, NF), 2.0, dtype=np.float32)
    got = score(x, one_hot, qm, tm, thresholds=dev(threshold))
    assert got.n_clashes.tolist() == [0, 1] and got.n_contacts.tolist() == [1, 1]
    assert_exact(got, clash_ref.clash_scores(x, one_hot, qm, threshold, tm), 'strict')
    moved = score(x, one_hot, qm, tm, thresholds=dev(threshold), contact_cutoff=2.0)
    assert moved.n_contacts.tolist() == [0, 1], 'the contact cut-off is strict too'


@pytest.mark.parametrize('own', [True, False], ids=['with_own_targets', 'shared_only'])
@pytest.mark.parametrize('M', [0, 1, 257, 5000])
def test_shared_target_list(mixed, M, own):
    pick = [1, 4, 5, 9, 16]                                             # 1, 65, 110, 0 and 40 (+5) queries
    x, one_hot, qm = mixed['x'][pick], mixed['one_hot'][pick], mixed['qm'][pick]
    tm = mixed['tm'][pick] if own else None
    rng = np.random.default_rng(M)
    px = (50.0 + rng.uniform(0, 20.0, size=(M, 3))).astype(np.float32)
    pt = rng.integers(0, NF, size=M).astype(np.int32)
    got = score(x, one_hot, qm, tm, protein=(px, pt))
    want = clash_ref.clash_scores(x, one_hot, qm, mixed['threshold'], tm, px, pt)
    assert_exact(got, want, f'M={M}')
    assert got.status.tolist() == [0] * len(pick)
    if M >= 257:
        assert int(got.n_clashes.sum()) > 0
        # a type of -1 and one of nf: skipped, bit 4, everything else stands
        pt_bad = pt.copy()
        pt_bad[[3, M - 1]] = [-1, NF]
        got = score(x, one_hot, qm, tm, protein=(px, pt_bad))
        assert_exact(got, clash_ref.clash_scores(x, one_hot, qm, mixed['threshold'], tm, px, pt_bad), 'bad types')
        assert got.status.tolist() == [4] * len(pick)
        assert got.n_target.tolist() == [n - 2 for n in want['n_target']]
        # a NaN in the shared list flags every molecule
        px_bad = px.copy()
        px_bad[M - 2, 1] = np.nan
        got = score(x, one_hot, qm, tm, protein=(px_bad, pt))
        assert_exact(got, clash_ref.clash_scores(x, one_hot, qm, mixed['threshold'], tm, px_bad, pt), 'shared NaN')
        assert got.status.tolist() == [1] * len(pick) and int(got.n_clashes.sum()) == 0
        assert bool(torch.isnan(got.min_dist2).all())


def test_flagged_molecules_leave_their_neighbours_alone(mixed):
    pick = [5, 4, 8, 3, 16]                                             # good, NaN query, good, infinite target, good
    x, one_hot, qm, tm = (mixed[k][pick].copy() for k in ('x', 'one_hot', 'qm', 'tm'))
    x[1, np.nonzero(qm[1])[0][7], 2] = np.nan
    x[3, np.nonzero(tm[3])[0][-1], 0] = np.inf
    got = score(x, one_hot, qm, tm)
    assert_exact(got, clash_ref.clash_scores(x, one_hot, qm, mixed['threshold'], tm), 'flagged')
    assert got.status.tolist() == [0, 1, 0, 1, 0]
    for b in (1, 3):
        assert [int(getattr(got, n)[b]) for n in ('n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts')] == [0] * 5
        assert int(got.atom_clashes[b].abs().sum()) == 0 and bool(torch.isnan(got.min_dist2[b]))
        assert bool(torch.isnan(got.atom_min_dist2[b][dev(qm[b]) != 0]).all())
        assert bool(torch.isinf(got.atom_min_dist2[b][dev(qm[b]) == 0]).all())
    good = [0, 2, 4]
    alone = score(x[good], one_hot[good], qm[good], tm[good])
    for name in INT_FIELDS + FLOAT_FIELDS:
        assert torch.equal(getattr(got, name)[good], getattr(alone, name)), name


def test_too_many_query_atoms():
    rng = np.random.default_rng(5)
    mols = [molecule(rng, 1100, 1025, 10), molecule(rng, 1100, 30, 200), molecule(rng, 1100, 1024, 40)]
    x, one_hot, qm, tm = stack(mols)
    threshold = np.full((NF, NF), 2.5, dtype=np.float32)
    got = score(x, one_hot, qm, tm, thresholds=dev(threshold))
    assert_exact(got, clash_ref.clash_scores(x, one_hot, qm, threshold, tm), 'too large')
    assert got.status.tolist() == [2, 0, 0] and got.n_query.tolist() == [0, 30, 1024]
    assert int(got.n_clashes[0]) == 0 and bool(torch.isnan(got.min_dist2[0])) and int(got.n_clashes[2]) > 0


def test_single_molecule_empty_batch_and_cpu_tensors(mixed):
    from difflinker_amd import _lib
    from difflinker_amd.metrics import analyze_clashes, clashes_to_host
    b = 5
    one = score(mixed['x'][b:b + 1], mixed['one_hot'][b:b + 1], mixed['qm'][b:b + 1], mixed['tm'][b:b + 1])
    for name in INT_FIELDS + FLOAT_FIELDS:
        assert np.array_equal(getattr(one, name).cpu().numpy(), mixed['want'][name][b:b + 1]), name
    record = clashes_to_host(one)[0]
    rows = mixed['qm'][b] != 0
    assert record.n_clashes == mixed['want']['n_clashes'][b] and len(record.atom_clashes) == 110 == record.n_query
    assert record.atom_clashes == mixed['want']['atom_clashes'][b][rows].tolist()
    assert record.min_distance == float(np.sqrt(np.float64(mixed['want']['min_dist2'][b])))
    assert record.atom_min_distance == np.sqrt(mixed['want']['atom_min_dist2'][b][rows].astype(np.float64)).tolist()
    none = score(np.zeros((0, 7, 3)), np.zeros((0, 7, NF)), np.zeros((0, 7)), np.zeros((0, 7)))
    assert none.n_clashes.shape == (0,) and none.atom_clashes.shape == (0, 7) and clashes_to_host(none) == []
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_clashes(torch.zeros(1, 4, NF), torch.zeros(1, 4, 3), torch.ones(1, 4))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        analyze_clashes(dev(np.zeros((1, 4, NF))), dev(np.zeros((1, 4, 3))), torch.ones(1, 4))


# ---- the public path ------------------------------------------------------------------------------------------------------
def pocket_file(tmp_path, protein, fragments):
    """The residues of the committed case-study protein with an atom within 6 A of the fragments, as a PDB file of their own."""
    lines = [ln for ln in open(protein) if ln[:6] in ('ATOM  ', 'HETATM')]
    xyz = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in lines])
    near = np.linalg.norm(xyz[:, None] - np.asarray(fragments)[None], axis=-1).min(1) <= 6.0
    residues = {ln[21:27] for ln, hit in zip(lines, near) if hit}
    path = str(tmp_path / 'pocket.pdb')
    with open(path, 'w') as f:
        f.writelines(ln for ln in lines if ln[21:27] in residues)
    return path


def check_written(out_dir, files, n_frag, targets, target_types, n_target):
    """``clashes.json`` and ``metrics.json`` of a run against ``clash_ref`` on what the run wrote.

    THE BOUND on ``min_distance``.  The files hold ``%.9f`` coordinates: a value read back is within 5e-10 of the fp32 value
    the kernel saw, and IS that value after rounding to fp32 whenever the coordinate is at least 2^-6 in size (half an fp32
    step then exceeds 5e-10); a smaller one lands within 1e-9.  The protein's coordinates are the same fp32 values on both
    sides.  So a pair's true distance moves by at most sqrt(3) * 1e-9 < 2e-9.  Each side then evaluates the distance in fp32
    with every operation within e = 2^-24 relative: a difference (e), its square (2e + e), two sums of non-negative terms
    (2e more) - d2 within 5e - and the square root, taken in fp64 on both sides, halves that: d within 2.5e per side, 5e for the two.
    The test allows |d_json - d_ref| <= 2e-9 + 12 * 2^-24 * d."""
    from difflinker_amd import const
    from difflinker_amd.metrics import CLASH_NAMES
    from test_gpu_generate import read_xyz
    records = json.load(open(os.path.join(out_dir, 'clashes.json')))
    assert sorted(records) == sorted(os.path.basename(f) for f in files) and len(records) == 3
    threshold = const.clash_threshold_table(True).numpy()
    total = 0
    for f in files:
        syms, pos = read_xyz(f)
        linker = np.arange(len(syms)) >= n_frag
        x = np.concatenate([pos, targets])[None].astype(np.float32)
        types = [const.GEOM_ATOM2IDX[s] for s in syms] + list(target_types)
        qm = np.concatenate([linker, np.zeros(len(targets), bool)])[None]
        tm = np.concatenate([np.zeros(len(syms), bool), np.ones(len(targets), bool)])[None]
        want = clash_ref.clash_scores(x, np.eye(NF, dtype=np.float32)[types][None], qm, threshold, tm)
        got = records[os.path.basename(f)]
        assert want['n_query'][0] == 5 and want['n_target'][0] == n_target
        assert got['n_clashes'] == want['n_clashes'][0] and got['n_clash_atoms'] == want['n_clash_atoms'][0]
        d = float(np.sqrt(np.float64(want['min_dist2'][0])))
        assert abs(got['min_distance'] - d) <= 2e-9 + 12 * 2.0 ** -24 * d
        total += got['n_clashes']
    scores = json.load(open(os.path.join(out_dir, 'metrics.json')))
    assert set(CLASH_NAMES) <= set(scores) and 'clash_excess' not in scores
    assert scores['clash_molecules'] == 3 and scores['clash_flagged'] == 0
    assert scores['clashes_per_molecule'] == total / 3
    return scores


def test_generate_with_pocket_scores_the_written_molecules(tmp_path):
    from difflinker_amd import DDPM, io
    from difflinker_amd.generate import generate_with_pocket
    from test_gpu_generate import ddpm_hparams
    sdf = os.path.join(CASES, 'jnk_fragments.sdf')
    frag = io.read_molecule(sdf)
    pocket = pocket_file(tmp_path, os.path.join(CASES, 'jnk_protein_12A.pdb'), frag.positions)
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(True))
    kw = dict(backbone_atoms_only=False, model=ddpm, n_samples=3, n_steps=5, linker_size='5', random_seed=3)
    files = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'scored'), clashes=True, **kw)
    pos, one_hot, _ = io.pocket_arrays(io.read_pocket(pocket), False)
    assert 100 < len(pos) < 400
    scores = check_written(str(tmp_path / 'scored'), files, len(frag), pos, one_hot.argmax(1), len(pos))
    assert 'valence_validity' not in scores, 'alone when --metrics is not given'
    plain = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'plain'), **kw)
    assert [open(a, 'rb').read() for a in files] == [open(b, 'rb').read() for b in plain], 'the molecules do not change'
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(os.path.basename(f) for f in plain), 'no JSON without the flag'
    both = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'both'), clashes=True, metrics=True, **kw)
    scores = check_written(str(tmp_path / 'both'), both, len(frag), pos, one_hot.argmax(1), len(pos))
    assert 'valence_validity' in scores and scores['molecules'] == 3, 'beside the --metrics keys when both are given'
    with_metrics = generate_with_pocket(sdf, pocket, output_dir=str(tmp_path / 'metrics'), metrics=True, **kw)
    assert not os.path.exists(tmp_path / 'metrics' / 'clashes.json') and len(with_metrics) == 3
    assert not set(json.load(open(tmp_path / 'metrics' / 'metrics.json'))) & {'clash_free', 'clash_molecules', 'min_distance'}


def test_generate_with_protein_scores_against_the_whole_protein(tmp_path):
    from difflinker_amd import DDPM, io
    from difflinker_amd.generate import generate_with_protein
    from test_gpu_generate import ddpm_hparams
    sdf, pdb = os.path.join(CASES, 'jnk_fragments.sdf'), os.path.join(CASES, 'jnk_protein_12A.pdb')
    frag = io.read_molecule(sdf)
    torch.manual_seed(0)
    ddpm = DDPM(**ddpm_hparams(True))
    kw = dict(backbone_atoms_only=False, model=ddpm, n_samples=3, n_steps=5, linker_size='5', random_seed=3)
    files = generate_with_protein(sdf, pdb, output_dir=str(tmp_path / 'scored'), clashes=True, **kw)
    positions, types = io.get_protein_atoms(pdb)
    n_pocket = len(io.get_pocket(frag, pdb)[0])
    assert len(types) == 685 > n_pocket > 100, 'every in-vocabulary atom of the file, not the 6 A pocket the model saw'
    check_written(str(tmp_path / 'scored'), files, len(frag), positions, types, len(types))
    plain = generate_with_protein(sdf, pdb, output_dir=str(tmp_path / 'plain'), **kw)
    assert [open(a, 'rb').read() for a in files] == [open(b, 'rb').read() for b in plain]
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(os.path.basename(f) for f in plain)
