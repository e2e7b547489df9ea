"""Pocket selection on the GPU (``dl_pocket_select``, ``csrc/pocket.hip``) against the numpy fp64 rule of ``tests/pocket_ref.py``.
Every output is a flag, a count or a position and every comparison is exact.  Every launch of ``launch`` writes into outputs
pre-filled with 0x5a bytes, so no result may depend on stale memory.  The public path (``select_all`` + ``pocket_examples``,
``python -m difflinker_amd.prepare --proteins``, a training step on what it wrote) comes last."""
import ctypes
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

import pocket_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = pocket_ref.FIELDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO_DIR = os.path.join(ROOT, 'tests', 'golden', 'io')
CASES = os.path.join(IO_DIR, 'case_studies')
GARBAGE = np.array([np.nan, np.inf, -1e300])     # what ligand rows with mask 0 hold: never read


def residues(rng, n_atoms, centre, box, first_group=0, spread=1.5):
    """``n_atoms`` protein atoms in runs of 1..12 that share a group, each run a blob around a point of the box around ``centre``."""
    x, group, g = [], [], first_group
    while len(x) < n_atoms:
        middle = centre + rng.uniform(-box / 2, box / 2, 3)
        for _ in range(min(int(rng.integers(1, 13)), n_atoms - len(x))):
            x.append(middle + rng.normal(0, spread, 3))
            group.append(g)
        g += 1
    return np.array(x, dtype=np.float32).reshape(n_atoms, 3), np.array(group, dtype=np.int32)


def ligand(rng, n_atoms, centre=(0.0, 0.0, 0.0), spread=2.0):
    return np.round(np.asarray(centre) + rng.normal(0, spread, (n_atoms, 3)), 4)          # SDF decimals


def pack(rng, proteins, pairs, width=None):
    """``proteins``: list of ``(x [M,3], group [M])``; ``pairs``: list of ``(protein number, ligand [n,3])``.  The real ligand
    rows are scattered over ``width`` rows; the others hold garbage and mask 0."""
    width = max([len(lig) for _, lig in pairs] + [1]) + 3 if width is None else width
    B = len(pairs)
    out = {'protein_x': np.concatenate([x for x, _ in proteins] + [np.zeros((0, 3), np.float32)]).astype(np.float32),
           'protein_group': np.concatenate([g for _, g in proteins] + [np.zeros(0, np.int32)]).astype(np.int32),
           'protein_offset': np.concatenate([[0], np.cumsum([len(g) for _, g in proteins])]).astype(np.int32),
           'pair_protein': np.array([p for p, _ in pairs], dtype=np.int32).reshape(B),
           'ligand_x': rng.choice(GARBAGE, (B, width, 3)), 'ligand_mask': np.zeros((B, width), np.float32)}
    for b, (_, lig) in enumerate(pairs):
        real = np.sort(rng.choice(width, len(lig), replace=False))
        out['ligand_x'][b, real] = lig
        out['ligand_mask'][b, real] = 1
    return out


def dev(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def tensors(case):
    return (dev(case['protein_x'], torch.float32), dev(case['protein_group'], torch.int32), dev(case['protein_offset'], torch.int32),
            dev(case['pair_protein'], torch.int32), dev(case['ligand_x'], torch.float64), dev(case['ligand_mask'], torch.float32))


def launch(case, R, Mmax=None, cutoff=6.0):
    """``dl_pocket_select`` itself, into outputs full of 0x5a bytes.  Returns a dict of numpy arrays."""
    from difflinker_amd import _lib
    B, L = case['ligand_mask'].shape
    M_total = len(case['protein_group'])
    Mmax = M_total if Mmax is None else Mmax
    names = ('protein_x', 'protein_group', 'protein_offset', 'pair_protein', 'ligand_x', 'ligand_mask')
    ins = dict(zip(names, tensors(case)))
    shapes = {'n_ligand': (B,), 'n_contact_atoms': (B,), 'n_groups_selected': (B,), 'n_pocket': (B,), 'status': (B,),
              'member': (B, Mmax), 'index': (B, R)}
    outs = {k: torch.full(s, 0x5a, dtype=torch.uint8, device=DEV) if k == 'member' else
            torch.full(s, 0x5a5a5a5a, dtype=torch.int32, device=DEV) for k, s in shapes.items()}
    ptr = lambda t: None if t.numel() == 0 else t.data_ptr()                                        # noqa: E731
    args = _lib.DLPocketArgs(B=B, L=L, P=len(case['protein_offset']) - 1, M_total=M_total, cutoff=cutoff, Mmax=Mmax, capacity=R,
                             **{k: ptr(t) for k, t in ins.items()}, **{k: ptr(t) for k, t in outs.items()})
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    _lib.check(_lib.load().dl_pocket_select(ctypes.byref(args), stream), 'dl_pocket_select')
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in outs.items()}


def reference(case, R, Mmax=None, cutoff=6.0):
    return pocket_ref.select_pockets(case['protein_x'], case['protein_group'], case['protein_offset'], case['pair_protein'],
                                     case['ligand_x'], case['ligand_mask'], cutoff, Mmax, R)


def assert_exact(got, want, what=''):
    if not isinstance(got, dict):
        got = {name: getattr(got, name).cpu().numpy() for name in FIELDS}
    for name in FIELDS:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


PROTEIN_SIZES = (0, 1, 255, 256, 257, 513)       # the edges of the 256-atom tiles
LIGAND_SIZES = (0, 1, 63, 64, 65, 256, 257)      # 257: DL_POCKET_TOO_LARGE


def test_tile_edges_and_ligand_sizes():
    rng = np.random.default_rng(1)
    proteins = [residues(rng, m, np.zeros(3), 34.0) for m in PROTEIN_SIZES]
    pairs = [(p, ligand(rng, n)) for p in range(len(PROTEIN_SIZES)) for n in LIGAND_SIZES]
    case = pack(rng, proteins, pairs, width=300)
    want = reference(case, 600)
    got = launch(case, 600)
    assert_exact(got, want)
    assert want['n_ligand'].tolist() == list(LIGAND_SIZES) * len(PROTEIN_SIZES)
    assert (want['status'] == pocket_ref.TOO_LARGE).tolist() == [n == 257 for _, lig in pairs for n in [len(lig)]]
    assert not want['n_pocket'][want['n_ligand'] == 0].any(), 'no ligand atom: nothing is selected'
    last = {n: want['n_pocket'][len(LIGAND_SIZES) * 5 + k] for k, n in enumerate(LIGAND_SIZES)}     # the protein of 513 atoms
    assert 0 < last[1] < last[64] < 513 and last[257] == 0
    again = launch(case, 600)
    assert all(got[name].tobytes() == again[name].tobytes() for name in FIELDS), 'the same batch twice: the same bytes'


def line_protein(groups_of_atoms, near):
    """Atom k at (3 k' , 0, 0) when its group is in ``near`` (k' counts those: within 6 A for k' <= 2), else 50 A away."""
    x, close = [], 0
    for k, g in enumerate(groups_of_atoms):
        if g in near and close < 3:
            x.append([3.0 * close, 0.0, 0.0])
            close += 1
        else:
            x.append([50.0 + k, 0.0, 0.0])
    return np.array(x, np.float32).reshape(len(groups_of_atoms), 3), np.array(groups_of_atoms, np.int32)


def test_groups_and_word_edges_of_the_bitset():
    rng = np.random.default_rng(2)
    top = pocket_ref.MAX_GROUPS
    proteins = [line_protein(list(range(n)) * 2, {n - 1}) for n in (1, 31, 32, 33)]                  # the last group is touched
    proteins.append(line_protein([0, 31, 32, 33, 63, 64, top - 1, 5, top - 1], {31, 32, top - 1}))
    proteins.append(line_protein([0, 1, top, 2], {1}))                                              # one id too many
    proteins.append(line_protein([0, 1, -1, 2], {1}))
    proteins.append(line_protein([7, 3, 4, 7, 5, 7], {7}))               # chain A's residue 7, other residues, chain B's residue 7
    origin = np.zeros((1, 3))
    case = pack(rng, proteins, [(p, origin) for p in range(len(proteins))])
    want = reference(case, 80)
    got = launch(case, 80)
    assert_exact(got, want)
    assert want['n_groups_selected'].tolist() == [1, 1, 1, 1, 3, 0, 0, 1]
    assert want['n_pocket'].tolist() == [2, 2, 2, 2, 4, 0, 0, 3] and want['index'][7, :4].tolist() == [0, 3, 5, -1]
    assert want['index'][4, :5].tolist() == [1, 2, 6, 8, -1] and want['member'][4, :9].tolist() == [0, 3, 3, 0, 0, 0, 3, 0, 2]
    assert want['status'].tolist() == [0] * 5 + [pocket_ref.TOO_MANY_GROUPS] * 2 + [0]


def test_the_boundary_is_inside():
    rng = np.random.default_rng(3)
    six, up = np.float32(6), np.nextafter(np.float32(6), np.float32(np.inf))
    x = np.array([[six, 0, 0], [up, 0, 0], [0, six, 0], [0, 0, -six], [0, -up, 0], [np.nextafter(six, np.float32(0)), 0, 0]], np.float32)
    proteins = [(x, np.arange(6, dtype=np.int32))]
    # cut-offs 3.5 (its square is exact) and 3.7, 3.3 (no fp64 numbers; their squares round): fp32 neighbours of the cut-off on
    # an axis and on the diagonals, where d2 itself rounds
    for c in (3.5, 3.7, 3.3):
        near = [np.float32(c)]
        for _ in range(3):
            near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
        rows = [[v, 0, 0] for v in near] + [[v / np.sqrt(np.float32(3))] * 3 for v in near] + \
               [[v * np.float32(0.6), v * np.float32(0.8), 0] for v in near]
        proteins.append((np.array(rows, np.float32), np.arange(len(rows), dtype=np.int32)))
    origin = np.zeros((1, 3))
    case = pack(rng, proteins, [(0, origin)])
    want = reference(case, 8)
    assert_exact(launch(case, 8), want, 6.0)
    assert want['member'][0, :6].tolist() == [3, 0, 3, 3, 0, 3], '(6, 0, 0) and (0, 6, 0) are selected, the next fp32 number is not'
    for p, c in enumerate((3.5, 3.7, 3.3), start=1):
        case = pack(rng, proteins, [(p, origin), (0, origin)])
        want = reference(case, 24, cutoff=c)
        assert_exact(launch(case, 24, cutoff=c), want, c)
        inside = want['member'][0, :21] != 0
        assert inside[:3].all() and not inside[4:7].any() and 0 < inside.sum() < 21, (c, inside.tolist())
        assert inside[3] == (float(np.float32(c)) <= c), 'fp32(3.7) lies above 3.7, fp32(3.5) is 3.5 and fp32(3.3) lies below 3.3'


def test_nonfinite_coordinates():
    rng = np.random.default_rng(4)
    good = residues(rng, 300, np.zeros(3), 20.0)
    nan_far = (good[0].copy(), good[1])
    nan_far[0][299, 1] = np.nan                                          # in the second tile
    inf_near = (good[0].copy(), good[1])
    inf_near[0][0, 0] = -np.inf
    lig = ligand(rng, 9)
    bad = lig.copy()
    bad[8, 2] = np.inf
    case = pack(rng, [good, nan_far, inf_near], [(0, lig), (1, lig), (2, lig), (0, bad), (0, lig)], width=12)
    hidden = np.nonzero(case['ligand_mask'][4] == 0)[0]
    case['ligand_x'][4, hidden] = np.nan                                 # a masked row does not count
    want = reference(case, 300)
    got = launch(case, 300)
    assert_exact(got, want)
    assert want['status'].tolist() == [0, pocket_ref.NONFINITE, pocket_ref.NONFINITE, pocket_ref.NONFINITE, 0]
    assert want['n_pocket'][0] == want['n_pocket'][4] > 0 and want['n_ligand'].tolist() == [9] * 5
    assert not got['member'][1:4].any() and (got['index'][1:4] == -1).all() and not got['n_pocket'][1:4].any()


def test_capacity_truncation_and_select_all():
    from difflinker_amd.pocket import select_all, select_pockets
    rng = np.random.default_rng(5)
    proteins = [residues(rng, m, np.zeros(3), 24.0) for m in (400, 150, 30)]
    case = pack(rng, proteins, [(0, ligand(rng, 12)), (1, ligand(rng, 5)), (2, ligand(rng, 3, centre=(200.0, 0.0, 0.0)))])
    full = reference(case, 400)
    n = full['n_pocket'].tolist()
    assert n[0] > n[1] > 0 and n[2] == 0
    for R in (0, n[1] - 1, n[1], n[0] - 1, n[0], n[0] + 7):              # R = 0: `index` is NULL
        want = reference(case, R)
        got = launch(case, R)
        assert_exact(got, want, R)
        assert got['n_pocket'].tolist() == n, 'the count is complete'
        assert (got['status'] & pocket_ref.TRUNCATED != 0).tolist() == [n[0] > R, n[1] > R, False]
        assert np.array_equal(got['index'], full['index'][:, :R]) and np.array_equal(got['member'], full['member'])
    assert (full['index'][1, n[1]:] == -1).all()
    assert_exact(select_pockets(*tensors(case), capacity=5), reference(case, 5), 'the wrapper')
    assert_exact(select_pockets(*tensors(case), capacity=5, max_atoms=401, cutoff=4.5), reference(case, 5, 401, 4.5), 'its options')
    assert_exact(select_all(*tensors(case), capacity=5), reference(case, n[0]), 'widened once')
    assert_exact(select_all(*tensors(case)), reference(case, 512), 'wide enough from the start')


def test_shared_proteins_any_order_bad_pairs_and_the_empty_batch():
    rng = np.random.default_rng(6)
    proteins = [residues(rng, m, np.zeros(3), 26.0) for m in (300, 40, 0, 270)]
    order = [3, 0, 3, 1, 2, 0, 3, 0]
    case = pack(rng, proteins, [(p, ligand(rng, int(rng.integers(1, 30)))) for p in order])
    want = reference(case, 300)
    assert_exact(launch(case, 300), want)
    assert (want['n_pocket'][[0, 2, 6]] > 0).all() and len({int(v) for v in want['n_pocket'][[0, 2, 6]]}) > 1
    assert_exact(launch(case, 300, Mmax=300), reference(case, 300, Mmax=300), 'member rows as wide as the largest protein')
    # pairs that point at no protein, and a row of `member` below a protein's size: answered with a status, nothing is touched
    case['pair_protein'][[1, 4]] = [4, -1]
    want = reference(case, 300, Mmax=280)
    assert_exact(launch(case, 300, Mmax=280), want, 'bad pairs')
    assert want['status'].tolist() == [0, pocket_ref.BAD_PROTEIN, 0, 0, pocket_ref.BAD_PROTEIN, pocket_ref.BAD_PROTEIN, 0,
                                       pocket_ref.BAD_PROTEIN]
    crossed = dict(case, pair_protein=np.array(order, np.int32), protein_offset=np.array([0, 300, 290, 340, 611], np.int32))
    want = reference(crossed, 64)
    assert_exact(launch(crossed, 64), want, 'offsets that do not ascend')
    assert want['status'][[3, 4]].tolist() == [pocket_ref.BAD_PROTEIN, 0]
    none = dict(case, pair_protein=case['pair_protein'][:0], ligand_x=case['ligand_x'][:0], ligand_mask=case['ligand_mask'][:0])
    got = launch(none, 4)
    assert got['index'].shape == (0, 4) and got['n_pocket'].shape == (0,)
    bare = pack(rng, [], [(0, ligand(rng, 2))])                          # no protein at all: protein_x and protein_group are NULL
    assert_exact(launch(bare, 3), reference(bare, 3), 'no proteins')


def test_batch_independence():
    rng = np.random.default_rng(7)
    proteins = [residues(rng, m, np.zeros(3), 26.0) for m in (520, 90)]
    mine, other, big = (0, ligand(rng, 17)), (1, ligand(rng, 40)), (1, ligand(rng, 257))
    width = 260
    alone = launch(pack(rng, proteins, [mine], width), 64)
    assert alone['n_pocket'][0] > 64 and alone['status'][0] == pocket_ref.TRUNCATED
    for pairs, at in (([mine, other, other], 0), ([other, other, mine], 2), ([big, mine, big], 1), ([other, big, mine, mine], 3)):
        got = launch(pack(rng, proteins, pairs, width), 64)
        for name in FIELDS:
            assert got[name][at].tobytes() == alone[name][0].tobytes(), (at, name)


def test_random_pairs():
    rng = np.random.default_rng(8)
    proteins, first = [], 0
    for _ in range(60):
        first = int(rng.integers(0, 3000))                               # dense ids need not start at 0 for the kernel
        proteins.append(residues(rng, int(rng.integers(1, 601)), np.zeros(3), 30.0, first_group=first))
    pairs = [(int(rng.integers(0, 60)), ligand(rng, int(rng.integers(1, 41)), centre=rng.uniform(-8, 8, 3))) for _ in range(200)]
    case = pack(rng, proteins, pairs, width=48)
    want = reference(case, 64, Mmax=600)
    got = launch(case, 64, Mmax=600)
    assert_exact(got, want)
    sizes = np.diff(case['protein_offset'])[case['pair_protein']]
    some = (want['n_pocket'] > 0) & (want['n_pocket'] < sizes)
    print(f'{int(some.sum())} of 200 pairs select a pocket that is neither empty nor the whole protein')
    assert some.sum() >= 100 and (want['status'] & pocket_ref.TRUNCATED).any() and (want['status'] == 0).any()
    assert (want['n_contact_atoms'] < want['n_pocket']).any(), 'residues ride along with their contact atoms'


FIXTURES = {
    'toy': (os.path.join(IO_DIR, 'protein.pdb'), os.path.join(IO_DIR, 'frag.sdf')),
    'hsp90_whole': (os.path.join(CASES, 'hsp90', '3hz1_protein.pdb'), os.path.join(CASES, 'hsp90_fragments.sdf')),
    'hsp90_12A': (os.path.join(CASES, 'hsp90_protein_12A.pdb'), os.path.join(CASES, 'hsp90_fragments.sdf')),
    'jnk_12A': (os.path.join(CASES, 'jnk_protein_12A.pdb'), os.path.join(CASES, 'jnk_fragments.sdf')),
}


def hand_item(mol):
    """A ``fragment.examples`` dict of a molecule whose last two atoms are called the linker."""
    from difflinker_amd import const, io
    pos, one_hot, charges = io.parse_molecule(mol, is_geom=True)
    n = len(mol)
    tensor = lambda v: torch.tensor(np.asarray(v), dtype=const.TORCH_FLOAT)                          # noqa: E731
    linker = torch.tensor([0.0] * (n - 2) + [1.0] * 2)
    anchors = torch.zeros(n)
    anchors[[0, n - 3]] = 1
    return {'uuid': 0, 'name': mol.name, 'positions': tensor(pos), 'one_hot': tensor(one_hot), 'charges': tensor(charges),
            'anchors': anchors, 'fragment_mask': 1 - linker, 'linker_mask': linker, 'num_atoms': n}


def test_fixtures_through_select_all_and_pocket_examples():
    """All four fixture pairs in ONE batch (the two hsp90 files serve the same ligand), then the data-set dicts."""
    from difflinker_amd import io
    from difflinker_amd.pocket import pocket_atoms, pocket_examples
    from difflinker_amd.prepare import select_ligand_pockets
    names = list(FIXTURES)
    proteins = [io.read_pdb_arrays(FIXTURES[name][0]) for name in names]
    mols = [io.read_molecule(FIXTURES[name][1]) for name in names]
    chosen = select_ligand_pockets([m.positions for m in mols], proteins, list(range(len(names))), torch.device(DEV))
    for name, protein, mol, idx in zip(names, proteins, mols, chosen):
        for mode, bb in (('full', False), ('bb', True)):
            want = io.get_pocket(mol, FIXTURES[name][0], backbone_atoms_only=bb)
            got = pocket_atoms(protein.coords[idx], [protein.name[j] for j in idx], [protein.element[j] for j in idx], mode)
            assert np.array_equal(got[0], np.asarray(want[0], dtype=np.float32)), (name, mode)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and len(want[2]) > 0, (name, mode)
            (item,) = pocket_examples([hand_item(mol)], [got])
            n, m = len(mol), len(want[2])
            assert item['num_atoms'] == n + m and item['pocket_mask'].tolist() == [0.0] * (n - 2) + [1.0] * m + [0.0] * 2
            assert torch.equal(item['positions'][n - 2:n - 2 + m], torch.tensor(np.asarray(want[0]), dtype=torch.float32))
            assert torch.equal(item['one_hot'][n - 2:n - 2 + m], torch.tensor(want[1], dtype=torch.float32))
            assert item['anchors'].nonzero().flatten().tolist() == [0, n - 3]


def test_prepare_with_proteins_then_a_training_step(tmp_path, capsys):
    import fragment_ref
    from difflinker_amd import const, io, prepare, train
    from difflinker_amd.datasets import MOADDataset
    ligands = {'3hz1': os.path.join(CASES, 'hsp90', '3hz1_ligand_obabel.sdf'), '3fi3': os.path.join(CASES, 'jnk', '3fi3_ligand.sdf')}
    proteins = os.path.join(tmp_path, 'proteins')
    os.makedirs(proteins)
    shutil.copy(os.path.join(CASES, 'hsp90', '3hz1_protein.pdb'), os.path.join(proteins, '3hz1_protein.pdb'))
    shutil.copy(os.path.join(CASES, 'jnk_protein_12A.pdb'), os.path.join(proteins, '3fi3_protein.pdb'))
    sdf = os.path.join(tmp_path, 'ligands.sdf')
    with open(sdf, 'w') as out:
        for code, path in ligands.items():
            with open(path) as f:
                out.write(f.read())
        with open(ligands['3hz1']) as f:
            out.write(f.read().replace('3hz1_ligand', '9xyz_ligand', 1))                            # its protein is not there
    molecules, malformed = io.read_sdf_molecules(sdf)
    assert malformed == 0 and [m.name for m in molecules] == ['3hz1_ligand', '3fi3_ligand', '9xyz_ligand']
    cuts = {}
    for m in molecules[:2]:                                                                         # the default rule cuts both
        n = len(m)
        one_hot = np.eye(const.GEOM_NUMBER_OF_ATOM_TYPES)[[const.GEOM_ATOM2IDX[s] for s in m.symbols]]
        cuts[m.name] = fragment_ref.molecule([1.0] * n, one_hot.tolist(), list(m.bonds), len(m.bonds), 64, m.charges,
                                             carbon_type=const.GEOM_ATOM2IDX['C'])['n_cuts']
    assert min(cuts.values()) >= 1
    total = sum(cuts.values())

    summary = prepare.main(['--sdf', sdf, '--out', str(tmp_path), '--prefix', 'mine', '--proteins', proteins, '--geom', '--device', DEV])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary['examples'] == total >= 1 and summary['files'] == {'mine': total} and summary['molecules_read'] == 3
    assert summary['molecules_skipped']['no_protein_file'] == 1 and summary['molecules_skipped']['empty_pocket'] == 0
    want = {(m.name, mode): io.get_pocket(m, prepare.protein_path(proteins, m.name), backbone_atoms_only=mode == 'bb')
            for m in molecules[:2] for mode in ('full', 'bb')}
    with open(os.path.join(tmp_path, 'mine_table.csv')) as f:
        table = [row.split(',') for row in f.read().splitlines()]
    assert tuple(table[0]) == prepare.POCKET_TABLE_COLUMNS and len(table) == total + 1
    size = {m.name: len(m) for m in molecules}
    for row in table[1:]:
        row = dict(zip(table[0], row))
        assert int(row['pocket_full_size']) == len(want[row['molecule'], 'full'][2])
        assert int(row['pocket_bb_size']) == len(want[row['molecule'], 'bb'][2]) and int(row['molecule_size']) == size[row['molecule']]
        assert int(row['fragments_size']) == int(row['n_frag_1']) + int(row['n_frag_2']) and row['linker_size'] == row['n_linker']
        assert int(row['fragments_size']) + int(row['linker_size']) == int(row['molecule_size'])
    for mode in ('full', 'bb'):
        data = MOADDataset(data_path=str(tmp_path), prefix=f'mine.{mode}', device='cpu')
        assert len(data) == total and [item['uuid'] for item in data] == list(range(total))
        assert [item['name'] for item in data] == [name for name, k in cuts.items() for _ in range(k)]
        for item, row in zip(data, table[1:]):
            pos, one_hot, charges = want[item['name'], mode]
            n_frag, n_pock, n_link = int(row[table[0].index('fragments_size')]), len(charges), int(row[table[0].index('linker_size')])
            assert item['num_atoms'] == n_frag + n_pock + n_link == len(item['positions'])
            assert item['fragment_only_mask'].tolist() == [1.0] * n_frag + [0.0] * (n_pock + n_link)
            assert item['pocket_mask'].tolist() == [0.0] * n_frag + [1.0] * n_pock + [0.0] * n_link
            assert item['fragment_mask'].tolist() == [1.0] * (n_frag + n_pock) + [0.0] * n_link
            assert item['linker_mask'].tolist() == [0.0] * (n_frag + n_pock) + [1.0] * n_link
            block = slice(n_frag, n_frag + n_pock)
            assert torch.equal(item['positions'][block], torch.tensor(np.asarray(pos), dtype=torch.float32))
            assert torch.equal(item['one_hot'][block], torch.tensor(one_hot, dtype=torch.float32))
            assert torch.equal(item['charges'][block], torch.tensor(charges, dtype=torch.float32))
            assert item['anchors'].nonzero().flatten().tolist() == sorted([int(row[2]), int(row[3])])
            assert max(int(row[2]), int(row[3])) < n_frag and all(item[k].dtype == const.TORCH_FLOAT for k in list(item)[2:10])
    # --pocket_by residue: chain-aware groups select no more than the reference's rule
    narrow = prepare.main(['--sdf', sdf, '--out', str(tmp_path), '--prefix', 'narrow', '--proteins', proteins, '--pocket_by', 'residue',
                           '--pocket_cutoff', '4.5', '--device', DEV])
    assert narrow['examples'] == total
    small = MOADDataset(data_path=str(tmp_path), prefix='narrow.full', device='cpu')
    assert all(a['num_atoms'] < b['num_atoms'] for a, b in zip(small, MOADDataset(data_path=str(tmp_path), prefix='mine_full', device='cpu')))

    # split by molecule, then one optimiser step of the pocket trainer on what was written
    split = prepare.main(['--sdf', sdf, '--out', str(tmp_path), '--prefix', 'MOAD', '--proteins', proteins, '--val_fraction', '0.5',
                          '--seed', '1', '--pocket_by', 'residue', '--pocket_cutoff', '4.5', '--device', DEV])
    assert sorted(split['files'].values()) == sorted(cuts.values())
    for part in ('train', 'val'):
        assert all(os.path.exists(os.path.join(tmp_path, f'MOAD_{part}_{mode}.pt')) for mode in ('full', 'bb'))
        assert len(MOADDataset(data_path=str(tmp_path), prefix=f'MOAD_{part}.bb', device='cpu')) == split['files'][f'MOAD_{part}']
    cfg = os.path.join(tmp_path, 'cfg.yml')
    with open(cfg, 'w') as f:
        f.write('nf: 128\nn_layers: 1\ninv_sublayers: 1\ntanh: False\nattention: False\nnorm_constant: 0.000001\n'
                'normalization_factor: 100\ninclude_charges: False\nbatch_size: 3\nlr: 0.0002\nnormalize_factors: [1, 4, 10]\n'
                'train_data_prefix: MOAD_train.full\nval_data_prefix: MOAD_val.full\ngraph_type: FC-10A-4A\n'
                'data_augmentation: True\n')
    capsys.readouterr()
    train.main(['--config', cfg, '--data', str(tmp_path), '--checkpoints', os.path.join(tmp_path, 'ck'), '--max_steps', '1',
                '--no_validation', '--device', DEV])
    steps = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines() if '"loss"' in ln]
    assert [s['step'] for s in steps] == [1] and math.isfinite(steps[0]['loss'])
