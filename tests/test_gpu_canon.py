"""``dl_canonical_ranks`` (``csrc/canon.hip``) on the GPU against ``tests/canon_ref.py``, bit for bit - ranks, code, leaf
count and status - on the smallest shapes at which each part of the kernel can go wrong, every batch mixing sizes in one
launch; the wrappers' input handling; and ``generate`` / ``sample`` with ``--smiles`` end to end."""
import csv
import filecmp
import functools
import json
import os
import random

import pytest
import torch

import canon_cases as cc
import canon_ref as cr
import mol_keys_ref as kr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NF = 8
FIELDS = ('rank', 'code', 'n_leaves', 'status')


def molecule(types, entries, keep=None, status=0, n_bonds=None):
    return dict(types=list(types), entries=[tuple(e) for e in entries], keep=keep, status=status, n_bonds=n_bonds)


def batch_of(molecules, N, scatter=True, capacity=None):
    """Host tensors of a batch: the atoms of molecule ``b`` on ``len(types)`` of ``N`` rows (scattered in row order among
    padding rows unless ``scatter`` is off), the bond list as given, and a ``Bonds`` around it."""
    from difflinker_amd.molecule_builder import Bonds
    B = len(molecules)
    capacity = max([len(m['entries']) for m in molecules] + [1]) if capacity is None else capacity
    one_hot, mask, drop = torch.zeros(B, N, NF), torch.zeros(B, N), torch.zeros(B, N)
    bonds = torch.full((B, capacity, 3), 0x7F7F7F7F, dtype=torch.int32)
    n_bonds, status = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, m in enumerate(molecules):
        n = len(m['types'])
        rows = sorted(random.Random(b).sample(range(N), n)) if scatter else list(range(n))
        for k, r in enumerate(rows):
            mask[b, r] = 1
            one_hot[b, r, m['types'][k]] = 1
            if m['keep'] is not None and not m['keep'][k]:
                drop[b, r] = 1
        for e, row in enumerate(m['entries'][:capacity]):
            bonds[b, e] = torch.tensor(row, dtype=torch.int32)
        n_bonds[b] = len(m['entries']) if m['n_bonds'] is None else m['n_bonds']
        status[b] = m['status']
    zeros = torch.zeros(B, N, dtype=torch.int32)
    found = Bonds(n_bonds, bonds, zeros, torch.ones(B, dtype=torch.int32), zeros.clone(), status)
    return one_hot, mask, drop, found


def reference(molecules, N, max_leaves=256, capacity=None):
    """What the kernel must write for ``batch_of(molecules, N, capacity=capacity)``: the four outputs as lists.  The kernel
    reads ``min(max(n_bonds, 0), capacity)`` entries (those beyond the molecule's own hold the batch's filler, which is no
    bond) and adds ``DL_BONDS_OVERFLOW`` when ``n_bonds`` exceeds the capacity."""
    capacity = max([len(m['entries']) for m in molecules] + [1]) if capacity is None else capacity
    out = {name: [] for name in FIELDS}
    for m in molecules:
        given = len(m['entries']) if m['n_bonds'] is None else m['n_bonds']
        read = min(max(given, 0), capacity)
        entries = (m['entries'][:capacity] + [(0x7F7F7F7F,) * 3] * capacity)[:read]
        got = cr.canonical_ranks(m['types'], entries, m['keep'], max_leaves, m['status'] | (1 if given > capacity else 0))
        out['rank'].append(got['rank'] + [-1] * (N - len(m['types'])))
        out['code'].append(kr.signed(got['code']))
        out['n_leaves'].append(got['n_leaves'])
        out['status'].append(got['status'])
    return out


def on_device(found, place=lambda t: t.to(DEV)):
    return type(found)(*(place(t) for t in found))


def launch(batch, max_leaves=256, with_drop=True, place=lambda t: t.to(DEV)):
    from difflinker_amd.metrics import canonical_ranks
    one_hot, mask, drop, found = batch
    return canonical_ranks(place(one_hot), place(mask), on_device(found, place), False,
                           drop_mask=place(drop) if with_drop else None, max_leaves=max_leaves)


def assert_equals_reference(got, want, names=None):
    for name in FIELDS:
        a = got[name].cpu().tolist()
        for b in range(len(a)):
            assert a[b] == want[name][b], (name, b, names[b] if names else None)


def named(name):
    return molecule(*cc.NAMED[name][:2])


def pieces(k):
    return molecule([cc.C] * (2 * k), [(2 * i, 2 * i + 1, 1) for i in range(k)])


@functools.lru_cache(maxsize=None)
def edge_molecules():
    """name -> molecule: the smallest shapes at which each part of the kernel can go wrong."""
    middle = [not 3 <= k < 9 for k in range(14)]                             # a middle block of rows removed
    ring14 = cc.ring(14, [1, 2])
    out = {
        'no atoms': molecule([], []),
        'one atom': molecule([cc.O], []),
        'two bonded atoms': molecule([cc.C, cc.C], [(1, 0, 1)]),              # a two-cell that is no twin cell
        'status carried': molecule([cc.C, cc.O], [(0, 1, 2)], status=2),
        'dropped middle block': molecule([cc.C, cc.N] * 7, ring14, keep=middle),
        'everything dropped': molecule([cc.C] * 3, [(0, 1, 1), (1, 2, 1)], keep=[False] * 3),
        'repeated pair': molecule([cc.C] * 4, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 0, 2)]),
        'entry out of range': molecule([cc.C] * 4, [(0, 1, 1), (1, 2, 1), (2, 4, 1), (2, 3, 1)]),
        'order out of range and a loop': molecule([cc.C] * 3, [(0, 1, 4), (1, 1, 1), (1, 2, 1)]),
        'negative count': molecule([cc.C] * 3, [(0, 1, 1), (1, 2, 1)], n_bonds=-5),
        'chain 257': molecule(*cc.chain(257)),
        'chain 257, one dropped': molecule(*cc.chain(257), keep=[k != 128 for k in range(257)]),
    }
    for name in ('neopentane', 'cf3_cyclohexane', 'benzene', 'six_ring', 'cubane', 'cuneane', 'two_ethanes', 'sulfone', 'decalin'):
        out[name] = named(name)
    for n in (63, 64, 65, 255, 256):
        out[f'chain {n}'] = molecule(*cc.chain(n))
    return out


@functools.lru_cache(maxsize=None)
def edge_reference():
    names = list(edge_molecules())
    molecules = [edge_molecules()[name] for name in names]
    return names, molecules, reference(molecules, 300, capacity=256)


# ---- bit-exactness ----------------------------------------------------------------------------------------------------------------
def test_every_edge_shape_in_one_launch():
    names, molecules, want = edge_reference()
    got = launch(batch_of(molecules, 300, capacity=256))
    assert_equals_reference(got, want, names)
    at = {name: b for b, name in enumerate(names)}
    leaves, status = got['n_leaves'].cpu().tolist(), got['status'].cpu().tolist()
    for name, n in (('neopentane', 1), ('cf3_cyclohexane', 2), ('benzene', 6), ('six_ring', 12), ('cubane', 48), ('cuneane', 12),
                    ('two_ethanes', 8), ('two bonded atoms', 2), ('chain 256', 2), ('no atoms', 1), ('chain 257', 0)):
        assert leaves[at[name]] == n, name
    assert status[at['chain 257']] == cr.TOO_LARGE and status[at['chain 257, one dropped']] == 0
    assert status[at['repeated pair']] == status[at['entry out of range']] == cr.BAD_BOND and status[at['status carried']] == 2
    assert status[at['negative count']] == 0 and leaves[at['negative count']] == 6, 'three atoms and no bond: 3! leaves, no twins'
    assert int(got['code'][at['no atoms']]) == kr.signed(kr.mix2(kr.mix2(kr.SEED_KEY, 0), 0))
    for b, m in enumerate(molecules):                                        # a permutation over the kept atoms, whatever the status
        kept = sorted(r for r in got['rank'][b].cpu().tolist() if r >= 0)
        n_kept = sum(m['keep']) if m['keep'] is not None else len(m['types'])
        assert kept == (list(range(n_kept)) if leaves[b] else []), names[b]


def test_a_list_cut_short_at_its_capacity():
    """``n_bonds`` beyond the capacity: the first ``capacity`` entries are the graph and ``DL_BONDS_OVERFLOW`` is added; a count
    beyond the molecule's own entries reads the filler behind them, which is no bond."""
    molecules = [molecule(*cc.chain(4)), molecule(*cc.chain(3), n_bonds=1000), molecule(*cc.chain(3), n_bonds=3), named('benzene')]
    got = launch(batch_of(molecules, 7, capacity=2))
    want = reference(molecules, 7, capacity=2)
    assert_equals_reference(got, want)
    assert want['status'] == [1, 1, 1, 1], 'three, 1000 and three entries claimed, six listed: all beyond a capacity of two'
    got = launch(batch_of(molecules[:3], 7, capacity=4))
    want = reference(molecules[:3], 7, capacity=4)
    assert_equals_reference(got, want)
    assert want['status'] == [0, 1 | cr.BAD_BOND, cr.BAD_BOND]


def test_an_empty_batch():
    got = launch(batch_of([], 5))
    assert [tuple(got[name].shape) for name in FIELDS] == [(0, 5), (0,), (0,), (0,)]


def test_without_a_drop_mask_and_unscattered():
    names, molecules, _ = edge_reference()
    chosen = [m for name, m in zip(names, molecules) if m['keep'] is None and len(m['types']) <= 65 and m['n_bonds'] is None]
    got = launch(batch_of(chosen, 65, scatter=False), with_drop=False)
    assert_equals_reference(got, reference(chosen, 65))


@pytest.mark.parametrize('max_leaves,budget', [(1, True), (4, True), (47, True), (48, False)])
def test_the_leaf_budget_of_cubane(max_leaves, budget):
    molecules = [named('cubane'), named('benzene'), named('cuneane'), named('neopentane')]
    got = launch(batch_of(molecules, 12), max_leaves=max_leaves)
    assert_equals_reference(got, reference(molecules, 12, max_leaves))
    assert int(got['n_leaves'][0]) == max_leaves and bool(int(got['status'][0]) & cr.BUDGET) == budget
    assert sorted(got['rank'][0].cpu().tolist())[4:] == list(range(8))


def test_the_depth_budget():
    """33 separate two-atom pieces give a path of 33 branching levels (``test_canon_host.test_the_depth_budget``): 66 atoms
    reach ``DL_CANON_MAX_DEPTH`` well within 256.  32 pieces stay within it and stop at the leaf budget instead."""
    molecules = [pieces(cr.MAX_DEPTH + 1), pieces(cr.MAX_DEPTH), pieces(3), named('benzene')]
    for max_leaves in (1, 3):
        got = launch(batch_of(molecules, 70), max_leaves=max_leaves)
        assert_equals_reference(got, reference(molecules, 70, max_leaves))
        status = got['status'].cpu().tolist()
        assert status[0] == cr.BUDGET and status[1] == cr.BUDGET and status[3] == cr.BUDGET


# ---- renumbering on the device ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_pairs():
    rng = random.Random(11)
    originals = [cc.random_graph(seed) for seed in range(100)]
    return originals, [cc.renumber(t, b, rng) for t, b in originals]


def test_renumbered_copies_get_the_same_code_and_string():
    from difflinker_amd.metrics import smiles_to_host
    originals, copies = random_pairs()
    results, strings = [], []
    for graphs in (originals, copies):
        molecules = [molecule(t, b) for t, b in graphs]
        batch = batch_of(molecules, 24)
        got = launch(batch)
        assert_equals_reference(got, reference(molecules, 24))
        one_hot, mask, drop, found = batch
        results.append(got)
        strings.append(smiles_to_host(got, one_hot, mask, found, drop))
    assert torch.equal(results[0]['code'], results[1]['code']) and torch.equal(results[0]['n_leaves'], results[1]['n_leaves'])
    assert strings[0] == strings[1] and None not in strings[0]
    assert int(results[0]['status'].abs().sum()) == 0 and len(set(strings[0])) > 90


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_batch():
    names = ('cubane', 'benzene', 'two_ethanes', 'neopentane', 'sulfone')
    molecules = [named(name) for name in names] + [edge_molecules()['dropped middle block'], edge_molecules()['status carried']]
    return molecules, batch_of(molecules, 16)


@pytest.mark.parametrize('form', ['strided', 'sliced', 'wide'])
def test_input_forms(form):
    """Strided, sliced and float64 / int64 / bool inputs, the ``Bonds`` members included, give the canonical run's bits and
    nothing is written to an input or around it."""
    import input_forms as F
    molecules, batch = small_batch()
    want = reference(molecules, 16)
    keep = []

    def place(t):
        out = F.BY_NAME[form](t, DEV)
        keep.append((F.buffer_of(out), F.as_bytes(F.buffer_of(out)).clone()))
        return out
    got = launch(batch, place=place)
    torch.cuda.synchronize()
    assert_equals_reference(got, want)
    assert len(keep) == 9
    for buf, copy in keep:
        assert torch.equal(F.as_bytes(buf), copy)
    one_hot, mask, drop, found = batch
    squeezed = launch((one_hot, mask.reshape(7, 16, 1), drop.reshape(7, 16, 1), found))
    assert_equals_reference(squeezed, want)


def test_stale_output_memory(monkeypatch):
    """Every output element is written whatever the buffers held before (the harness of ``test_gpu_scratch.py``)."""
    import test_gpu_scratch as SC
    molecules, batch = small_batch()
    more = molecules + [molecule(*cc.chain(17))]                             # and a molecule that fills every row
    batch = batch_of(more, 17)

    def run():
        got = launch(batch)
        torch.cuda.synchronize()
        return SC.Ran(got, [(name, got[name], got[name].element_size() * got[name].numel()) for name in FIELDS])
    got = SC.check_contract(monkeypatch, run)
    assert_equals_reference(got, reference(more, 17))


def test_arguments_are_checked_before_the_launch():
    from difflinker_amd.metrics import canonical_ranks
    _, (one_hot, mask, drop, found) = small_batch()
    with pytest.raises(ValueError, match='max_leaves'):
        launch((one_hot, mask, drop, found), max_leaves=0)
    with pytest.raises(ValueError, match='shapes disagree'):
        canonical_ranks(one_hot.to(DEV), mask[:, :5].to(DEV), on_device(found), False)
    from difflinker_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        canonical_ranks(one_hot, mask, found, False)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def strings_of_file(path, n_linker):
    """``(smiles, linker_smiles, code as hex)`` of a written ``.sdf`` file under the reference, from the file alone."""
    from difflinker_amd.molecule_builder import smiles
    from test_gpu_fingerprint import written
    types, bonds, linker = written(path, n_linker)
    whole = cr.canonical_ranks(types, bonds)
    part = cr.canonical_ranks(types, bonds, keep=linker)
    new = {k: at for at, k in enumerate(k for k in range(len(types)) if linker[k])}
    linker_text = smiles([types[k] for k in new], [(new[i], new[j], o) for i, j, o in bonds if i in new and j in new],
                         [part['rank'][k] for k in new])
    assert not (whole['status'] | part['status'])
    return smiles(types, bonds, whole['rank']), linker_text, format(whole['code'], '016x')


def read_csv(path):
    from difflinker_amd.metrics import SMILES_COLUMNS
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == SMILES_COLUMNS == ('file', 'smiles', 'linker_smiles', 'code', 'canonical')
    return [dict(zip(rows[0], row)) for row in rows[1:]]


def test_generate_writes_the_strings_and_changes_no_file(tmp_path, monkeypatch):
    """``generate`` behind the sampler, as ``test_gpu_select.test_generate_selects_among_valid_samples`` drives it: hand-made
    linkers that bridge two fragments stand in for sampled ones (the synthetic checkpoint on ``frag.sdf`` gives no sample
    in one piece).  Samples 0 and 1 are one molecule under two numberings - the linker rows of sample 1 are those of sample
    0 in reverse order - and sample 2 is another molecule."""
    import test_gpu_select as SEL
    from difflinker_amd.generate import generate
    monkeypatch.setattr(SEL, 'LINKERS', ('CNCC', 'CNCC', 'CCOC'))
    ddpm = SEL.synthetic_ddpm()

    def chain_of(data, sample_fn=None, keep_frames=None):
        chain, mask = SEL.bridging_chain(data, ddpm)
        chain[0, 1, 5:] = chain[0, 1, 5:].flip(0)                            # the four linker rows of sample 1, backwards
        return chain, mask
    monkeypatch.setattr(ddpm, 'sample_chain', chain_of, raising=False)
    frag = str(tmp_path / 'bridge.sdf')
    with open(frag, 'w') as f:
        f.write(SEL.BRIDGE_SDF)
    runs = {}
    for tag, flags in (('plain', {}), ('strings', {'smiles': True}), ('both', {'smiles': True, 'metrics': True}),
                       ('scores', {'metrics': True})):
        torch.manual_seed(11)
        runs[tag] = generate(frag, ddpm, str(tmp_path / tag), n_samples=3, n_steps=5, linker_size='4', output_format='both', **flags)
    names = [os.path.basename(path) for path in runs['plain']]
    assert len(names) == 6 and all([os.path.basename(path) for path in runs[tag]] == names for tag in runs)
    for tag, added in (('strings', {'smiles.csv'}), ('both', {'smiles.csv', 'metrics.json'}), ('scores', {'metrics.json'})):
        assert set(os.listdir(tmp_path / tag)) - set(os.listdir(tmp_path / 'plain')) == added, tag
        for name in sorted(os.listdir(tmp_path / 'plain')):
            assert filecmp.cmp(tmp_path / 'plain' / name, tmp_path / tag / name, shallow=False), (tag, name)
    assert filecmp.cmp(tmp_path / 'strings' / 'smiles.csv', tmp_path / 'both' / 'smiles.csv', shallow=False)
    rows = read_csv(tmp_path / 'both' / 'smiles.csv')
    assert [row['file'] for row in rows] == names, 'one row per written file, in the order they were written'
    by_sample = {}
    for row in rows:
        sample = row['file'].rsplit('_.', 1)[0]
        want = strings_of_file(tmp_path / 'both' / f'{sample}_.sdf', 4)
        assert (row['smiles'], row['linker_smiles'], row['code']) == want and row['canonical'] == '1', row
        by_sample[sample] = want
    first, second, third = (by_sample[f'output_{k}_bridge'] for k in range(3))
    assert first == second and third[0] != first[0] and third[2] != first[2]
    from difflinker_amd.metrics import Graph, same_molecule
    linker = cc.parse_smiles(first[1])
    assert same_molecule(Graph(linker[0], linker[1], None), Graph([cc.C, cc.N, cc.C, cc.C], [(0, 1, 1), (1, 2, 1), (2, 3, 1)], None)), first
    assert '.' not in first[0] and sorted(cc.parse_smiles(first[0])[0]) == sorted([cc.C] * 7 + [cc.N] * 2)
    scores = json.load(open(tmp_path / 'both' / 'metrics.json'))
    plain_scores = json.load(open(tmp_path / 'scores' / 'metrics.json'))
    assert {k: v for k, v in scores.items() if not k.startswith('smiles_')} == plain_scores
    assert scores['validity_and_connectivity'] == 1.0 and scores['uniqueness'] == 2 / 3
    assert scores['smiles_uniqueness'] == scores['uniqueness'] and scores['smiles_canonical'] == 1.0, 'no budget hit: share zero'


def test_sample_writes_the_strings_and_changes_no_file(tmp_path):
    import test_gpu_rings as RG
    from difflinker_amd.sample import sample
    m = RG.gentle_model(tmp_path, False)
    outs = {}
    for tag, flags in (('plain', {'metrics': True}), ('strings', {'metrics': True, 'smiles': True})):
        m.edm.noise_seed = 5
        outs[tag] = sample(m, str(tmp_path / tag), 'zinc_final_test', 2, str(DEV), data=str(tmp_path), n_steps=5,
                           output_format='sdf', **flags)
    plain, out = outs['plain'], outs['strings']
    names = sorted(os.path.join(u, name) for u in os.listdir(out) if os.path.isdir(os.path.join(out, u))
                   for name in os.listdir(os.path.join(out, u)))
    for name in names:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain))) == ['smiles.csv']
    rows = read_csv(os.path.join(out, 'smiles.csv'))
    sampled = [name for name in names if name.endswith('_.sdf')]
    assert sorted(row['file'] for row in rows) == sampled and len(sampled) == 10, 'one row per written file'
    from difflinker_amd.io import read_sdf_molecules
    from difflinker_amd import const
    from difflinker_amd.molecule_builder import smiles
    for row in rows:
        (mol,), _ = read_sdf_molecules(os.path.join(out, row['file']))
        types = [const.ATOM2IDX[s] for s in mol.symbols]
        whole = cr.canonical_ranks(types, list(mol.bonds))
        assert row['smiles'] == smiles(types, list(mol.bonds), whole['rank']) and row['code'] == format(whole['code'], '016x'), row
        assert row['canonical'] == '1'
    scores, plain_scores = json.load(open(os.path.join(out, 'metrics.json'))), json.load(open(os.path.join(plain, 'metrics.json')))
    assert {k: v for k, v in scores.items() if not k.startswith('smiles_')} == plain_scores
    assert scores['smiles_uniqueness'] == scores['uniqueness'] and scores['smiles_canonical'] == 1.0
