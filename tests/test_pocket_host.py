"""Pockets without a GPU: the ABI of ``dl_pocket_select``, the numpy rule of ``tests/pocket_ref.py`` against the reference's
``get_pocket`` as ``oracle/io_oracle.py`` and ``io.get_pocket`` state it, ``io.read_pdb_arrays`` / ``io.groups``,
``pocket.pocket_examples`` on hand-made inputs and the argument checks of the entry, which come before any device work."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pocket_ref
from difflinker_amd import _lib, const, io, pocket
from difflinker_amd.datasets import collate, collate_with_fragment_without_pocket_edges
from oracle import io_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO_DIR = os.path.join(ROOT, 'tests', 'golden', 'io')
CASES = os.path.join(IO_DIR, 'case_studies')
BAD_ARG = -1                                     # dl_status of include/difflinker_hip.h
FIXTURES = {                                     # protein, ligand
    'toy': (os.path.join(IO_DIR, 'protein.pdb'), os.path.join(IO_DIR, 'frag.sdf')),
    'hsp90_whole': (os.path.join(CASES, 'hsp90', '3hz1_protein.pdb'), os.path.join(CASES, 'hsp90_fragments.sdf')),
    'hsp90_12A': (os.path.join(CASES, 'hsp90_protein_12A.pdb'), os.path.join(CASES, 'hsp90_fragments.sdf')),
    'jnk_12A': (os.path.join(CASES, 'jnk_protein_12A.pdb'), os.path.join(CASES, 'jnk_fragments.sdf')),
}


def test_exports_header_and_constants():
    assert _lib.ABI_VERSION == 7
    at = _lib.EXPORTS.index('dl_fragment_cuts')
    assert _lib.EXPORTS[at + 1] == 'dl_pocket_select' and _lib.EXPORTS[at - 1] == 'dl_ring_scores' and _lib.EXPORTS[-1] == 'dl_best_rmsd'
    with open(os.path.join(ROOT, 'include', 'difflinker_hip.h')) as f:
        header = f.read()
    assert 'int32_t dl_pocket_select(const dl_pocket_args* args, void* stream);' in header and '#define DL_ABI_VERSION 7' in header
    for name, value in (('DL_POCKET_MAX_LIGAND', 256), ('DL_POCKET_MAX_GROUPS', 32768), ('DL_POCKET_NONFINITE', 1),
                        ('DL_POCKET_TOO_LARGE', 2), ('DL_POCKET_TOO_MANY_GROUPS', 4), ('DL_POCKET_BAD_PROTEIN', 8),
                        ('DL_POCKET_TRUNCATED', 32)):
        assert f'#define {name} {value} ' in header and getattr(_lib, name) == value
    assert (pocket_ref.MAX_LIGAND, pocket_ref.MAX_GROUPS, pocket_ref.NONFINITE, pocket_ref.TOO_LARGE, pocket_ref.TOO_MANY_GROUPS,
            pocket_ref.BAD_PROTEIN, pocket_ref.TRUNCATED) == \
        (_lib.DL_POCKET_MAX_LIGAND, _lib.DL_POCKET_MAX_GROUPS, _lib.DL_POCKET_NONFINITE, _lib.DL_POCKET_TOO_LARGE,
         _lib.DL_POCKET_TOO_MANY_GROUPS, _lib.DL_POCKET_BAD_PROTEIN, _lib.DL_POCKET_TRUNCATED)
    lib = _lib.load()
    assert lib.dl_abi_version() == 7 and hasattr(lib, 'dl_pocket_select')
    assert [name for name, _ in _lib.DLPocketArgs._fields_] == [
        'B', 'L', 'P', 'M_total', 'protein_x', 'protein_group', 'protein_offset', 'pair_protein', 'ligand_x', 'ligand_mask',
        'cutoff', 'Mmax', 'capacity', 'n_ligand', 'n_contact_atoms', 'n_groups_selected', 'n_pocket', 'status', 'member', 'index']
    assert pocket.Pockets._fields == pocket_ref.FIELDS


def test_struct_size_is_the_compilers(tmp_path):
    """``sizeof(dl_pocket_args)`` and the offsets of its first and last pointer, from the C compiler that reads the header."""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc, 'a C compiler is needed to read include/difflinker_hip.h'
    source, program = os.path.join(tmp_path, 'size.c'), os.path.join(tmp_path, 'size')
    with open(source, 'w') as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "difflinker_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(dl_pocket_args), offsetof(dl_pocket_args, protein_x), '
                'offsetof(dl_pocket_args, cutoff), offsetof(dl_pocket_args, index)); return 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), source, '-o', program], check=True)
    sizes = [int(v) for v in subprocess.run([program], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.DLPocketArgs
    assert sizes == [ctypes.sizeof(A), A.protein_x.offset, A.cutoff.offset, A.index.offset]


def test_argument_checks_come_before_device_work():
    lib = _lib.load()
    call = lambda **kw: int(lib.dl_pocket_select(ctypes.byref(_lib.DLPocketArgs(**kw)), None))      # noqa: E731
    sizes = dict(L=4, P=1, M_total=10, cutoff=6.0, Mmax=10, capacity=4)
    assert int(lib.dl_pocket_select(None, None)) == BAD_ARG
    assert call(B=2, **sizes) == BAD_ARG                                                            # null pointers
    assert call(B=2, L=0, P=0, M_total=0, cutoff=6.0, Mmax=0, capacity=0) == BAD_ARG                # also when most may be null
    assert call(B=0, **sizes) == _lib.DL_OK                             # an empty batch is looked at no further than its sizes
    assert call(B=0, L=0, P=0, M_total=0, cutoff=0.0, Mmax=0, capacity=0) == _lib.DL_OK
    for name in ('B', 'L', 'P', 'M_total', 'Mmax', 'capacity'):
        assert call(**dict(dict(B=0, **sizes), **{name: -1})) == BAD_ARG, name
    assert call(B=0, **dict(sizes, cutoff=-1.0)) == BAD_ARG and call(B=0, **dict(sizes, cutoff=float('nan'))) == BAD_ARG


def test_cpu_tensors_raise():
    args = (torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.tensor([0, 5], dtype=torch.int32),
            torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, 3, dtype=torch.float64), torch.ones(2, 3))
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        pocket.select_pockets(*args, capacity=4)
    with pytest.raises(_lib.HipLibraryError, match='no CPU fallback'):
        pocket.select_all(*args)


# ---- the rule on the committed fixtures -------------------------------------------------------------------------------------
def by_rule(pdb, ligand, mode, by='number', cutoff=6.0):
    """The data-set atoms of one pair through ``pocket_ref`` and the host helpers: what the GPU path computes."""
    arrays = io.read_pdb_arrays(pdb)
    group = io.groups(arrays, by)
    got = pocket_ref.pair(arrays.coords, group, ligand, np.ones(len(ligand), np.float32), cutoff, len(group), len(group))
    assert got['status'] == 0
    idx = got['index'][:got['n_pocket']]
    return pocket.pocket_atoms(arrays.coords[idx], [arrays.name[j] for j in idx], [arrays.element[j] for j in idx], mode), got


@pytest.mark.parametrize('case', list(FIXTURES))
def test_rule_against_the_oracle_and_get_pocket(case):
    pdb, sdf = FIXTURES[case]
    mol = io.read_molecule(sdf)
    arrays = io.read_pdb_arrays(pdb)
    # the condition under which `d2 <= c * c` and the reference's `sqrt(d2) <= c` are one rule: no pair within a rounding of 6 A
    d = np.linalg.norm(arrays.coords[:, None, :] - mol.positions[None, :, :], axis=-1)
    gap = float(np.abs(d - 6).min())
    print(f'{case}: {len(arrays.resseq)} protein atoms, {len(mol)} ligand atoms, min |d - 6| = {gap:.3g} A')
    assert gap > 1e-9
    contact = pocket_ref.contact_mask(arrays.coords, mol.positions)
    assert np.array_equal(contact, d.min(1) <= 6), 'the two forms of the comparison give one mask'
    for mode, bb in (('full', False), ('bb', True)):
        (pos, one_hot, charges), got = by_rule(pdb, mol.positions, mode)
        assert np.array_equal(got['member'] & 1 != 0, contact) and got['n_contact_atoms'] == int(contact.sum())
        want = io.get_pocket(mol, pdb, backbone_atoms_only=bb)
        assert pos.dtype == np.float32 and np.array_equal(pos, np.asarray(want[0], dtype=np.float32)), 'same atoms, same order'
        assert np.array_equal(one_hot, want[1]) and np.array_equal(charges, want[2]) and len(charges) > 0
        oracle_pos, oracle_sym = io_oracle.pocket_of_protein(pdb, mol.positions, backbone_atoms_only=bb)
        assert np.array_equal(pos, oracle_pos) and [const.GEOM_IDX2ATOM[int(k)] for k in one_hot.argmax(1)] == oracle_sym


def test_pocket_ref_outputs_and_dead_pairs():
    x = np.array([[6, 0, 0], [7, 0, 0], [0, 6, 0], [20, 0, 0], [np.nextafter(np.float32(6), np.float32(np.inf)), 0, 0]], np.float32)
    group = np.array([0, 0, 1, 2, 3])
    lig, mask = np.zeros((3, 3)), np.array([0, 1, 0], np.float32)
    lig[0] = np.nan                                                     # a masked row: never read
    got = pocket_ref.pair(x, group, lig, mask, 6.0, 7, 2)
    assert (got['n_ligand'], got['n_contact_atoms'], got['n_groups_selected'], got['n_pocket']) == (1, 2, 2, 3)
    assert got['member'].tolist() == [3, 2, 3, 0, 0, 0, 0] and got['index'].tolist() == [0, 1] and got['status'] == pocket_ref.TRUNCATED
    assert pocket_ref.pair(x, group, lig, mask, 6.0, 7, 3)['index'].tolist() == [0, 1, 2]
    dead = {'n_contact_atoms': 0, 'n_groups_selected': 0, 'n_pocket': 0}
    for change, status in ((dict(ligand_mask=np.ones(3, np.float32)), pocket_ref.NONFINITE),
                           (dict(protein_group=np.array([0, 0, 1, 2, pocket_ref.MAX_GROUPS])), pocket_ref.TOO_MANY_GROUPS),
                           (dict(protein_group=np.array([0, -1, 1, 2, 3])), pocket_ref.TOO_MANY_GROUPS),
                           (dict(Mmax=4), pocket_ref.BAD_PROTEIN)):
        args = dict(dict(protein_x=x, protein_group=group, ligand_x=lig, ligand_mask=mask, cutoff=6.0, Mmax=7, R=2), **change)
        got = pocket_ref.pair(**args)
        assert got['status'] == status and {k: got[k] for k in dead} == dead and not got['member'].any()
        assert got['index'].tolist() == [-1, -1]
    big = pocket_ref.pair(x, group, np.zeros((257, 3)), np.ones(257, np.float32), 6.0, 7, 2)
    assert big['status'] == pocket_ref.TOO_LARGE and big['n_ligand'] == 257 and big['n_pocket'] == 0
    batch = pocket_ref.select_pockets(x, group, [0, 2, 5], [1, 0, 2], np.zeros((3, 1, 3)), np.ones((3, 1), np.float32), R=4)
    assert batch['n_pocket'].tolist() == [1, 2, 0] and batch['status'].tolist() == [0, 0, pocket_ref.BAD_PROTEIN]
    assert batch['index'].tolist() == [[0, -1, -1, -1], [0, 1, -1, -1], [-1] * 4] and batch['member'].shape == (3, 5)
    assert batch['member'].dtype == np.uint8 and all(batch[k].dtype == np.int32 for k in pocket_ref.FIELDS if k != 'member')


# ---- parsing ----------------------------------------------------------------------------------------------------------------
PDB_LINE = 'ATOM  %5d %-4s %3s %1s%4d%1s   %8.3f%8.3f%8.3f  1.00  0.00          %2s\n'


def test_read_pdb_arrays_and_groups(tmp_path):
    path = os.path.join(tmp_path, 'two_chains.pdb')
    records = [(' N  ', 'ALA', 'A', 10, ' ', 'N'), (' CA ', 'ALA', 'A', 10, ' ', 'C'), (' N  ', 'GLY', 'A', 11, ' ', 'N'),
               (' N  ', 'SER', 'A', 11, 'A', 'N'), (' N  ', 'LYS', 'B', 10, ' ', 'N'), ('ZN  ', ' ZN', 'B', -5, ' ', 'ZN')]
    with open(path, 'w') as f:
        for k, (name, res, chain, number, icode, element) in enumerate(records):
            f.write(PDB_LINE % (k + 1, name, res, chain, number, icode, 1.5 * k, 0.25, -k, element))
        f.write('END\n')
    arrays = io.read_pdb_arrays(path)
    assert arrays.coords.dtype == np.float32 and arrays.coords.shape == (6, 3) and arrays.coords[3].tolist() == [4.5, 0.25, -3.0]
    assert arrays.resseq.tolist() == [10, 10, 11, 11, 10, -5] and arrays.chain == list('AAAABB')
    assert arrays.icode == [' ', ' ', ' ', 'A', ' ', ' '] and arrays.name == ['N', 'CA', 'N', 'N', 'N', 'ZN']
    assert arrays.element == ['N', 'C', 'N', 'N', 'N', 'ZN']
    walked = io._walk_pdb(path)
    assert [a.coord for a in walked] == [[1.5 * k, 0.25, -k] for k in range(6)], '_walk_pdb is what it was'
    assert io.groups(arrays).tolist() == [0, 0, 1, 1, 0, 2], 'by number: chain B rides along, and so does the inserted residue'
    assert io.groups(arrays, by='residue').tolist() == [0, 0, 1, 2, 3, 4] and io.groups(arrays).dtype == np.int32
    with pytest.raises(ValueError):
        io.groups(arrays, by='chain')
    # the two rules on a ligand that touches residue 10 of chain A alone
    ligand = np.array([[0.0, 3.0, 0.0]])
    number, _ = by_rule(path, ligand, 'full', cutoff=3.5)
    residue, _ = by_rule(path, ligand, 'full', by='residue', cutoff=3.5)
    assert number[0][:, 0].tolist() == [0.0, 1.5, 6.0] and residue[0][:, 0].tolist() == [0.0, 1.5]
    toy = io.read_pdb_arrays(FIXTURES['toy'][0])
    assert len(toy.resseq) == 13 and toy.element.count('ZN') == 1, 'alternate locations are one atom'


# ---- assembly ---------------------------------------------------------------------------------------------------------------
def hand_item():
    """A ``fragment.examples`` dict by hand: fragments of 3 + 2 atoms, a linker of 2, anchors at 1 and 4."""
    n, nf = 7, const.GEOM_NUMBER_OF_ATOM_TYPES
    one_hot = torch.zeros(n, nf)
    one_hot[torch.arange(n), torch.tensor([0, 1, 2, 0, 0, 3, 0])] = 1
    linker = torch.tensor([0.0] * 5 + [1.0] * 2)
    return {'uuid': 4, 'name': 'abcd_ligand', 'positions': torch.arange(21, dtype=torch.float32).reshape(7, 3),
            'one_hot': one_hot, 'charges': torch.tensor([6.0, 8, 7, 6, 6, 9, 6]), 'anchors': torch.tensor([0.0, 1, 0, 0, 1, 0, 0]),
            'fragment_mask': 1 - linker, 'linker_mask': linker, 'num_atoms': n}


def test_pocket_atoms_and_examples():
    positions = np.arange(18, dtype=np.float32).reshape(6, 3) + 100
    names, elements = ['N', 'CA', 'CB', 'ZN', 'O', 'SG'], ['N', 'C', 'C', 'ZN', 'O', 'S']
    full = pocket.pocket_atoms(positions, names, elements, 'full')
    bb = pocket.pocket_atoms(positions, names, elements, 'bb')
    assert full[0].tolist() == positions[[0, 1, 2, 4, 5]].tolist() and full[2].tolist() == [7, 6, 6, 8, 16], 'zinc is no type'
    assert bb[0].tolist() == positions[[0, 1, 4]].tolist() and bb[2].tolist() == [7, 6, 8] and bb[1].shape == (3, 9)
    with pytest.raises(ValueError):
        pocket.pocket_atoms(positions, names, elements, 'sidechain')
    item = hand_item()
    (got,) = pocket.pocket_examples([item], [full])
    assert list(got) == ['uuid', 'name', 'positions', 'one_hot', 'charges', 'anchors', 'fragment_only_mask', 'pocket_mask',
                         'fragment_mask', 'linker_mask', 'num_atoms']
    assert (got['uuid'], got['name'], got['num_atoms']) == (4, 'abcd_ligand', 12)
    assert got['positions'].tolist() == item['positions'][:5].tolist() + full[0].tolist() + item['positions'][5:].tolist()
    assert got['charges'].tolist() == [6, 8, 7, 6, 6] + [7, 6, 6, 8, 16] + [9, 6]
    assert got['one_hot'].argmax(1).tolist() == [0, 1, 2, 0, 0] + [const.GEOM_ATOM2IDX[s] for s in 'NCCOS'] + [3, 0]
    assert got['anchors'].nonzero().flatten().tolist() == [1, 4], 'the anchors keep their fragment indices'
    assert got['fragment_only_mask'].tolist() == [1.0] * 5 + [0.0] * 7 and got['pocket_mask'].tolist() == [0.0] * 5 + [1.0] * 5 + [0.0] * 2
    assert got['fragment_mask'].tolist() == [1.0] * 10 + [0.0] * 2 and got['linker_mask'].tolist() == [0.0] * 10 + [1.0] * 2
    assert all(got[k].dtype == const.TORCH_FLOAT for k in list(got)[2:10])
    (empty,) = pocket.pocket_examples([item], [pocket.pocket_atoms(positions[:0], [], [], 'bb')])
    assert empty['num_atoms'] == 7 and empty['positions'].shape == (7, 3) and not empty['pocket_mask'].any()
    zinc = dict(item, one_hot=item['one_hot'][:, :const.NUMBER_OF_ATOM_TYPES])
    with pytest.raises(ValueError, match='GEOM'):
        pocket.pocket_examples([zinc], [full])
    (short,) = pocket.pocket_examples([dict(item, uuid=5)], [bb])
    for fn in (collate, collate_with_fragment_without_pocket_edges):
        batch = fn([got, short])
        assert batch['positions'].shape == (2, 12, 3) and batch['pocket_mask'].shape == (2, 12, 1) and batch['uuid'] == [4, 5]
        assert int(batch['atom_mask'].sum()) == 12 + 10 and int(batch['fragment_only_mask'].sum()) == 10


def test_prepare_command_line_has_the_pocket_options():
    from difflinker_amd import prepare
    assert prepare.POCKET_TABLE_COLUMNS == prepare.TABLE_COLUMNS + ('pocket_full_size', 'pocket_bb_size', 'molecule_size',
                                                                    'fragments_size', 'linker_size')
    assert prepare.POCKET_SKIP_REASONS == ('no_protein_file', 'empty_pocket')
    assert prepare.protein_path('dir', '3hz1_ligand_2') == os.path.join('dir', '3hz1_protein.pdb')
    with pytest.raises(SystemExit):
        prepare.main(['--sdf', 'x', '--out', 'y', '--prefix', 'z', '--proteins', 'd', '--pocket_by', 'chain'])
