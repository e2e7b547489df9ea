"""Molecule I/O of the generation scripts without RDKit / Biopython / OpenBabel.

The reference reads its inputs with ``rdkit.Chem`` (``generate.py:50-59``) and ``Bio.PDB.PDBParser``
(``generate_with_pocket.py:84-113``, ``generate_with_protein.py:85-148``) and writes ``.xyz`` files with
``src/visualizer.py:14-31``.  None of those packages exist in this image, and the sampling path only needs element
symbols and coordinates, so the few record types involved are parsed here directly:

* ``read_molecule``: first molecule of an ``.sdf`` / ``.mol`` (V2000 and V3000 atom blocks), ``.pdb`` (first model,
  first alternate location), ``.mol2`` (``@<TRIPOS>ATOM``) or ``.xyz`` file, hydrogens removed
  (``removeHs=True`` + ``Chem.RemoveAllHs``, generate.py:53-59,117);
* ``read_sdf_molecules``: EVERY record of an ``.sdf`` with its bond block and formal charges, for ``difflinker_amd.prepare``;
* ``parse_molecule``: positions / one-hot / charges with the reference's vocabularies (src/datasets.py:22-37);
* ``read_pocket`` / ``get_pocket``: the pocket dictionaries of the two pocket scripts, including their quirks
  (every model is walked, the highest-occupancy alternate location is kept, contact residues are matched by residue
  NUMBER only, the 'full' atom list keeps whatever elements the file has);
* ``read_pdb_arrays`` / ``groups``: a protein parsed ONCE into arrays and the dense residue ids of its atoms, for the batched
  pocket selection of ``difflinker_amd.pocket`` and ``difflinker_amd.prepare --proteins``;
* ``save_xyz_file`` / ``load_xyz_files`` / ``load_molecule_xyz``: byte-compatible with src/visualizer.py:14-59;
* ``save_sdf_file``: V2000 mol blocks from the bond lists of ``molecule_builder.perceive_bonds``, in place of the
  reference's ``obabel xyz -> sdf`` call (generate.py:179-180).  The bonds are the reference's own ``molecule_builder``
  rule, not OpenBabel's.  With ``hydrogens=`` it also writes the explicit hydrogens of ``molecule_builder.add_hydrogens``.
"""
import os
from collections import namedtuple
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from . import const

_TWO_LETTER = {'CL': 'Cl', 'BR': 'Br', 'NA': 'Na', 'MG': 'Mg', 'ZN': 'Zn', 'FE': 'Fe', 'CA': 'Ca', 'MN': 'Mn',
               'CU': 'Cu', 'SE': 'Se', 'SI': 'Si', 'LI': 'Li', 'CO': 'Co', 'NI': 'Ni', 'AL': 'Al'}


def _symbol(raw):
    s = raw.strip()
    if not s:
        raise ValueError('empty element symbol')
    up = s.upper()
    if up in _TWO_LETTER:
        return _TWO_LETTER[up]
    return up[0] + up[1:].lower()


@dataclass
class Molecule:
    """Heavy atoms of one molecule: what ``parse_molecule`` needs from an RDKit ``Mol``."""
    symbols: List[str]
    positions: np.ndarray                      # [n, 3] float64, file order
    name: str = ''
    props: dict = field(default_factory=dict)

    def __len__(self):
        return len(self.symbols)


def _without_hydrogens(symbols, coords, name):
    keep = [i for i, s in enumerate(symbols) if s not in ('H', 'D', 'T')]
    pos = np.asarray([coords[i] for i in keep], dtype=np.float64).reshape(len(keep), 3)
    return Molecule([symbols[i] for i in keep], pos, name)


def _read_molblock(lines):
    """Atom block of the first molecule of an SDF / MOL file (CTfile V2000 or V3000)."""
    if len(lines) < 4:
        raise ValueError('truncated mol block')
    name = lines[0].strip()
    counts = lines[3]
    symbols, coords = [], []
    if 'V3000' in counts:
        in_atoms = False
        for ln in lines[4:]:
            t = ln.strip()
            if t.startswith('M  V30 BEGIN ATOM'):
                in_atoms = True
            elif t.startswith('M  V30 END ATOM'):
                break
            elif in_atoms and t.startswith('M  V30'):
                parts = t.split()
                symbols.append(_symbol(parts[3]))
                coords.append([float(parts[4]), float(parts[5]), float(parts[6])])
    else:
        try:
            n_atoms = int(counts[0:3])
        except ValueError as e:
            raise ValueError(f'bad counts line: {counts!r}') from e
        for ln in lines[4:4 + n_atoms]:
            coords.append([float(ln[0:10]), float(ln[10:20]), float(ln[20:30])])
            symbols.append(_symbol(ln[31:34]))
        if len(symbols) != n_atoms:
            raise ValueError('truncated atom block')
    return symbols, coords, name


def _pdb_element(line):
    el = line[76:78].strip() if len(line) >= 78 else ''
    if el and el.isalpha():
        return _symbol(el)
    name = line[12:16]
    # no element column: columns 13-14 right-justify the symbol (" CA " is carbon alpha, "CA  " is calcium)
    guess = name[:2].strip() if not name[0].isdigit() and name[0] != ' ' and name[:2].upper() in _TWO_LETTER else \
        ''.join(c for c in name if c.isalpha())[:1]
    return _symbol(guess)


def _read_pdb_ligand(lines):
    symbols, coords = [], []
    for ln in lines:
        rec = ln[0:6]
        if rec.startswith('ENDMDL'):
            break
        if rec in ('ATOM  ', 'HETATM'):
            if ln[16] not in (' ', 'A'):
                continue
            symbols.append(_pdb_element(ln))
            coords.append([float(ln[30:38]), float(ln[38:46]), float(ln[46:54])])
    return symbols, coords


def _read_mol2(lines):
    symbols, coords, name = [], [], ''
    section = None
    for k, ln in enumerate(lines):
        t = ln.strip()
        if t.startswith('@<TRIPOS>'):
            if section == 'ATOM':
                break
            section = t[len('@<TRIPOS>'):]
            if section == 'MOLECULE' and k + 1 < len(lines):
                name = lines[k + 1].strip()
            continue
        if section == 'ATOM' and t:
            parts = t.split()
            coords.append([float(parts[2]), float(parts[3]), float(parts[4])])
            symbols.append(_symbol(parts[5].split('.')[0]))
    return symbols, coords, name


def read_molecule(path):
    """First molecule of ``path`` with the hydrogens removed (generate.py:50-59 + :117)."""
    if path.split('.')[-1] not in ('pdb', 'mol', 'sdf', 'mol2', 'xyz'):
        raise Exception('Unknown file extension')
    with open(path) as f:
        lines = f.read().splitlines()
    base = '.'.join(os.path.basename(path).split('.')[:-1])
    if path.endswith('.pdb'):
        symbols, coords = _read_pdb_ligand(lines)
        name = base
    elif path.endswith('.mol') or path.endswith('.sdf'):
        symbols, coords, name = _read_molblock(lines)
    elif path.endswith('.mol2'):
        symbols, coords, name = _read_mol2(lines)
    elif path.endswith('.xyz'):
        n = int(lines[0].split()[0])
        symbols = [_symbol(ln.split()[0]) for ln in lines[2:2 + n]]
        coords = [[float(v) for v in ln.split()[1:4]] for ln in lines[2:2 + n]]
        name = base
    else:
        raise Exception('Unknown file extension')
    if not symbols:
        raise ValueError(f'no atoms found in {path}')
    return _without_hydrogens(symbols, coords, name or base)


@dataclass
class BondedMolecule(Molecule):
    """A record of ``read_sdf_molecules``: heavy atoms with their bonds ``(i, j, order)`` (0-based, as the file orients them,
    order 4 aromatic), formal ``charges`` per atom, and whether the record has 3D coordinates."""
    bonds: List[tuple] = field(default_factory=list)
    charges: List[int] = field(default_factory=list)
    is_3d: bool = True


_V2000_CHARGE = {0: 0, 1: 3, 2: 2, 3: 1, 4: 0, 5: -1, 6: -2, 7: -3}     # the atom block's charge column (4: a radical)


def _read_bonded_molblock(lines):
    """One whole CTfile record (V2000 or V3000): ``(symbols, coords, charges, bonds, name, flat)``, hydrogens included."""
    if len(lines) < 4:
        raise ValueError('truncated mol block')
    name, counts = lines[0].strip(), lines[3]
    symbols, coords, charges, bonds = [], [], [], []
    if 'V3000' in counts:
        section, index, n_atoms, n_bonds = None, {}, None, None
        for ln in lines[4:]:
            t = ln.strip()
            if not t.startswith('M  V30'):
                continue
            parts = t.split()[2:]
            if parts[:1] == ['COUNTS']:
                n_atoms, n_bonds = int(parts[1]), int(parts[2])
            elif parts[:1] in (['BEGIN'], ['END']):
                section = parts[1] if parts[0] == 'BEGIN' else None
            elif section == 'ATOM':
                index[int(parts[0])] = len(symbols)
                symbols.append(_symbol(parts[1]))
                coords.append([float(parts[2]), float(parts[3]), float(parts[4])])
                charges.append(sum(int(p[4:]) for p in parts[6:] if p.startswith('CHG=')))
            elif section == 'BOND':
                bonds.append((index[int(parts[2])], index[int(parts[3])], int(parts[1])))
        if n_atoms != len(symbols) or n_bonds != len(bonds):
            raise ValueError('the V3000 counts line and the blocks disagree')
    else:
        n_atoms, n_bonds = int(counts[0:3]), int(counts[3:6])
        if len(lines) < 4 + n_atoms + n_bonds:
            raise ValueError('truncated atom or bond block')
        for ln in lines[4:4 + n_atoms]:
            coords.append([float(ln[0:10]), float(ln[10:20]), float(ln[20:30])])
            symbols.append(_symbol(ln[31:34]))
            charges.append(_V2000_CHARGE[int(ln[36:39].strip() or 0)])
        for ln in lines[4 + n_atoms:4 + n_atoms + n_bonds]:
            i, j, order = int(ln[0:3]), int(ln[3:6]), int(ln[6:9])
            if not (1 <= i <= n_atoms and 1 <= j <= n_atoms):
                raise ValueError(f'bond {i}-{j} of {n_atoms} atoms')
            bonds.append((i - 1, j - 1, order))
        listed = [ln for ln in lines[4 + n_atoms + n_bonds:] if ln.startswith('M  CHG') or ln.startswith('M  RAD')]
        if listed:                               # property lines replace the whole charge column
            charges = [0] * n_atoms
        for ln in listed:
            if ln.startswith('M  CHG'):
                parts = ln.split()
                for k in range(int(parts[2])):
                    charges[int(parts[3 + 2 * k]) - 1] = int(parts[4 + 2 * k])
    flat = lines[1][20:22] == '2D' or all(c[2] == 0.0 for c in coords)
    return symbols, coords, charges, bonds, name, flat


def read_sdf_molecules(path):
    """EVERY record of an SDF file as a ``BondedMolecule``: atom AND bond blocks of V2000 and V3000 records, formal charges
    from ``M  CHG`` lines, the atom block's charge column or ``CHG=``.  Hydrogens are removed together with their bonds and
    the bond indices renumbered.  A malformed record is skipped and counted: returns ``(molecules, n_malformed)``.
    ``read_molecule`` (first record, atoms only) stays what the generation scripts use."""
    with open(path) as f:
        lines = f.read().splitlines()
    records, start = [], 0
    for k, ln in enumerate(lines):
        if ln.strip() == '$$$$':
            records.append(lines[start:k])
            start = k + 1
    if any(ln.strip() for ln in lines[start:]):
        records.append(lines[start:])            # a last record without its terminator
    molecules, malformed = [], 0
    for number, record in enumerate(records):
        try:
            symbols, coords, charges, bonds, name, flat = _read_bonded_molblock(record)
            if not symbols:
                raise ValueError('no atoms')
        except (ValueError, IndexError, KeyError):
            malformed += 1
            continue
        keep = [i for i, s in enumerate(symbols) if s not in ('H', 'D', 'T')]
        new = {old: k for k, old in enumerate(keep)}
        pos = np.asarray([coords[i] for i in keep], dtype=np.float64).reshape(len(keep), 3)
        molecules.append(BondedMolecule([symbols[i] for i in keep], pos, name or f'record_{number}',
                                        bonds=[(new[i], new[j], order) for i, j, order in bonds if i in new and j in new],
                                        charges=[charges[i] for i in keep], is_3d=not flat))
    return molecules, malformed


def get_one_hot(atom, atoms_dict):
    one_hot = np.zeros(len(atoms_dict))
    one_hot[atoms_dict[atom]] = 1
    return one_hot


def parse_molecule(mol, is_geom):
    """``(positions [n,3], one_hot [n,types], charges [n])`` — src/datasets.py:28-37."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    charges_dict = const.GEOM_CHARGES if is_geom else const.CHARGES
    one_hot, charges = [], []
    for s in mol.symbols:
        if s not in atom2idx:
            raise KeyError(f'element {s!r} is outside the model vocabulary {sorted(atom2idx)}')
        one_hot.append(get_one_hot(s, atom2idx))
        charges.append(charges_dict[s])
    return np.asarray(mol.positions, dtype=np.float64), np.array(one_hot), np.array(charges)


# ---------------------------------------------------------------------------------------------------
# protein pockets
@dataclass
class _PdbAtom:
    name: str
    element: str
    coord: List[float]
    resseq: int
    occupancy: float
    chain: str = ' '
    icode: str = ' '


def _walk_pdb(path):
    """Atoms in Bio.PDB iteration order (models, chains, residues, atoms as they appear); for an atom with alternate
    locations one entry at the position of its first record, holding the location with the highest occupancy."""
    atoms, index = [], {}
    model = 0
    with open(path) as f:
        for ln in f:
            rec = ln[0:6]
            if rec.startswith('ENDMDL'):
                model += 1
                continue
            if rec not in ('ATOM  ', 'HETATM'):
                continue
            name = ln[12:16].strip()
            try:
                occ = float(ln[54:60])
            except ValueError:
                occ = 1.0
            atom = _PdbAtom(name, _pdb_element(ln).upper(), [float(ln[30:38]), float(ln[38:46]), float(ln[46:54])],
                            int(ln[22:26]), occ, ln[21], ln[26])
            key = (model, ln[21], ln[22:27], ln[17:20], name)      # chain, resseq + icode, resname, atom
            if ln[16] != ' ' and key in index:
                if occ > atoms[index[key]].occupancy:
                    atoms[index[key]] = atom
                continue
            if ln[16] != ' ':
                index[key] = len(atoms)
            atoms.append(atom)
    return atoms


def read_pocket(path):
    """Pocket dictionary of generate_with_pocket.py:84-113 (the file already holds the pocket residues only)."""
    full_c, full_t, bb_c, bb_t = [], [], [], []
    for a in _walk_pdb(path):
        full_c.append(a.coord)
        full_t.append(a.element)
        if a.name == 'H':
            continue
        if a.name in {'N', 'CA', 'C', 'O'}:
            bb_c.append(a.coord)
            bb_t.append(a.element)
    return {'full_coord': np.array(full_c), 'full_types': np.array(full_t),
            'bb_coord': np.array(bb_c), 'bb_types': np.array(bb_t)}


def get_pocket(mol, pdb_path, backbone_atoms_only=False):
    """Residues with an atom within 6 A of the ligand (generate_with_protein.py:85-148).  Contact residues are matched
    by residue NUMBER alone, as the reference does: equal numbers in other chains are included."""
    atoms = _walk_pdb(pdb_path)
    residue_ids = np.array([a.resseq for a in atoms])
    atom_coords = np.array([a.coord for a in atoms], dtype=np.float32)       # Bio.PDB stores float32 coordinates
    mol_coords = np.asarray(mol.positions if isinstance(mol, Molecule) else mol, dtype=np.float64)
    distances = np.linalg.norm(atom_coords[:, None, :] - mol_coords[None, :, :], axis=-1)
    contact = set(np.unique(residue_ids[np.where(distances.min(1) <= 6)[0]]).tolist())
    pos, one_hot, charges = [], [], []
    for a in atoms:
        if a.resseq not in contact:
            continue
        if backbone_atoms_only and a.name not in {'N', 'CA', 'C', 'O'}:
            continue
        sym = _symbol(a.element)
        if a.element not in const.GEOM_ATOM2IDX and sym not in const.GEOM_ATOM2IDX:
            continue
        key = a.element if a.element in const.GEOM_ATOM2IDX else sym
        pos.append(a.coord)
        one_hot.append(get_one_hot(key, const.GEOM_ATOM2IDX))
        charges.append(const.GEOM_CHARGES[key])
    return np.array(pos), np.array(one_hot), np.array(charges)


PdbArrays = namedtuple('PdbArrays', 'coords resseq chain icode name element')


def read_pdb_arrays(path):
    """One PDB file, parsed once, per atom in ``_walk_pdb`` order: ``coords [M,3]`` fp32 (Bio.PDB keeps float32 coordinates, and
    ``get_pocket`` measures from them), ``resseq [M]`` residue numbers (int64), and the lists ``chain``, ``icode`` (insertion
    code, ``' '`` for none), ``name`` (atom name) and ``element`` (upper case, as ``_walk_pdb`` keeps it).  What
    ``pocket.select_pockets`` and ``pocket.pocket_atoms`` need of a protein; ``get_pocket`` parses the file again for every
    ligand."""
    atoms = _walk_pdb(path)
    return PdbArrays(np.array([a.coord for a in atoms], dtype=np.float32).reshape(len(atoms), 3),
                     np.array([a.resseq for a in atoms], dtype=np.int64), [a.chain for a in atoms], [a.icode for a in atoms],
                     [a.name for a in atoms], [a.element for a in atoms])


def groups(arrays, by='number'):
    """Dense group ids ``[M]`` int32 of a ``PdbArrays``, numbered ``0 .. G - 1`` in order of first appearance: the residues
    ``dl_pocket_select`` selects as a whole.  ``by='number'`` groups by the residue NUMBER alone, the reference's rule
    (``get_pocket``): equal numbers in other chains, and with other insertion codes, are one group.  ``by='residue'`` groups by
    ``(chain, number, insertion code)``."""
    if by not in ('number', 'residue'):
        raise ValueError(f"groups by {by!r}: 'number' or 'residue'")
    keys = arrays.resseq.tolist() if by == 'number' else list(zip(arrays.chain, arrays.resseq.tolist(), arrays.icode))
    ids = {}
    return np.array([ids.setdefault(key, len(ids)) for key in keys], dtype=np.int32)


def get_protein_atoms(pdb_path, is_geom=True):
    """``(positions [M,3], types [M] int32)`` of ALL atoms of a PDB file whose element is in the vocabulary, in the file's own
    frame and in ``_walk_pdb`` order: the shared target list of ``metrics.analyze_clashes``.  Unlike ``get_pocket`` nothing
    is cut to the 6 A neighbourhood - a generated linker can run into residues the model never saw - and other elements
    (hydrogens, metals) are left out as ``get_pocket`` leaves them out."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    pos, types = [], []
    for a in _walk_pdb(pdb_path):
        key = a.element if a.element in atom2idx else _symbol(a.element)
        if key in atom2idx:
            pos.append(a.coord)
            types.append(atom2idx[key])
    return np.array(pos, dtype=np.float64).reshape(-1, 3), np.array(types, dtype=np.int32)


def pocket_arrays(pocket_data, backbone_atoms_only):
    """One-hot / charges of a ``read_pocket`` dictionary (generate_with_pocket.py:200-209); unknown elements raise like
    the reference's dictionary lookup does."""
    mode = 'bb' if backbone_atoms_only else 'full'
    one_hot, charges = [], []
    for t in pocket_data[f'{mode}_types']:
        key = t if t in const.GEOM_ATOM2IDX else _symbol(t)
        if key not in const.GEOM_ATOM2IDX:
            raise KeyError(f'pocket element {t!r} is outside the model vocabulary {sorted(const.GEOM_ATOM2IDX)}')
        one_hot.append(get_one_hot(key, const.GEOM_ATOM2IDX))
        charges.append(const.GEOM_CHARGES[key])
    return pocket_data[f'{mode}_coord'], np.array(one_hot), np.array(charges)


# ---------------------------------------------------------------------------------------------------
# xyz output
def save_xyz_file(path, one_hot, positions, node_mask, names, is_geom, suffix=''):
    """One ``<name>_<suffix>.xyz`` per molecule, masked atoms only, ``%.9f`` coordinates (src/visualizer.py:14-31)."""
    idx2atom = const.GEOM_IDX2ATOM if is_geom else const.IDX2ATOM
    one_hot, positions, node_mask = one_hot.detach().cpu(), positions.detach().cpu(), node_mask.detach().cpu()
    for batch_i in range(one_hot.size(0)):
        mask = node_mask[batch_i].reshape(-1)
        atom_idx = torch.where(mask)[0]
        atoms = torch.argmax(one_hot[batch_i], dim=1)
        with open(os.path.join(path, f'{names[batch_i]}_{suffix}.xyz'), 'w') as f:
            f.write('%d\n\n' % int(mask.sum()))
            for atom_i in atom_idx:
                f.write('%s %.9f %.9f %.9f\n' % (idx2atom[atoms[atom_i].item()], positions[batch_i, atom_i, 0],
                                                 positions[batch_i, atom_i, 1], positions[batch_i, atom_i, 2]))


HYDROGENS_OVERFLOW = 32             # DL_HYDRO_OVERFLOW of include/difflinker_hip.h: the list of hydrogens was cut at its capacity


def save_sdf_file(path, one_hot, positions, node_mask, bonds, n_bonds, names, is_geom, suffix='', hydrogens=None):
    """One ``<name>_<suffix>.sdf`` per molecule (the naming of ``save_xyz_file``): a CTfile V2000 mol block of the masked
    atoms, in the order ``save_xyz_file`` writes them, with ``%10.4f`` coordinates, and the first ``n_bonds[b]`` rows
    ``(i, j, order)`` of ``bonds[b]`` (0-based atom numbers as ``perceive_bonds`` gives them) as 1-based bond lines
    ``i j order`` - the orientation of the reference's ``mol.AddBond(i, j)``, ``j < i``.  V2000 counts are three digits wide:
    more than 999 atoms or bonds raise ``ValueError``, and so does a bond list cut short by its capacity.
    ``hydrogens`` (a ``molecule_builder.Hydrogens`` for the same batch; ``None`` writes heavy atoms alone) adds its first
    ``n_h[b]`` hydrogens after the heavy atoms (symbol ``H``, the same ``%10.4f``) and, after the heavy bonds, one bond line
    ``n + t + 1, parent + 1, 1`` for hydrogen ``t`` of a molecule of ``n`` heavy atoms; the counts line and the 999 limit
    then hold the totals, and a hydrogen list cut short by its capacity (``DL_HYDRO_OVERFLOW``) raises ``ValueError``."""
    idx2atom = const.GEOM_IDX2ATOM if is_geom else const.IDX2ATOM
    one_hot, positions, node_mask = one_hot.detach().cpu(), positions.detach().cpu(), node_mask.detach().cpu()
    bonds, n_bonds = torch.as_tensor(bonds).detach().cpu(), torch.as_tensor(n_bonds).detach().cpu()
    if hydrogens is not None:
        n_h, h_parent, h_x, h_status = (torch.as_tensor(t).detach().cpu() for t in
                                        (hydrogens.n_h, hydrogens.parent, hydrogens.x, hydrogens.status))
    for batch_i in range(one_hot.size(0)):
        atom_idx = torch.where(node_mask[batch_i].reshape(-1))[0]
        atoms = torch.argmax(one_hot[batch_i], dim=1)
        n_atoms, nb = len(atom_idx), int(n_bonds[batch_i])
        if nb > bonds.shape[1]:
            raise ValueError(f'molecule {batch_i} has {nb} bonds, its list holds {bonds.shape[1]}')
        nh = 0
        if hydrogens is not None:
            nh = int(n_h[batch_i])
            if int(h_status[batch_i]) & HYDROGENS_OVERFLOW or nh > h_parent.shape[1]:
                raise ValueError(f'molecule {batch_i} has {nh} hydrogens, their list holds {h_parent.shape[1]}')
        if n_atoms + nh > 999 or nb + nh > 999:
            raise ValueError(f'molecule {batch_i} has {n_atoms + nh} atoms and {nb + nh} bonds: a V2000 mol block holds 999 '
                             'of each')
        rows = bonds[batch_i, :nb].tolist()
        if any(not (0 <= j < i < n_atoms and 1 <= order <= 3) for i, j, order in rows):
            raise ValueError(f'molecule {batch_i}: a bond is not (i, j, order) with j < i < {n_atoms} and order 1..3')
        parents = h_parent[batch_i, :nh].tolist() if nh else []
        if any(not 0 <= parent < n_atoms for parent in parents):
            raise ValueError(f'molecule {batch_i}: a hydrogen\'s parent is not an atom number below {n_atoms}')
        name = f'{names[batch_i]}_{suffix}'
        with open(os.path.join(path, f'{name}.sdf'), 'w') as f:
            f.write(f'{os.path.basename(name)}\n  difflinker_amd          3D\n\n')
            f.write('%3d%3d  0  0  0  0  0  0  0  0999 V2000\n' % (n_atoms + nh, nb + nh))
            for atom_i in atom_idx:
                f.write('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0\n' % (
                    positions[batch_i, atom_i, 0], positions[batch_i, atom_i, 1], positions[batch_i, atom_i, 2],
                    idx2atom[atoms[atom_i].item()]))
            for t in range(nh):
                f.write('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0\n' % (
                    h_x[batch_i, t, 0], h_x[batch_i, t, 1], h_x[batch_i, t, 2], 'H'))
            for i, j, order in rows:
                f.write('%3d%3d%3d  0  0  0  0\n' % (i + 1, j + 1, order))
            for t, parent in enumerate(parents):
                f.write('%3d%3d%3d  0  0  0  0\n' % (n_atoms + t + 1, parent + 1, 1))
            f.write('M  END\n$$$$\n')


def load_xyz_files(path, suffix=''):
    """Paths of the ``*_<suffix>.xyz`` files of a directory, latest frame index first (src/visualizer.py:34-40)."""
    files = [fname for fname in os.listdir(path) if fname.endswith(f'_{suffix}.xyz')]
    files = sorted(files, key=lambda f: -int(f.replace(f'_{suffix}.xyz', '').split('_')[-1]))
    return [os.path.join(path, fname) for fname in files]


def load_molecule_xyz(file, is_geom):
    """``(positions [n,3], one_hot [n,types], charges [n,1] zeros)`` of an ``.xyz`` written by ``save_xyz_file``
    (src/visualizer.py:43-59)."""
    atom2idx = const.GEOM_ATOM2IDX if is_geom else const.ATOM2IDX
    with open(file, encoding='utf8') as f:
        n_atoms = int(f.readline())
        one_hot = torch.zeros(n_atoms, len(atom2idx))
        charges = torch.zeros(n_atoms, 1)
        positions = torch.zeros(n_atoms, 3)
        f.readline()
        atoms = f.readlines()
        for i in range(n_atoms):
            parts = atoms[i].split(' ')
            one_hot[i, atom2idx[parts[0]]] = 1
            positions[i, :] = torch.Tensor([float(e) for e in parts[1:]])
    return positions, one_hot, charges
