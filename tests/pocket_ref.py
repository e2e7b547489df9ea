"""The pocket rule of ``dl_pocket_select`` (``csrc/pocket.hip``) restated in numpy fp64, in the kernel's operation order, with every
output of the kernel: counts, ``member``, ``index``, status and the dead outputs of a pair that cannot be answered.  numpy does
not contract a multiply and an add, so ``((dx*dx) + (dy*dy)) + (dz*dz)`` on fp64 arrays is the five roundings of the kernel."""
import numpy as np

MAX_LIGAND, MAX_GROUPS = 256, 32768
NONFINITE, TOO_LARGE, TOO_MANY_GROUPS, BAD_PROTEIN, TRUNCATED = 1, 2, 4, 8, 32
FIELDS = ('n_ligand', 'n_contact_atoms', 'n_groups_selected', 'n_pocket', 'status', 'member', 'index')


def contact_mask(protein_x32, ligand_x64, cutoff=6.0):
    """``[M]`` bool: protein atoms (fp32 coordinates, widened) with ``d2 <= cutoff * cutoff`` to some ligand atom (fp64)."""
    xp = np.asarray(protein_x32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    xl = np.asarray(ligand_x64, dtype=np.float64).reshape(-1, 3)
    c2 = np.float64(cutoff) * np.float64(cutoff)
    contact = np.zeros(len(xp), dtype=bool)
    for i in range(len(xl)):
        dx, dy, dz = xp[:, 0] - xl[i, 0], xp[:, 1] - xl[i, 1], xp[:, 2] - xl[i, 2]
        contact |= ((dx * dx) + (dy * dy)) + (dz * dz) <= c2
    return contact


def pair(protein_x, protein_group, ligand_x, ligand_mask, cutoff, Mmax, R, bad_protein=False):
    """One pair: the atoms of ITS protein, all ligand rows with their mask.  Returns a dict of ``FIELDS``."""
    out = {'n_ligand': 0, 'n_contact_atoms': 0, 'n_groups_selected': 0, 'n_pocket': 0, 'status': 0,
           'member': np.zeros(Mmax, np.uint8), 'index': np.full(R, -1, np.int32)}
    real = np.asarray(ligand_mask, dtype=np.float32) != 0
    out['n_ligand'] = int(real.sum())
    if out['n_ligand'] > MAX_LIGAND:
        out['status'] = TOO_LARGE
        return out
    M = len(protein_group)
    if bad_protein or M > Mmax:
        out['status'] = BAD_PROTEIN
        return out
    xl = np.asarray(ligand_x, dtype=np.float64).reshape(-1, 3)[real]
    xp = np.asarray(protein_x, dtype=np.float32).reshape(-1, 3)
    group = np.asarray(protein_group, dtype=np.int64)
    if not np.isfinite(xl).all() or not np.isfinite(xp).all():
        out['status'] |= NONFINITE
    if ((group < 0) | (group >= MAX_GROUPS)).any():
        out['status'] |= TOO_MANY_GROUPS
    if out['status']:
        return out
    contact = contact_mask(xp, xl, cutoff)
    selected = np.unique(group[contact])
    pocket = np.isin(group, selected)
    out['n_contact_atoms'], out['n_groups_selected'], out['n_pocket'] = int(contact.sum()), len(selected), int(pocket.sum())
    out['member'][:M] = contact.astype(np.uint8) | (pocket.astype(np.uint8) << 1)
    where = np.nonzero(pocket)[0][:R]
    out['index'][:len(where)] = where
    if out['n_pocket'] > R:
        out['status'] |= TRUNCATED
    return out


def select_pockets(protein_x, protein_group, protein_offset, pair_protein, ligand_x, ligand_mask, cutoff=6.0, Mmax=None, R=0):
    """The whole launch: arrays as ``dl_pocket_args`` takes them.  Returns a dict of ``FIELDS``, every array with the kernel's
    dtype and shape."""
    protein_x = np.asarray(protein_x, dtype=np.float32).reshape(-1, 3)
    offset = np.asarray(protein_offset, dtype=np.int64)
    P, M_total = len(offset) - 1, len(protein_x)
    Mmax = M_total if Mmax is None else Mmax
    B = len(pair_protein)
    L = np.shape(ligand_mask)[-1]
    ligand_x = np.asarray(ligand_x, dtype=np.float64).reshape(B, L, 3)
    ligand_mask = np.asarray(ligand_mask, dtype=np.float32).reshape(B, L)
    rows = []
    for b in range(B):
        p = int(pair_protein[b])
        ok = 0 <= p < P and 0 <= offset[p] <= offset[p + 1] <= M_total
        lo, hi = (offset[p], offset[p + 1]) if ok else (0, 0)
        rows.append(pair(protein_x[lo:hi], np.asarray(protein_group)[lo:hi], ligand_x[b], ligand_mask[b], cutoff, Mmax, R,
                         bad_protein=not ok))
    out = {k: np.array([r[k] for r in rows], dtype=np.int32).reshape(B) for k in FIELDS[:5]}
    out['member'] = np.array([r['member'] for r in rows], dtype=np.uint8).reshape(B, Mmax)
    out['index'] = np.array([r['index'] for r in rows], dtype=np.int32).reshape(B, R)
    return out
