"""Constants of the sampling boundary (reference ``src/const.py:6-61``; values restated) and of bond perception: the
typical bond lengths behind ``get_bond_order`` (``src/const.py:64-139,175``) as matrices over this project's atom indices,
from which ``bond_threshold_table`` builds the table of upper bounds the HIP kernel reads.  The RDKit enumerations of the
reference (``BOND_DICT``, ``BOND2IDX``) have no counterpart: bond orders are the integers 1, 2, 3."""
import math

import torch

TORCH_FLOAT = torch.float32
TORCH_INT = torch.int8          # masks are int8 end to end (const.py:7) — see datasets.collate

# one-hot atom vocabularies (const.py:14,29)
ATOM2IDX = {'C': 0, 'O': 1, 'N': 2, 'F': 3, 'S': 4, 'Cl': 5, 'Br': 6, 'I': 7}
IDX2ATOM = {v: k for k, v in ATOM2IDX.items()}
CHARGES = {'C': 6, 'O': 8, 'N': 7, 'F': 9, 'S': 16, 'Cl': 17, 'Br': 35, 'I': 53}
NUMBER_OF_ATOM_TYPES = len(ATOM2IDX)

GEOM_ATOM2IDX = dict(ATOM2IDX, P=8)
GEOM_IDX2ATOM = {v: k for k, v in GEOM_ATOM2IDX.items()}
GEOM_CHARGES = dict(CHARGES, P=15)
GEOM_NUMBER_OF_ATOM_TYPES = len(GEOM_ATOM2IDX)

# batch-key sets (const.py:39-47)
DATA_LIST_ATTRS = {'uuid', 'name', 'fragments_smi', 'linker_smi', 'num_atoms'}
DATA_ATTRS_TO_PAD = {
    'positions', 'one_hot', 'charges', 'anchors', 'fragment_mask', 'linker_mask', 'pocket_mask', 'fragment_only_mask'
}
DATA_ATTRS_TO_ADD_LAST_DIM = {
    'charges', 'anchors', 'fragment_mask', 'linker_mask', 'pocket_mask', 'fragment_only_mask'
}

# linker-size histogram of the ZINC train split (const.py:50-61)
# (insertion order as in the reference: DistributionNodes enumerates the dict, so the order decides which size a
# seeded Categorical draw maps to)
LINKER_SIZE_DIST = {4: 85540, 3: 113928, 6: 70946, 7: 30408, 5: 77671, 9: 5177, 10: 1214, 8: 12712, 11: 158, 12: 7}

# class tables of the size predictor (const.py:181-206)
ZINC_TRAIN_LINKER_ID2SIZE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
ZINC_TRAIN_LINKER_SIZE2ID = {size: idx for idx, size in enumerate(ZINC_TRAIN_LINKER_ID2SIZE)}
GEOM_TRAIN_LINKER_ID2SIZE = list(range(3, 33)) + [36, 38, 41]
GEOM_TRAIN_LINKER_SIZE2ID = {size: idx for idx, size in enumerate(GEOM_TRAIN_LINKER_ID2SIZE)}

# typical bond lengths in pm (const.py:64-139) by GEOM atom index (C O N F S Cl Br I P; the ZINC vocabulary is the leading
# 8 x 8 block), 0 = the reference has no entry.  The reference looks a pair up with the atom of the LOWER index first, so
# entry [a][b] = [b][a] is what that lookup finds; Cl-I, Br-I and I-P have no single-bond length and never bond.
BOND_LENGTHS = (
    (   # single
        (154, 143, 147, 135, 182, 177, 194, 214, 184),  # C
        (143, 148, 140, 142, 151, 164, 172, 194, 163),  # O
        (147, 140, 145, 136, 168, 175, 214, 222, 177),  # N
        (135, 142, 136, 142, 158, 166, 178, 187, 156),  # F
        (182, 151, 168, 158, 204, 207, 225, 234, 210),  # S
        (177, 164, 175, 166, 207, 199, 214,   0, 203),  # Cl
        (194, 172, 214, 178, 225, 214, 228,   0, 222),  # Br
        (214, 194, 222, 187, 234,   0,   0, 266,   0),  # I
        (184, 163, 177, 156, 210, 203, 222,   0, 221),  # P
    ),
    (   # double
        (134, 120, 129,   0, 160,   0,   0,   0,   0),  # C
        (120, 121, 121,   0,   0,   0,   0,   0, 150),  # O
        (129, 121, 125,   0,   0,   0,   0,   0,   0),  # N
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # F
        (160,   0,   0,   0,   0,   0,   0,   0, 186),  # S
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # Cl
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # Br
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # I
        (  0, 150,   0,   0, 186,   0,   0,   0,   0),  # P
    ),
    (   # triple
        (120, 113, 116,   0,   0,   0,   0,   0,   0),  # C
        (113,   0,   0,   0,   0,   0,   0,   0,   0),  # O
        (116,   0, 110,   0,   0,   0,   0,   0,   0),  # N
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # F
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # S
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # Cl
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # Br
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # I
        (  0,   0,   0,   0,   0,   0,   0,   0,   0),  # P
    ),
)
MARGINS_EDM = (10, 5, 2)            # pm added to the single / double / triple length (const.py:175)
NO_BOND_THRESHOLD = -1.0            # "no such order": distances are >= 0, so `d < -1` never holds


def bond_threshold_table(is_geom, margins=MARGINS_EDM):
    """``[n_types][n_types][3]`` fp32 upper bounds in pm: a pair at ``d`` pm has order >= k + 1 when ``d < table[a][b][k]``
    and every lower order holds too (the kernel and ``get_bond_order`` nest the comparisons)."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    table = torch.full((n, n, 3), NO_BOND_THRESHOLD, dtype=TORCH_FLOAT)
    for k in range(3):
        for a in range(n):
            for b in range(n):
                if BOND_LENGTHS[k][a][b]:
                    table[a, b, k] = BOND_LENGTHS[k][a][b] + margins[k]
    return table

# most bonds an atom may carry (const.py:156-171, ALLOWED_BONDS) by this project's atom indices; a list entry such as
# P: [3, 5] keeps its alternatives.  Hydrogens are implicit in these data sets, so the valence rule of ``metrics`` is
# "at most", not "exactly"
ALLOWED_BONDS = {'C': 4, 'O': 2, 'N': 3, 'F': 1, 'S': 4, 'Cl': 1, 'Br': 1, 'I': 1, 'P': [3, 5]}


def max_valence_table(is_geom):
    """int32 ``[n_types]``: the largest allowed bond count of every element of the vocabulary, in index order."""
    idx2atom = GEOM_IDX2ATOM if is_geom else IDX2ATOM
    limits = [ALLOWED_BONDS[idx2atom[k]] for k in range(len(idx2atom))]
    return torch.tensor([max(v) if isinstance(v, (list, tuple)) else v for v in limits], dtype=torch.int32)


def ring_class_table(is_geom):
    """int32 ``[n_types]``: the class ``dl_aromatic_rings`` gives every element of the vocabulary, in index order: 1 for
    carbon, 2 for nitrogen, 3 for oxygen and sulphur, 0 for everything else (halogens and phosphorus are never ring atoms of
    an aromatic ring here)."""
    idx2atom = GEOM_IDX2ATOM if is_geom else IDX2ATOM
    classes = {'C': 1, 'N': 2, 'O': 3, 'S': 3}
    return torch.tensor([classes.get(idx2atom[k], 0) for k in range(len(idx2atom))], dtype=torch.int32)


# what ``dl_pharmacophore_features`` needs to know of an element: its class (1 C, 2 N, 3 O, 4 S, 5 P, 6 F, 7 Cl / Br / I) and
# the number of bonds it carries when neutral, from which the open valences (implicit hydrogens) are counted
FEATURE_CLASSES = {'C': 1, 'N': 2, 'O': 3, 'S': 4, 'P': 5, 'F': 6, 'Cl': 7, 'Br': 7, 'I': 7}
DEFAULT_VALENCE = {'C': 4, 'N': 3, 'O': 2, 'F': 1, 'S': 2, 'Cl': 1, 'Br': 1, 'I': 1, 'P': 3}


def feature_class_table(is_geom):
    """int32 ``[n_types]``: the class ``dl_pharmacophore_features`` gives every element of the vocabulary, in index order."""
    idx2atom = GEOM_IDX2ATOM if is_geom else IDX2ATOM
    return torch.tensor([FEATURE_CLASSES.get(idx2atom[k], 0) for k in range(len(idx2atom))], dtype=torch.int32)


def default_valence_table(is_geom):
    """int32 ``[n_types]``: the default valence of every element of the vocabulary, in index order (``DEFAULT_VALENCE``)."""
    idx2atom = GEOM_IDX2ATOM if is_geom else IDX2ATOM
    return torch.tensor([DEFAULT_VALENCE[idx2atom[k]] for k in range(len(idx2atom))], dtype=torch.int32)


def atomic_number_table(is_geom):
    """int32 ``[n_types]``: the atomic number of every element of the vocabulary, in index order (``CHARGES``)."""
    idx2atom, numbers = (GEOM_IDX2ATOM, GEOM_CHARGES) if is_geom else (IDX2ATOM, CHARGES)
    return torch.tensor([numbers[idx2atom[k]] for k in range(len(idx2atom))], dtype=torch.int32)


# X-H bond lengths in Angstrom at which ``molecule_builder.add_hydrogens`` places a hydrogen on an atom of every element
# (the usual textbook single-bond lengths to hydrogen; the rule itself is stated in ``include/difflinker_hip.h``)
XH_LENGTH = {'C': 1.09, 'N': 1.01, 'O': 0.96, 'F': 0.92, 'S': 1.34, 'Cl': 1.27, 'Br': 1.41, 'I': 1.61, 'P': 1.42}


def xh_length_table(is_geom):
    """fp64 ``[n_types]``: the X-H bond length of every element of the vocabulary, in index order (``XH_LENGTH``)."""
    idx2atom = GEOM_IDX2ATOM if is_geom else IDX2ATOM
    return torch.tensor([XH_LENGTH[idx2atom[k]] for k in range(len(idx2atom))], dtype=torch.float64)


# Bondi's van der Waals radii in Angstrom (J. Phys. Chem. 68, 441 (1964)) by GEOM atom index (C O N F S Cl Br I P; the ZINC
# vocabulary is the leading 8): what the clash rule of ``metrics.analyze_clashes`` is built from
VDW_RADII = (1.70, 1.52, 1.55, 1.47, 1.80, 1.75, 1.85, 1.98, 1.80)


def clash_threshold_table(is_geom, scale=0.75, tolerance=0.0):
    """``[n_types][n_types]`` fp32 distances in Angstrom: a query atom of type ``a`` and a target atom of type ``b`` clash
    when they are closer than ``table[a][b] = scale * (r[a] + r[b]) - tolerance`` (``VDW_RADII``; computed in fp64, rounded to
    fp32 once) and that entry is positive.  Hydrogens are implicit in these data sets, so the plain sum (``scale = 1``) flags
    ordinary contacts between heavy atoms; the default 0.75 is the usual heavy-atom convention."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    table = torch.zeros((n, n), dtype=torch.float64)
    for a in range(n):
        for b in range(n):
            table[a, b] = float(scale) * (VDW_RADII[a] + VDW_RADII[b]) - float(tolerance)
    return table.to(TORCH_FLOAT)


# ---- the tables of ``metrics.analyze_pose_checks`` (``dl_pose_checks``): every threshold is formed here, once, in fp64 as
# plain Python floats with one rounding per operation, so that the kernel only compares
ANGLE_CLASSES = ('linear', 'trigonal', 'tetrahedral')     # the order of ``angle_cos_table``'s rows
ANGLE_IDEALS = (180.0, 120.0, 109.47122063449069)         # degrees; the last is acos(-1/3)


def length_bounds_table(is_geom, lo=0.75, hi=1.25):
    """fp64 ``[n_types][n_types][3][2]`` SQUARED bond-length bounds in Angstrom^2: for a pair of types ``(s, t)`` of order
    ``k + 1`` with the typical length ``L0 = BOND_LENGTHS[k][s][t] / 100.0``, entry ``[s][t][k]`` is ``((lo * L0) ** 2,
    (hi * L0) ** 2)``; ``(0, 0)`` where the reference has no length for that order.  0.75 and 1.25 are PoseBusters' factors."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    rows = [[[[0.0, 0.0] for _ in range(3)] for _ in range(n)] for _ in range(n)]
    for k in range(3):
        for a in range(n):
            for b in range(n):
                if BOND_LENGTHS[k][a][b]:
                    length = BOND_LENGTHS[k][a][b] / 100.0
                    low, high = float(lo) * length, float(hi) * length
                    rows[a][b][k] = [low * low, high * high]
    return torch.tensor(rows, dtype=torch.float64)


def angle_cos_table(tolerance_deg=25.0):
    """fp64 ``[3][2]``: the lowest and the highest cosine a bond angle of the classes ``ANGLE_CLASSES`` may have,
    ``cos(theta0 + tol)`` and ``cos(theta0 - tol)`` for ``ANGLE_IDEALS``; -2 where ``theta0 + tol`` reaches 180 degrees and 2
    where ``theta0 - tol`` reaches 0, which no cosine is below or above."""
    tol = float(tolerance_deg)
    return torch.tensor([[math.cos(math.radians(t + tol)) if t + tol < 180.0 else -2.0,
                          math.cos(math.radians(t - tol)) if t - tol > 0.0 else 2.0] for t in ANGLE_IDEALS], dtype=torch.float64)


def internal_clash_table(is_geom, scale=0.75):
    """fp64 ``[n_types][n_types]`` SQUARED distances in Angstrom^2: two atoms of one molecule four or more bonds apart clash
    when ``d2 < (scale * (VDW_RADII[a] + VDW_RADII[b])) ** 2``.  0.75 is the heavy-atom convention of
    ``clash_threshold_table``."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    reach = [[float(scale) * (VDW_RADII[a] + VDW_RADII[b]) for b in range(n)] for a in range(n)]
    return torch.tensor([[v * v for v in row] for row in reach], dtype=torch.float64)


# ---- the tables and constants of ``molecule_builder.relax`` (``dl_relax_molecules``): formed here in fp64 as plain Python
# floats, one rounding per operation.  The force constants are design parameters of this project's own restraint energy, in
# units of its own (NOT UFF or MMFF parameters); the FIRE constants are those of Bitzek et al., PRL 97, 170201 (2006)
RELAX_DEFAULTS = dict(k_bond=100.0, k_angle=50.0, k_rep=10.0, k_wall=10.0, k_pos=1.0, dt0=0.03, dt_max=0.1, alpha0=0.1, n_min=5,
                      f_inc=1.1, f_dec=0.5, f_alpha=0.99, max_step=0.1, f_tol=1e-3)
RELAX_STEPS = 200
RELAX_REACH_SCALE = 0.8             # just outside the 0.75 at which ``internal_clash_table`` flags a clash
IDEAL_COS = (-1.0, -0.5, -1.0 / 3.0)                      # the cosines of ``ANGLE_IDEALS``, exact
# ring bond lengths in Angstrom: benzene, pyridine, furan, thiophene and pyrazole (Allen et al., J. Chem. Soc., Perkin Trans. 2
# 1987, S1-S19, the values every textbook table rounds to)
AROMATIC_LENGTHS = {('C', 'C'): 1.39, ('C', 'N'): 1.34, ('C', 'O'): 1.36, ('C', 'S'): 1.71, ('N', 'N'): 1.35}


def length0_table(is_geom):
    """fp64 ``[n_types][n_types][3]``: the typical length ``BOND_LENGTHS[k][s][t] / 100.0`` of every order in Angstrom; 0 where
    the reference has none (no bond term)."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    return torch.tensor([[[BOND_LENGTHS[k][a][b] / 100.0 for k in range(3)] for b in range(n)] for a in range(n)],
                        dtype=torch.float64)


def aromatic_length0_table(is_geom):
    """fp64 ``[n_types][n_types]``: the length of a bond ``dl_aromatic_rings`` flags aromatic: ``AROMATIC_LENGTHS`` where it
    has the pair, else the mean of the single and the double length, else the single length (0: no term)."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    rows = [[0.0] * n for _ in range(n)]
    for a in range(n):
        for b in range(n):
            pair = (GEOM_IDX2ATOM[a], GEOM_IDX2ATOM[b])
            single, double = BOND_LENGTHS[0][a][b] / 100.0, BOND_LENGTHS[1][a][b] / 100.0
            if pair in AROMATIC_LENGTHS or pair[::-1] in AROMATIC_LENGTHS:
                rows[a][b] = AROMATIC_LENGTHS.get(pair, AROMATIC_LENGTHS.get(pair[::-1]))
            elif single and double:
                rows[a][b] = (single + double) / 2.0
            else:
                rows[a][b] = single
    return torch.tensor(rows, dtype=torch.float64)


def ideal_cos_table():
    """fp64 ``[3]``: the ideal cosine of the classes ``ANGLE_CLASSES``: -1, -1/2 and -1/3."""
    return torch.tensor(IDEAL_COS, dtype=torch.float64)


def relax_reach_table(is_geom, scale=RELAX_REACH_SCALE):
    """fp64 ``[n_types][n_types]`` SQUARED distances in Angstrom^2 inside which two atoms repel in ``relax``:
    ``(scale * (VDW_RADII[a] + VDW_RADII[b])) ** 2``, formed as ``internal_clash_table`` forms its own."""
    return internal_clash_table(is_geom, scale)


# The atom radii of Trott & Olson's scoring function (AutoDock Vina, J. Comput. Chem. 31, 455 (2010)) in Angstrom by GEOM atom
# index (C O N F S Cl Br I P), from which ``metrics.analyze_interactions`` forms surface distances, and the published weights
# of its five intermolecular terms: gauss1, gauss2, repulsion, hydrophobic, hydrogen bond.  The rotor weight is not used
XS_RADII = (1.9, 1.7, 1.8, 1.5, 2.0, 1.8, 2.0, 2.2, 2.1)
INTERACTION_WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)


def xs_radius_table(is_geom):
    """fp64 ``[n_types]``: ``XS_RADII`` of the vocabulary, in index order."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    return torch.tensor(XS_RADII[:n], dtype=torch.float64)


def shape_radius_table(is_geom, scale=0.8, step=0.25):
    """``[n_types][3]`` fp32 SQUARED radii in Angstrom^2 of the three levels of the shape rule (``metrics.analyze_shapes``):
    ``r_k = scale * VDW_RADII[type] + k * step`` for ``k = 0, 1, 2`` in fp64, rounded to fp32 once, then ``r_k * r_k`` as one
    fp32 multiplication.  The defaults follow RDKit's shape encoding (``vdwScale`` 0.8, ``stepSize`` 0.25, two layers)."""
    n = GEOM_NUMBER_OF_ATOM_TYPES if is_geom else NUMBER_OF_ATOM_TYPES
    radii = torch.tensor([[float(scale) * VDW_RADII[t] + k * float(step) for k in range(3)] for t in range(n)],
                         dtype=torch.float64).to(TORCH_FLOAT)
    return radii * radii


# ---- the parameters of ``metrics.stereo`` (``dl_stereo_perceive``).  Parameters of the rule, not measurements: a centre
# squashed to a quarter of the ideal chiral volume cannot be called (``flat``), and neither can a double bond whose reference
# arms are twisted more than 60 degrees out of plane (``twist`` = cos 60).  The two ideal volumes are the determinants of the
# rule at the regular tetrahedron, 16/(3 sqrt 3) with four neighbours and 4/(3 sqrt 3) with three and a hydrogen, formed in
# fp64 as plain Python floats with one rounding per operation
STEREO_DEFAULTS = {'flat': 0.25, 'twist': 0.5}
STEREO_V_IDEAL = (16.0 / (3.0 * math.sqrt(3.0)), 4.0 / (3.0 * math.sqrt(3.0)))
