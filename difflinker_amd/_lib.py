"""ctypes binding of ``libdifflinker_hip.so`` (C ABI declared in ``include/difflinker_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``hipcc --offload-arch=gfx950``).
There is deliberately NO fallback: if the shared object is missing or cannot be loaded every
compute entry point of the package raises, it never routes to a CPU/PyTorch implementation.
"""
import ctypes
import os

import torch  # noqa: F401  (loads PyTorch-ROCm's libamdhip64 first so both share one HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFFLINKER_HIP_LIB: load another build of the same library (kernel A/B experiments)
LIB_PATH = os.environ.get('DIFFLINKER_HIP_LIB') or os.path.join(_HERE, 'libdifflinker_hip.so')
# the same sources compiled with -DDL_TEST_HOOKS (fault injection for tests/test_gpu_team.py); never loaded by the package itself
TEST_HOOKS_LIB_PATH = os.path.join(_HERE, 'libdifflinker_hip_testhooks.so')

DL_OK = 0
ABI_VERSION = 7
PRECISIONS = {'fp32': 0, 'f16x3': 1, 'f16x2': 2}
DL_ERR_TOO_MANY_ATOMS = -3


class DLConfig(ctypes.Structure):
    _fields_ = [
        ('n_dims', ctypes.c_int32), ('in_node_nf', ctypes.c_int32), ('context_node_nf', ctypes.c_int32),
        ('hidden_nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('inv_sublayers', ctypes.c_int32),
        ('condition_time', ctypes.c_int32), ('norm_constant', ctypes.c_float),
        ('normalization_factor', ctypes.c_float), ('precision', ctypes.c_int32),
        ('attention', ctypes.c_int32), ('tanh', ctypes.c_int32), ('coords_range', ctypes.c_float),
        ('aggregation_mean', ctypes.c_int32), ('sin_embedding', ctypes.c_int32),
    ]


class DLSizeConfig(ctypes.Structure):
    _fields_ = [('in_node_nf', ctypes.c_int32), ('hidden_nf', ctypes.c_int32), ('out_node_nf', ctypes.c_int32),
                ('n_layers', ctypes.c_int32)]


class DLInpaintCoef(ctypes.Structure):
    _fields_ = [('alpha_ts', ctypes.c_float), ('c_eps', ctypes.c_float), ('sigma', ctypes.c_float),
                ('a_q', ctypes.c_float), ('b_q', ctypes.c_float), ('decode', ctypes.c_int32),
                ('inv_alpha0', ctypes.c_float), ('sigma0', ctypes.c_float), ('sigma_x', ctypes.c_float),
                ('norm_x', ctypes.c_float), ('norm_h', ctypes.c_float), ('bias_h', ctypes.c_float)]


class DLStepCoef(ctypes.Structure):
    _fields_ = [('t', ctypes.c_float), ('alpha_ts', ctypes.c_float), ('c_eps', ctypes.c_float),
                ('sigma', ctypes.c_float)]


class DLChainArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('T', ctypes.c_int32), ('keep_frames', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('h', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('fragment_mask', ctypes.c_void_p), ('linker_mask', ctypes.c_void_p), ('edge_mask', ctypes.c_void_p),
        ('context', ctypes.c_void_p), ('noise_x', ctypes.c_void_p), ('noise_h', ctypes.c_void_p),
        ('noise_seed', ctypes.c_uint64), ('mol_offset', ctypes.c_int32), ('team', ctypes.c_int32),
        ('coefs', ctypes.c_void_p),
        ('inv_alpha0', ctypes.c_float), ('sigma0', ctypes.c_float), ('sigma_x', ctypes.c_float),
        ('norm_x', ctypes.c_float), ('norm_h', ctypes.c_float), ('bias_h', ctypes.c_float),
        ('chain', ctypes.c_void_p), ('nan_flags', ctypes.c_void_p), ('nan_step', ctypes.c_void_p),
        ('order', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
        ('mol_index', ctypes.c_void_p), ('order_first', ctypes.c_int32), ('order_count', ctypes.c_int32),
        ('q_begin', ctypes.c_void_p), ('q_end', ctypes.c_void_p), ('z_state', ctypes.c_void_p), ('skip_flags', ctypes.c_void_p),
    ]


class DLJoinArgs(ctypes.Structure):
    _fields_ = [
        ('teams', ctypes.c_int32), ('team_of', ctypes.c_void_p), ('team_mol', ctypes.c_void_p),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t), ('wait_ticks', ctypes.c_void_p),
    ]


LOSS_ROW = 8          # DL_LOSS_ROW: error_t, |eps_hat|, kl_prior, log p(x|z0), log p(h|z0), log constant, SNR weight, atoms


class DLLossArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32), ('T', ctypes.c_int32),
        ('timesteps', ctypes.c_int32), ('inpainting', ctypes.c_int32),
        ('xh', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('fragment_mask', ctypes.c_void_p),
        ('linker_mask', ctypes.c_void_p), ('gamma_table', ctypes.c_void_p), ('noise_x', ctypes.c_void_p),
        ('noise_h', ctypes.c_void_p), ('noise_seed', ctypes.c_uint64), ('mol_offset', ctypes.c_int32),
        ('t_given', ctypes.c_int32), ('t_int', ctypes.c_void_p), ('t', ctypes.c_void_p), ('gamma', ctypes.c_void_p),
        ('z_t', ctypes.c_void_p), ('eps_hat', ctypes.c_void_p), ('norm_h', ctypes.c_float), ('bias_h', ctypes.c_float),
        ('prior', ctypes.c_void_p), ('rows', ctypes.c_void_p),
    ]


class DLBackwardArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('in_node_nf', ctypes.c_int32), ('context_node_nf', ctypes.c_int32),
        ('condition_time', ctypes.c_int32), ('hidden_nf', ctypes.c_int32), ('n_layers', ctypes.c_int32),
        ('inv_sublayers', ctypes.c_int32), ('centering', ctypes.c_int32), ('norm_constant', ctypes.c_float),
        ('normalization_factor', ctypes.c_float), ('params', ctypes.c_void_p), ('n_params', ctypes.c_int64),
        ('xh', ctypes.c_void_p), ('t', ctypes.c_void_p), ('t_is_scalar', ctypes.c_int32), ('node_mask', ctypes.c_void_p),
        ('linker_mask', ctypes.c_void_p), ('edge_mask', ctypes.c_void_p), ('context', ctypes.c_void_p),
        ('grad_out', ctypes.c_void_p), ('grad_params', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
        ('workspace_bytes', ctypes.c_size_t),
    ]


class DLSizeTrainArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('in_node_nf', ctypes.c_int32), ('hidden_nf', ctypes.c_int32),
        ('out_node_nf', ctypes.c_int32), ('n_layers', ctypes.c_int32), ('batch_norm', ctypes.c_int32),
        ('params', ctypes.c_void_p), ('n_params', ctypes.c_int64), ('one_hot', ctypes.c_void_p),
        ('positions', ctypes.c_void_p), ('fragment_mask', ctypes.c_void_p), ('edge_mask', ctypes.c_void_p),
        ('logits', ctypes.c_void_p), ('batch_stats', ctypes.c_void_p), ('flags', ctypes.c_void_p),
        ('grad_logits', ctypes.c_void_p), ('grad_params', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
        ('workspace_bytes', ctypes.c_size_t),
    ]


DL_BONDS_OVERFLOW, DL_BONDS_NONFINITE = 1, 2      # dl_bonds_args.status bits


class DLBondsArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('x', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('table', ctypes.c_void_p),
        ('table_len', ctypes.c_int32), ('capacity', ctypes.c_int32),
        ('n_bonds', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('valence', ctypes.c_void_p),
        ('n_components', ctypes.c_void_p), ('component', ctypes.c_void_p), ('status', ctypes.c_void_p),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_size_t),
    ]


DL_KEYS_TOO_LARGE, DL_KEYS_BAD_BOND = 4, 8         # dl_mol_keys_args.status bits, beside the DL_BONDS_* bits carried forward


class DLMolKeysArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('drop_mask', ctypes.c_void_p),
        ('capacity', ctypes.c_int32), ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p),
        ('valence_in', ctypes.c_void_p), ('n_components_in', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('max_valence', ctypes.c_void_p), ('max_valence_len', ctypes.c_int32),
        ('n_atoms', ctypes.c_void_p), ('n_over', ctypes.c_void_p), ('n_components', ctypes.c_void_p),
        ('n_bonds', ctypes.c_void_p), ('key', ctypes.c_void_p), ('colour', ctypes.c_void_p), ('status', ctypes.c_void_p),
    ]


DL_RMSD_NONFINITE, DL_RMSD_NO_MAP, DL_RMSD_TOO_LARGE = 1, 2, 4      # dl_rmsd_args.status bits


class DLRmsdArgs(ctypes.Structure):
    _fields_ = [
        ('P', ctypes.c_int32), ('n_max', ctypes.c_int32), ('xa', ctypes.c_void_p), ('xb', ctypes.c_void_p),
        ('n_atoms', ctypes.c_void_p), ('map_offsets', ctypes.c_void_p), ('maps', ctypes.c_void_p),
        ('maps_capacity', ctypes.c_int32), ('rmsd', ctypes.c_void_p), ('best', ctypes.c_void_p), ('status', ctypes.c_void_p),
    ]


DL_CLASH_NONFINITE, DL_CLASH_TOO_LARGE, DL_CLASH_BAD_TYPE = 1, 2, 4      # dl_clash_args.status bits


class DLClashArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('query_mask', ctypes.c_void_p),
        ('target_mask', ctypes.c_void_p), ('M', ctypes.c_int32), ('target_x', ctypes.c_void_p),
        ('target_type', ctypes.c_void_p), ('threshold', ctypes.c_void_p), ('contact_cutoff', ctypes.c_float),
        ('n_query', ctypes.c_void_p), ('n_target', ctypes.c_void_p), ('n_clashes', ctypes.c_void_p),
        ('n_clash_atoms', ctypes.c_void_p), ('n_contacts', ctypes.c_void_p), ('min_dist2', ctypes.c_void_p),
        ('status', ctypes.c_void_p), ('atom_clashes', ctypes.c_void_p), ('atom_min_dist2', ctypes.c_void_p),
    ]


DL_XS_HYDROPHOBIC, DL_XS_DONOR, DL_XS_ACCEPTOR = 16, 32, 64               # xs_type bits above the element index (bits 0-3)
DL_INTERACT_TERMS = 5                                                     # gauss1, gauss2, repulsion, hydrophobic, hbond
DL_INTERACT_NONFINITE, DL_INTERACT_TOO_LARGE, DL_INTERACT_BAD_TYPE, DL_INTERACT_UNTYPED = 1, 2, 4, 8   # status bits


class DLInteractTypesArgs(ctypes.Structure):           # the stream is the last FIELD, as for dl_fingerprints
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('group', ctypes.c_void_p), ('table', ctypes.c_void_p),
        ('xs_type', ctypes.c_void_p), ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


class DLInteractArgs(ctypes.Structure):                # likewise
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('xs_type', ctypes.c_void_p), ('query_mask', ctypes.c_void_p),
        ('target_mask', ctypes.c_void_p), ('M', ctypes.c_int32), ('target_x', ctypes.c_void_p),
        ('target_xs', ctypes.c_void_p), ('radius', ctypes.c_void_p),
        ('n_query', ctypes.c_void_p), ('n_target', ctypes.c_void_p), ('n_pairs', ctypes.c_void_p),
        ('n_hbonds', ctypes.c_void_p), ('n_hydrophobic', ctypes.c_void_p), ('terms', ctypes.c_void_p),
        ('status', ctypes.c_void_p), ('atom_terms', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


DL_SHAPE_NONFINITE, DL_SHAPE_OUT_OF_RANGE, DL_SHAPE_TOO_LARGE = 1, 2, 4  # dl_shape_args.status: one of these, or 0


class DLShapeArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('Na', ctypes.c_int32), ('Nb', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x_a', ctypes.c_void_p), ('one_hot_a', ctypes.c_void_p), ('mask_a', ctypes.c_void_p),
        ('x_b', ctypes.c_void_p), ('one_hot_b', ctypes.c_void_p), ('mask_b', ctypes.c_void_p),
        ('r2', ctypes.c_void_p),
        ('vol_a', ctypes.c_void_p), ('vol_b', ctypes.c_void_p), ('vol_min', ctypes.c_void_p),
        ('core_a', ctypes.c_void_p), ('core_b', ctypes.c_void_p), ('core_both', ctypes.c_void_p),
        ('n_a', ctypes.c_void_p), ('n_b', ctypes.c_void_p), ('status', ctypes.c_void_p),
    ]


DL_RINGS_MAX_ATOMS, DL_RING_BINS = 256, 7             # dl_rings_args: kept atoms per molecule; bins of ring_hist
DL_RINGS_TOO_LARGE, DL_RINGS_BAD_BOND = 4, 8          # dl_rings_args.status bits, beside the DL_BONDS_* bits carried forward


class DLRingsArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32),
        ('node_mask', ctypes.c_void_p), ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('n_atoms', ctypes.c_void_p), ('n_bonds', ctypes.c_void_p), ('n_components', ctypes.c_void_p),
        ('n_rings', ctypes.c_void_p), ('bond_ring', ctypes.c_void_p), ('atom_ring', ctypes.c_void_p),
        ('ring_hist', ctypes.c_void_p), ('status', ctypes.c_void_p),
    ]


DL_FRAG_MAX_ATOMS, DL_FRAG_CUT_FIELDS = 256, 10        # dl_fragment_args: atoms per molecule; int32 values per cut record
DL_FRAG_TOO_LARGE, DL_FRAG_BAD_BOND = 4, 8            # dl_fragment_args.status bits, beside the DL_BONDS_* bits carried forward
DL_FRAG_DISCONNECTED, DL_FRAG_TRUNCATED = 16, 32


class DLFragmentArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('charge', ctypes.c_void_p),
        ('carbon_type', ctypes.c_int32), ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('min_linker', ctypes.c_int32), ('min_fragment', ctypes.c_int32), ('min_path_atoms', ctypes.c_int32),
        ('linker_leq_frags', ctypes.c_int32), ('R', ctypes.c_int32),
        ('n_atoms', ctypes.c_void_p), ('n_bonds', ctypes.c_void_p), ('n_cuttable', ctypes.c_void_p),
        ('n_cuts', ctypes.c_void_p), ('status', ctypes.c_void_p), ('bond_side', ctypes.c_void_p),
        ('cuts', ctypes.c_void_p), ('labels', ctypes.c_void_p),
    ]


DL_FRAG_MULTI_FIELDS, DL_FRAG_MULTI_MIN_CUTS, DL_FRAG_MULTI_MAX_CUTS = 22, 3, 5     # dl_fragment_multi_args: ints per record; k
DL_FRAG_MULTI_MAX_CUTTABLE, DL_FRAG_MULTI_LINKER = 64, 5                        # cuttable bonds of a molecule that is cut; a label
DL_FRAG_MANY_CUTTABLE = 64                                                      # dl_fragment_multi_args.status bit


class DLFragmentMultiArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('charge', ctypes.c_void_p),
        ('carbon_type', ctypes.c_int32), ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('min_cuts', ctypes.c_int32), ('max_cuts', ctypes.c_int32), ('min_linker', ctypes.c_int32),
        ('min_fragment', ctypes.c_int32), ('max_atoms', ctypes.c_int32), ('min_rings', ctypes.c_int32), ('R', ctypes.c_int32),
        ('n_atoms', ctypes.c_void_p), ('n_bonds', ctypes.c_void_p), ('n_cuttable', ctypes.c_void_p),
        ('n_cuts', ctypes.c_void_p), ('status', ctypes.c_void_p), ('n_cuts_k', ctypes.c_void_p),
        ('cuts', ctypes.c_void_p), ('labels', ctypes.c_void_p),
    ]


DL_AROM_MAX_ATOMS, DL_AROM_MAX_RINGS, DL_AROM_MAX_SYSTEM = 256, 64, 32        # dl_aromatic_args: kept atoms, planar rings, system atoms
DL_AROM_TOO_LARGE, DL_AROM_BAD_BOND = 4, 8            # dl_aromatic_args.status bits, beside the DL_BONDS_* bits carried forward
DL_AROM_MANY_RINGS, DL_AROM_BIG_SYSTEM = 16, 32


class DLAromaticArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p), ('ring_class', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('tol2_ring', ctypes.c_double), ('tol2_sub', ctypes.c_double),
        ('order_out', ctypes.c_void_p), ('bond_aromatic', ctypes.c_void_p), ('atom_aromatic', ctypes.c_void_p),
        ('valence_out', ctypes.c_void_p), ('n_planar_rings', ctypes.c_void_p), ('n_aromatic_rings', ctypes.c_void_p),
        ('n_aromatic_marked', ctypes.c_void_p), ('status', ctypes.c_void_p),
    ]


DL_POCKET_MAX_LIGAND, DL_POCKET_MAX_GROUPS = 256, 32768                     # dl_pocket_args: ligand atoms per pair; groups per protein
DL_POCKET_NONFINITE, DL_POCKET_TOO_LARGE, DL_POCKET_TOO_MANY_GROUPS = 1, 2, 4  # dl_pocket_args.status bits
DL_POCKET_BAD_PROTEIN, DL_POCKET_TRUNCATED = 8, 32


class DLPocketArgs(ctypes.Structure):
    _fields_ = [
        ('B', ctypes.c_int32), ('L', ctypes.c_int32), ('P', ctypes.c_int32), ('M_total', ctypes.c_int32),
        ('protein_x', ctypes.c_void_p), ('protein_group', ctypes.c_void_p), ('protein_offset', ctypes.c_void_p),
        ('pair_protein', ctypes.c_void_p), ('ligand_x', ctypes.c_void_p), ('ligand_mask', ctypes.c_void_p),
        ('cutoff', ctypes.c_double), ('Mmax', ctypes.c_int32), ('capacity', ctypes.c_int32),
        ('n_ligand', ctypes.c_void_p), ('n_contact_atoms', ctypes.c_void_p), ('n_groups_selected', ctypes.c_void_p),
        ('n_pocket', ctypes.c_void_p), ('status', ctypes.c_void_p), ('member', ctypes.c_void_p), ('index', ctypes.c_void_p),
    ]


DL_FP_MAX_ATOMS, DL_FP_MAX_RADIUS = 256, 4              # dl_fingerprint_args: kept atoms per molecule; rounds of refinement
DL_FP_TOO_LARGE, DL_FP_BAD_BOND = 4, 8                # dl_fingerprint_args.status bits, beside the DL_BONDS_* bits carried forward
DL_FP_BITS = (512, 1024, 2048)                        # n_bits dl_fingerprints takes
DL_TANIMOTO_TILE = 128                                # rows of B a workgroup of dl_tanimoto_nearest stages at a time


class DLFingerprintArgs(ctypes.Structure):            # the stream is the last FIELD: the entry point takes the struct alone
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('drop_mask', ctypes.c_void_p),
        ('centre_mask', ctypes.c_void_p), ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('radius', ctypes.c_int32), ('n_bits', ctypes.c_int32),
        ('bits', ctypes.c_void_p), ('n_on', ctypes.c_void_p), ('n_atoms', ctypes.c_void_p), ('n_centres', ctypes.c_void_p),
        ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


class DLTanimotoArgs(ctypes.Structure):               # likewise
    _fields_ = [
        ('Ma', ctypes.c_int32), ('Mb', ctypes.c_int32), ('W', ctypes.c_int32), ('G', ctypes.c_int32),
        ('a_bits', ctypes.c_void_p), ('b_bits', ctypes.c_void_p), ('a_offsets', ctypes.c_void_p), ('b_offsets', ctypes.c_void_p),
        ('exclude_diagonal', ctypes.c_int32),
        ('nn_index', ctypes.c_void_p), ('nn_common', ctypes.c_void_p), ('nn_union', ctypes.c_void_p), ('n_pairs', ctypes.c_void_p),
        ('sum_q20', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


DL_SELECT_MAX_ROWS = 4096                             # rows per group of dl_tanimoto_cluster and dl_tanimoto_pick
DL_SELECT_TOO_LARGE, DL_SELECT_BAD_FIRST = 4, 16      # dl_cluster_args.status / dl_pick_args.status bits


class DLClusterArgs(ctypes.Structure):                # the stream is the last FIELD, as for dl_tanimoto_nearest
    _fields_ = [
        ('M', ctypes.c_int32), ('W', ctypes.c_int32), ('G', ctypes.c_int32),
        ('bits', ctypes.c_void_p), ('offsets', ctypes.c_void_p), ('num', ctypes.c_int32), ('den', ctypes.c_int32),
        ('cluster', ctypes.c_void_p), ('centroid', ctypes.c_void_p), ('n_neighbours', ctypes.c_void_p),
        ('n_clusters', ctypes.c_void_p), ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


class DLPickArgs(ctypes.Structure):                   # likewise
    _fields_ = [
        ('M', ctypes.c_int32), ('W', ctypes.c_int32), ('G', ctypes.c_int32), ('K', ctypes.c_int32),
        ('bits', ctypes.c_void_p), ('offsets', ctypes.c_void_p), ('first', ctypes.c_void_p),
        ('picks', ctypes.c_void_p), ('pick_common', ctypes.c_void_p), ('pick_union', ctypes.c_void_p),
        ('n_picked', ctypes.c_void_p), ('status', ctypes.c_void_p), ('pick_rank', ctypes.c_void_p),
        ('stream', ctypes.c_void_p),
    ]


DL_PHARM_MAX_ATOMS, DL_PHARM_MAX_RINGS, DL_PHARM_FAMILIES = 256, 64, 7   # dl_pharm_args: kept atoms, aromatic rings; families
DL_PHARM_TOO_LARGE, DL_PHARM_BAD_BOND = 4, 8          # dl_pharm_args.status bits, beside the DL_BONDS_* bits carried forward
DL_PHARM_MANY_RINGS, DL_PHARM_OVERFLOW, DL_PHARM_NONFINITE = 16, 32, 64


class DLPharmArgs(ctypes.Structure):                  # the stream is the last FIELD, as for dl_fingerprints
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p), ('feature_class', ctypes.c_void_p),
        ('default_valence', ctypes.c_void_p), ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('bond_aromatic', ctypes.c_void_p),
        ('status_in', ctypes.c_void_p), ('Fcap', ctypes.c_int32),
        ('family', ctypes.c_void_p), ('anchor', ctypes.c_void_p), ('position', ctypes.c_void_p), ('marked', ctypes.c_void_p),
        ('n_features', ctypes.c_void_p), ('family_count', ctypes.c_void_p), ('status', ctypes.c_void_p),
        ('stream', ctypes.c_void_p),
    ]


DL_HYDRO_MAX_ATOMS = 256                              # dl_hydrogens_args: kept atoms per molecule
DL_HYDRO_TOO_LARGE, DL_HYDRO_BAD_BOND = 4, 8          # dl_hydrogens_args.status bits, beside the DL_BONDS_* bits carried forward
DL_HYDRO_OVERFLOW, DL_HYDRO_NONFINITE = 32, 64


class DLHydrogensArgs(ctypes.Structure):                # the stream is the last FIELD, as for dl_fingerprints
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('atom_planar', ctypes.c_void_p), ('default_valence', ctypes.c_void_p),
        ('xh_length', ctypes.c_void_p), ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('Hcap', ctypes.c_int32),
        ('n_h', ctypes.c_void_p), ('h_count', ctypes.c_void_p), ('h_parent', ctypes.c_void_p), ('h_x', ctypes.c_void_p),
        ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


DL_POSE_MAX_ATOMS, DL_POSE_COUNTS = 256, 8            # dl_pose_args: kept atoms per molecule; values per row of counts
DL_POSE_TOO_LARGE, DL_POSE_BAD_BOND, DL_POSE_NONFINITE = 4, 8, 64     # dl_pose_args.status bits, beside the DL_BONDS_* bits carried forward


class DLPoseArgs(ctypes.Structure):                   # the stream is the last FIELD, as for dl_add_hydrogens
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p), ('atom_planar', ctypes.c_void_p),
        ('length_bounds2', ctypes.c_void_p), ('angle_cos', ctypes.c_void_p), ('clash2', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('counts', ctypes.c_void_p), ('atom_flags', ctypes.c_void_p), ('status', ctypes.c_void_p),
        ('stream', ctypes.c_void_p),
    ]


DL_RELAX_MAX_ATOMS, DL_RELAX_MAX_STEPS, DL_RELAX_TERMS = 256, 1000, 5     # dl_relax_args: kept atoms, steps, values per row of energy
DL_RELAX_DIVERGED = 128                               # dl_relax_args.status bit, beside the DL_POSE_* and DL_BONDS_* bits
RELAX_CONSTANTS = ('k_bond', 'k_angle', 'k_rep', 'k_wall', 'k_pos', 'dt0', 'dt_max', 'alpha0', 'f_inc', 'f_dec', 'f_alpha',
                   'max_step', 'f_tol')               # the fp64 fields of dl_relax_args, in its order


class DLRelaxArgs(ctypes.Structure):                  # the stream is the last FIELD, as for dl_pose_checks
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p), ('atom_planar', ctypes.c_void_p),
        ('length0', ctypes.c_void_p), ('aromatic_length0', ctypes.c_void_p), ('ideal_cos', ctypes.c_void_p),
        ('reach2', ctypes.c_void_p), ('wall_reach2', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('bond_aromatic', ctypes.c_void_p),
        ('status_in', ctypes.c_void_p),
        ('use_wall', ctypes.c_int32), ('steps', ctypes.c_int32), ('n_min', ctypes.c_int32),
    ] + [(name, ctypes.c_double) for name in RELAX_CONSTANTS] + [
        ('x_out', ctypes.c_void_p), ('energy', ctypes.c_void_p), ('steps_done', ctypes.c_void_p), ('f_max', ctypes.c_void_p),
        ('moved2', ctypes.c_void_p), ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


DL_CANON_MAX_ATOMS, DL_CANON_MAX_BONDS, DL_CANON_MAX_DEPTH, DL_CANON_MAX_LEAVES = 256, 2048, 32, 65536   # dl_canon_args limits
DL_CANON_TOO_LARGE, DL_CANON_BAD_BOND, DL_CANON_BUDGET = 4, 8, 256     # dl_canon_args.status bits, beside the DL_BONDS_* bits


class DLCanonArgs(ctypes.Structure):                  # the stream is the last FIELD, as for dl_relax_molecules
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('drop_mask', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('status_in', ctypes.c_void_p),
        ('max_leaves', ctypes.c_int32),
        ('rank', ctypes.c_void_p), ('code', ctypes.c_void_p), ('n_leaves', ctypes.c_void_p), ('status', ctypes.c_void_p),
        ('stream', ctypes.c_void_p),
    ]


DL_SUB_MAX_ATOMS, DL_SUB_MAX_BONDS = 256, 2048         # dl_substructure_args: kept atoms and kept list entries per molecule
DL_SUB_MAX_PATTERN_ATOMS, DL_SUB_MAX_SUBPATTERNS, DL_SUB_MAX_LEVELS, DL_SUB_MAX_PRED = 48, 256, 4, 32      # the limits of a catalogue
DL_SUB_TOO_LARGE, DL_SUB_BAD_BOND, DL_SUB_BUDGET = 4, 8, 512       # dl_substructure_args.status bits, beside the DL_BONDS_* bits


class DLSubstructureArgs(ctypes.Structure):           # the stream is the last FIELD, as for dl_canonical_ranks
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p), ('drop_mask', ctypes.c_void_p),
        ('mark_mask', ctypes.c_void_p), ('atomic_number', ctypes.c_void_p), ('default_valence', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('bond_aromatic', ctypes.c_void_p),
        ('status_in', ctypes.c_void_p),
        ('n_sub', ctypes.c_int32), ('n_top', ctypes.c_int32), ('n_levels', ctypes.c_int32),
        ('level_end', ctypes.c_int32 * DL_SUB_MAX_LEVELS),
        ('pat', ctypes.c_void_p), ('atoms', ctypes.c_void_p), ('closures', ctypes.c_void_p), ('preds', ctypes.c_void_p),
        ('n_atoms_table', ctypes.c_int32), ('n_closures', ctypes.c_int32), ('n_preds', ctypes.c_int32),
        ('max_steps', ctypes.c_int32),
        ('first_root', ctypes.c_void_p), ('first_root_marked', ctypes.c_void_p), ('n_hits', ctypes.c_void_p),
        ('n_hits_marked', ctypes.c_void_p), ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


DL_STEREO_MAX_ATOMS, DL_STEREO_MAX_BONDS, DL_STEREO_COUNTS = 256, 2048, 4     # dl_stereo_args: kept atoms, kept list entries, values per row of counts
DL_STEREO_TOO_LARGE, DL_STEREO_BAD_BOND, DL_STEREO_NONFINITE = 4, 8, 64      # dl_stereo_args.status bits, beside the DL_BONDS_* bits


class DLStereoArgs(ctypes.Structure):                 # the stream is the last FIELD, as for dl_pose_checks
    _fields_ = [
        ('B', ctypes.c_int32), ('N', ctypes.c_int32), ('nf', ctypes.c_int32),
        ('x', ctypes.c_void_p), ('one_hot', ctypes.c_void_p), ('node_mask', ctypes.c_void_p),
        ('drop_mask', ctypes.c_void_p), ('mark_mask', ctypes.c_void_p), ('atom_planar', ctypes.c_void_p),
        ('default_valence', ctypes.c_void_p),
        ('capacity', ctypes.c_int32),
        ('n_bonds_in', ctypes.c_void_p), ('bonds', ctypes.c_void_p), ('bond_aromatic', ctypes.c_void_p),
        ('status_in', ctypes.c_void_p),
        ('flat', ctypes.c_double), ('twist', ctypes.c_double), ('v_ideal4', ctypes.c_double), ('v_ideal3', ctypes.c_double),
        ('atom_class', ctypes.c_void_p), ('atom_stereo', ctypes.c_void_p), ('bond_stereo', ctypes.c_void_p),
        ('counts', ctypes.c_void_p), ('status', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


class DLFeatureMatchArgs(ctypes.Structure):           # likewise
    _fields_ = [
        ('B', ctypes.c_int32), ('Fa', ctypes.c_int32), ('Fb', ctypes.c_int32),
        ('family_a', ctypes.c_void_p), ('position_a', ctypes.c_void_p), ('marked_a', ctypes.c_void_p),
        ('n_features_a', ctypes.c_void_p),
        ('family_b', ctypes.c_void_p), ('position_b', ctypes.c_void_p), ('marked_b', ctypes.c_void_p),
        ('n_features_b', ctypes.c_void_p),
        ('radius2', ctypes.c_float), ('marked_only', ctypes.c_int32),
        ('best_index', ctypes.c_void_p), ('best_d2', ctypes.c_void_p), ('n_a', ctypes.c_void_p), ('n_b', ctypes.c_void_p),
        ('n_matched', ctypes.c_void_p), ('stream', ctypes.c_void_p),
    ]


EXPORTS = ('dl_abi_version', 'dl_last_hip_error', 'dl_max_atoms', 'dl_error_string', 'dl_model_num_tensors',
           'dl_model_create', 'dl_model_destroy', 'dl_egnn_forward_fc', 'dl_sampler_step', 'dl_sample_chain_fc',
           'dl_set_profile_buffer', 'dl_profile_max_events', 'dl_pocket_workspace_bytes', 'dl_egnn_forward_pocket',
           'dl_size_model_num_tensors', 'dl_size_model_create', 'dl_size_model_destroy', 'dl_size_max_fragment_atoms',
           'dl_size_gnn_forward', 'dl_philox_fill', 'dl_egnn_forward_fc_large', 'dl_inpaint_step', 'dl_workspace_bytes',
           'dl_team_max', 'dl_egnn_forward_fc_team', 'dl_team_max_atoms',
           'dl_edm_loss_prologue', 'dl_edm_loss_epilogue', 'dl_edm_loss_grad', 'dl_egnn_backward_fc_num_params',
           'dl_egnn_backward_fc_workspace_bytes', 'dl_egnn_backward_max_atoms', 'dl_egnn_backward_fc',
           'dl_egnn_backward_pocket_workspace_bytes', 'dl_egnn_backward_pocket',
           'dl_size_train_num_params', 'dl_size_train_workspace_bytes', 'dl_size_train_forward', 'dl_size_train_backward',
           'dl_substructure_match', 'dl_stereo_perceive',
           'dl_join_workspace_bytes', 'dl_sample_chain_fc_join', 'dl_tanimoto_cluster', 'dl_tanimoto_pick',
           'dl_bonds_workspace_bytes', 'dl_canonical_ranks', 'dl_perceive_bonds',
           'dl_pose_checks',
           'dl_interaction_types', 'dl_relax_molecules', 'dl_interaction_scores', 'dl_add_hydrogens',
           'dl_molecule_keys', 'dl_clash_scores', 'dl_shape_scores', 'dl_ring_scores', 'dl_fragment_cuts',
           'dl_pocket_select', 'dl_fragment_multicuts', 'dl_aromatic_rings', 'dl_fingerprints',
           'dl_tanimoto_nearest', 'dl_pharmacophore_features', 'dl_feature_match', 'dl_best_rmsd')
TEST_HOOK_EXPORTS = ('dl_debug_team_fault', 'dl_debug_slot_order')       # declared under #ifdef DL_TEST_HOOKS: the test-hooks build only

# The entry points that take one struct and return a status: ``int32 f(const STRUCT*)`` when the struct's last field is
# ``stream``, ``int32 f(const STRUCT*, void* stream)`` otherwise.  ``_open`` declares them from this table and ``launch``
# calls them; which of the two forms an entry point has is read from the struct (``_stream_is_field``) and stated nowhere else.
STRUCT_ENTRY_POINTS = {
    'dl_edm_loss_prologue': DLLossArgs, 'dl_edm_loss_epilogue': DLLossArgs, 'dl_egnn_backward_fc': DLBackwardArgs,
    'dl_size_train_forward': DLSizeTrainArgs, 'dl_size_train_backward': DLSizeTrainArgs,
    'dl_perceive_bonds': DLBondsArgs, 'dl_molecule_keys': DLMolKeysArgs, 'dl_best_rmsd': DLRmsdArgs,
    'dl_clash_scores': DLClashArgs, 'dl_shape_scores': DLShapeArgs, 'dl_ring_scores': DLRingsArgs,
    'dl_fragment_cuts': DLFragmentArgs, 'dl_fragment_multicuts': DLFragmentMultiArgs, 'dl_aromatic_rings': DLAromaticArgs,
    'dl_pocket_select': DLPocketArgs,
    'dl_interaction_types': DLInteractTypesArgs, 'dl_interaction_scores': DLInteractArgs,
    'dl_fingerprints': DLFingerprintArgs, 'dl_tanimoto_nearest': DLTanimotoArgs,
    'dl_pharmacophore_features': DLPharmArgs, 'dl_feature_match': DLFeatureMatchArgs,
    'dl_add_hydrogens': DLHydrogensArgs, 'dl_pose_checks': DLPoseArgs,
}
# The selections over fingerprint sets (select.hip), declared and called in the same way: a table of its own, because
# tests/test_lib_host.py pins the table above name by name.
SELECT_ENTRY_POINTS = {'dl_tanimoto_cluster': DLClusterArgs, 'dl_tanimoto_pick': DLPickArgs}
# The relaxation (relax.hip), likewise a table of its own: tests/test_select_host.py pins the one above.
RELAX_ENTRY_POINTS = {'dl_relax_molecules': DLRelaxArgs}
# The canonical labelling (canon.hip), likewise: tests/test_relax_host.py pins the one above.
CANON_ENTRY_POINTS = {'dl_canonical_ranks': DLCanonArgs}
# The substructure search (substructure.hip), likewise: tests/test_canon_host.py pins the one above.
SUBSTRUCTURE_ENTRY_POINTS = {'dl_substructure_match': DLSubstructureArgs}
# The stereo perception (stereo.hip), likewise: tests/test_substructure_host.py pins the one above.
STEREO_ENTRY_POINTS = {'dl_stereo_perceive': DLStereoArgs}
ALL_ENTRY_POINTS = {**STRUCT_ENTRY_POINTS, **SELECT_ENTRY_POINTS, **RELAX_ENTRY_POINTS, **CANON_ENTRY_POINTS,
                    **SUBSTRUCTURE_ENTRY_POINTS, **STEREO_ENTRY_POINTS}


def entry_struct(name):
    """The args struct of a struct-taking entry point, from whichever of the tables lists it."""
    return ALL_ENTRY_POINTS[name]


def _stream_is_field(struct):
    return any(name == 'stream' for name, _ in struct._fields_)

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises ``HipLibraryError`` when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


class test_hooks:
    """Context manager for the fault-injection tests: inside it ``load()`` returns the ``-DDL_TEST_HOOKS`` build of the
    library (``dl_debug_team_fault`` and ``dl_debug_slot_order`` exist there and nowhere else).  Handles (``dl_model``) are plain structs of device
    pointers and work across the two builds, but the tests create their models inside the context anyway."""

    def __enter__(self):
        global _lib
        self.saved = _lib
        lib = _open(TEST_HOOKS_LIB_PATH)
        lib.dl_debug_team_fault.restype = None
        lib.dl_debug_team_fault.argtypes = [ctypes.c_int32]
        lib.dl_debug_slot_order.restype = ctypes.c_int32
        lib.dl_debug_slot_order.argtypes = [ctypes.c_int32]
        _lib = lib
        return lib

    def __exit__(self, *exc):
        global _lib
        _lib.dl_debug_team_fault(0)
        _lib = self.saved
        return False


def _open(path):
    if not os.path.exists(path):
        raise HipLibraryError(
            f'{path} not found: build the HIP extension first '
            '(python -c "import __graft_entry__ as g; g.build()"). There is no CPU fallback.')
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f'cannot load {path}: {e}') from e
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.dl_abi_version.restype = i32
    lib.dl_last_hip_error.restype = i32
    lib.dl_max_atoms.restype = i32
    lib.dl_error_string.restype = ctypes.c_char_p
    lib.dl_error_string.argtypes = [i32]
    lib.dl_model_num_tensors.restype = i32
    lib.dl_model_num_tensors.argtypes = [ctypes.POINTER(DLConfig)]
    lib.dl_model_create.restype = i32
    lib.dl_model_create.argtypes = [ctypes.POINTER(DLConfig), ctypes.POINTER(vp), i32, ctypes.POINTER(vp)]
    lib.dl_model_destroy.restype = None
    lib.dl_model_destroy.argtypes = [vp]
    lib.dl_egnn_forward_fc.restype = i32
    lib.dl_egnn_forward_fc.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.dl_egnn_forward_fc_team.restype = i32
    lib.dl_egnn_forward_fc_team.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, ctypes.c_size_t, vp]
    lib.dl_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_workspace_bytes.argtypes = [i32, i32]
    lib.dl_team_max.restype = i32
    lib.dl_team_max.argtypes = [i32]
    lib.dl_team_max_atoms.restype = i32
    lib.dl_team_max_atoms.argtypes = [i32]
    lib.dl_sampler_step.restype = i32
    lib.dl_sampler_step.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, DLStepCoef, vp, vp]
    lib.dl_set_profile_buffer.restype = None
    lib.dl_set_profile_buffer.argtypes = [vp]
    lib.dl_profile_max_events.restype = i32
    lib.dl_pocket_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_pocket_workspace_bytes.argtypes = [i32, i32]
    lib.dl_egnn_forward_pocket.restype = i32
    lib.dl_egnn_forward_pocket.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.dl_egnn_forward_fc_large.restype = i32
    lib.dl_egnn_forward_fc_large.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.dl_sample_chain_fc.restype = i32
    lib.dl_sample_chain_fc.argtypes = [vp, ctypes.POINTER(DLChainArgs), vp]
    lib.dl_join_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_join_workspace_bytes.argtypes = [i32]
    lib.dl_sample_chain_fc_join.restype = i32
    lib.dl_sample_chain_fc_join.argtypes = [vp, ctypes.POINTER(DLChainArgs), ctypes.POINTER(DLJoinArgs), vp]
    lib.dl_inpaint_step.restype = i32
    lib.dl_inpaint_step.argtypes = [i32, i32, i32] + [vp] * 10 + [DLInpaintCoef, vp, vp]
    lib.dl_philox_fill.restype = i32
    lib.dl_philox_fill.argtypes = [ctypes.c_uint64, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    for name, struct in ALL_ENTRY_POINTS.items():
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [ctypes.POINTER(struct)] if _stream_is_field(struct) else [ctypes.POINTER(struct), vp]
    lib.dl_edm_loss_grad.restype = i32
    lib.dl_edm_loss_grad.argtypes = [ctypes.POINTER(DLLossArgs), vp, vp, vp]
    lib.dl_egnn_backward_fc_num_params.restype = ctypes.c_int64
    lib.dl_egnn_backward_fc_num_params.argtypes = [ctypes.POINTER(DLBackwardArgs)]
    lib.dl_egnn_backward_fc_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_egnn_backward_fc_workspace_bytes.argtypes = [ctypes.POINTER(DLBackwardArgs)]
    lib.dl_egnn_backward_max_atoms.restype = i32
    lib.dl_egnn_backward_pocket_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_egnn_backward_pocket_workspace_bytes.argtypes = [ctypes.POINTER(DLBackwardArgs), i32]
    lib.dl_egnn_backward_pocket.restype = i32
    lib.dl_egnn_backward_pocket.argtypes = [ctypes.POINTER(DLBackwardArgs), i32, vp]
    lib.dl_size_train_num_params.restype = ctypes.c_int64
    lib.dl_size_train_num_params.argtypes = [ctypes.POINTER(DLSizeTrainArgs)]
    lib.dl_size_train_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_size_train_workspace_bytes.argtypes = [ctypes.POINTER(DLSizeTrainArgs)]
    lib.dl_bonds_workspace_bytes.restype = ctypes.c_size_t
    lib.dl_bonds_workspace_bytes.argtypes = [i32, i32]
    lib.dl_size_model_num_tensors.restype = i32
    lib.dl_size_model_num_tensors.argtypes = [ctypes.POINTER(DLSizeConfig)]
    lib.dl_size_model_create.restype = i32
    lib.dl_size_model_create.argtypes = [ctypes.POINTER(DLSizeConfig), ctypes.POINTER(vp), i32, ctypes.POINTER(vp)]
    lib.dl_size_model_destroy.restype = None
    lib.dl_size_model_destroy.argtypes = [vp]
    lib.dl_size_max_fragment_atoms.restype = i32
    lib.dl_size_gnn_forward.restype = i32
    lib.dl_size_gnn_forward.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


def check(status, what):
    if status != DL_OK:
        lib = load()
        msg = lib.dl_error_string(status).decode()
        raise HipLibraryError(f'{what}: {msg} (status {status}, hip error {lib.dl_last_hip_error()})')


def ptr(t):
    """Device/host pointer of a tensor (or NULL for None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def launch(name, args, device):
    """Call the entry point ``name`` of ``ALL_ENTRY_POINTS`` (the tables above) on ``args`` with ``device`` current and on torch's current
    stream of that device, handed over as the entry point takes it, and raise ``HipLibraryError`` unless it answers ``DL_OK``.
    Nothing is built, allocated or synchronised here."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if _stream_is_field(entry_struct(name)):
            args.stream = stream
            status = getattr(load(), name)(ctypes.byref(args))
        else:
            status = getattr(load(), name)(ctypes.byref(args), ctypes.c_void_p(stream))
        check(status, name)


def require_device(who, **tensors):
    """Raise ``HipLibraryError`` when one of the named tensors (``None``: not given) is not on a HIP device."""
    given = {name: t for name, t in tensors.items() if t is not None}
    if not all(t.is_cuda for t in given.values()):
        raise HipLibraryError(f'{who} runs on the HIP device only (no CPU fallback): got '
                              + ', '.join(f'{name} on {t.device}' for name, t in given.items()))


def dense(t, device, dtype):
    """``t`` as a contiguous tensor of ``dtype`` on ``device`` - what a kernel reads at its ``data_ptr()``; ``None`` stays."""
    return None if t is None else t.to(device=device, dtype=dtype).contiguous()


def empty_i32(device, *shape):
    return torch.empty(shape, dtype=torch.int32, device=device)
