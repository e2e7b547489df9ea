/*
 * difflinker_hip.h — C ABI of the MI355X (gfx950) implementation of DiffLinker's EGNN
 * denoising-diffusion sampling hot path.
 *
 * The reference (igashov/DiffLinker) is pure Python/PyTorch and has no FFI of its own; the
 * entry points below are what a native replacement of its hot path binds, one per reference
 * interface (file:line into the reference tree):
 *
 *   dl_model_create / dl_model_destroy   <- Dynamics.__init__ + load_state_dict
 *                                           src/egnn.py:324-372, src/lightning.py:81-100
 *   dl_egnn_forward_fc                   <- Dynamics.forward (FC graph)       src/egnn.py:374-447
 *                                           (EGNN.forward :218-238, EquivariantBlock :157-178,
 *                                            GCL :45-80, EquivariantUpdate :101-125,
 *                                            coord2diff :295-301, unsorted_segment_sum :304-320)
 *   dl_egnn_forward_pocket               <- DynamicsWithPockets.forward       src/egnn.py:470-552
 *                                           (+ get_dist_edges / get_dist_edges_4A :554-596)
 *   dl_sampler_step                      <- EDM.sample_p_zs_given_zt_only_linker, the part after
 *                                           the denoiser call                   src/edm.py:198-208
 *   dl_sample_chain_fc                   <- EDM.sample_chain                  src/edm.py:126-176
 *                                           (+ :178-208 reverse step, :210-242 final decode,
 *                                            :328-361 noise / (un)normalisation)
 *   dl_workspace_bytes                   <- (no reference counterpart) scratch the fully-connected entry points need
 *   dl_egnn_forward_fc_team, dl_team_max, dl_team_max_atoms
 *                                        <- the same Dynamics.forward / EDM.sample_chain with several compute
 *                                           units per molecule (batches smaller than the chip; no reference
 *                                           counterpart: a launch-geometry knob, results agree to fp32 rounding)
 *   dl_edm_loss_prologue / dl_edm_loss_epilogue
 *                                        <- EDM.forward / InpaintingEDM.forward around the denoiser call
 *                                           (src/edm.py:41-124, :467-548; the terms of :244-326): the noising of
 *                                           the data at a drawn t and the per-molecule loss / VLB terms
 *   dl_size_model_create / dl_size_gnn_forward
 *                                        <- SizeGNN (src/linker_size.py:45-91) as driven by
 *                                           SizeClassifier.forward at inference
 *                                           (src/linker_size_lightning.py:83-110): the `sample_fn`
 *                                           of generate.py:86-99 that runs once before a chain
 *   dl_perceive_bonds                    <- build_xae_molecule / get_bond_order of a whole batch
 *                                           (src/molecule_builder.py:44-102) and the fragment count behind
 *                                           metrics.is_connected
 *   dl_molecule_keys                     <- the questions metrics.py asks of a built molecule (src/metrics.py:12-54), put to
 *                                           the bond graph instead of RDKit: valences within the element's limit,
 *                                           one piece, and a renumbering-invariant key per molecule
 *   dl_best_rmsd                         <- the RMSD block of compute_metrics.py:366-402: rdMolAlign.GetBestRMS of every
 *                                           recovered sample against its true molecule, the minimum over the graph
 *                                           isomorphisms the host enumerated, proper rotations only
 *   dl_clash_scores                      <- (no reference counterpart: the paper reports clash counts of pocket samples, the
 *                                           scripts do not compute them) generated atoms against protein atoms under a
 *                                           van der Waals rule stated below, one launch per batch
 *   dl_interaction_types / dl_interaction_scores
 *                                        <- (no reference counterpart: the field answers "does it make contacts?" with an
 *                                           external docking program) heavy atoms typed as hydrophobic, donor or acceptor
 *                                           from elements and geometry, and the intermolecular terms of Trott & Olson
 *                                           (AutoDock Vina, J. Comput. Chem. 2010) between generated and protein atoms, in
 *                                           place.  The rule stated below is this project's own after that published
 *                                           form, NOT AutoDock Vina's numbers
 *   dl_shape_scores                      <- the shape half of SC-RDKit (src/delinker_utils/calc_SC_RDKit.py:36-38,
 *                                           1 - rdShapeHelpers.ShapeProtrudeDist, compute_metrics.py:404-441): the gridded
 *                                           van der Waals overlap of every sample with its true molecule.  The rule stated
 *                                           below is this project's own after RDKit's defaults, NOT RDKit's grid
 *   dl_ring_scores                       <- rings_n of compute_metrics.py:128-145 (CalcNumRings of the linker) and the ring
 *                                           perception under its ring filter (:269-298), asked of the bond graph: the
 *                                           cyclomatic number and the smallest ring through every bond.  Aromaticity, which
 *                                           the filter needs, is dl_aromatic_rings
 *   dl_aromatic_rings                    <- (no reference counterpart in its own code: the reference hands every .xyz to
 *                                           `obabel`, and check_ring_filter of compute_metrics.py:269-277 asks RDKit) planar
 *                                           five- and six-rings from the geometry, Kekule orders for them and the aromatic
 *                                           ones, under a rule stated below that is this project's own, NOT OpenBabel's or
 *                                           RDKit's
 *   dl_fingerprints                      <- (no reference counterpart: the field reports internal diversity and similarity
 *                                           to the training set over RDKit's Morgan fingerprints; the reference computes
 *                                           neither) circular fingerprints from the colour refinement of dl_molecule_keys.
 *                                           This project's own fingerprint, NOT RDKit's: stated below
 *   dl_tanimoto_nearest                  <- (no reference counterpart) for every row of one fingerprint set the most similar
 *                                           row and the summed Tanimoto similarity among a segment of another set
 *   dl_tanimoto_cluster                  <- (no reference counterpart) Taylor-Butina sphere-exclusion clusters of every group
 *                                           of a fingerprint set, in a fixed order.  This project's own statement of the rule
 *                                           on this project's fingerprint, NOT RDKit's Butina.ClusterData on ties
 *   dl_tanimoto_pick                     <- (no reference counterpart) a MaxMin diverse subset of every group of a
 *                                           fingerprint set, with this project's own tie rules, NOT RDKit's MaxMinPicker
 *   dl_pharmacophore_features            <- the feature half of SC-RDKit (src/delinker_utils/calc_SC_RDKit.py:7-25,
 *                                           BuildFeatureFactory over BaseFeatures.fdef): donors, acceptors, ionizable
 *                                           groups, hydrophobes and aromatic rings of every molecule, from the bond graph.
 *                                           The rule stated below is this project's own after that file, NOT RDKit's
 *   dl_feature_match                     <- get_FeatureMapScore of the same file (:20-30): the Best-mode feature-map match
 *                                           of every sample's features with its true molecule's, the Gaussian left to the host
 *   dl_fragment_cuts                     <- FragmentMol(minCuts = maxCuts = 2) with DeLinker's pattern
 *                                           (data/geom/generate_geom_multifrag.py:199-206) and the re-assembly of
 *                                           data/zinc/prepare_dataset.py, src/datasets.py:56-100
 *   dl_fragment_multicuts                <- fragment_by_mmpa(min_cuts=3, max_cuts=5, min_frag_size=3) on molecules of at
 *                                           most 40 atoms with three rings (data/geom/generate_geom_multifrag.py:227-231):
 *                                           one linker joined to three, four or five fragments
 *   dl_pocket_select                     <- get_pocket of data/pocket/prepare_dataset.py (residues with an atom within 6 A
 *                                           of the ligand), for every (ligand, protein) pair of a batch
 *   dl_pose_checks                       <- (no reference counterpart: the field asks PoseBusters whether a generated molecule's own
 *                                           geometry is plausible) bond lengths against the reference's typical lengths, bond
 *                                           angles against the ideal of the centre's class, and clashes between atoms four or
 *                                           more bonds apart.  The rule stated below is this project's own, NOT PoseBusters'
 *   dl_relax_molecules                   <- (no reference counterpart: the field cleans a sampled linker up with RDKit's or
 *                                           OpenBabel's force fields on the host) a restrained FIRE minimisation of the linker
 *                                           atoms in fp64 with the topology frozen.  The rule stated below is this project's
 *                                           own, NOT UFF, MMFF or either toolkit's optimiser
 *   dl_canonical_ranks                   <- the identity the reference gets from Chem.MolToSmiles (src/metrics.py:12-54, the
 *                                           strings behind its uniqueness, novelty and recovery): canonical atom ranks and
 *                                           a canonical 64-bit code by an individualisation-refinement search over the
 *                                           colours of dl_molecule_keys.  The rule stated below is this project's own, NOT
 *                                           RDKit's canonical ranks or SMILES
 *   dl_substructure_match                <- the PAINS filter of compute_metrics.py (FilterCatalog over the SMARTS of the file
 *                                           given as pains_smarts_loc) and every other "does the sample contain X": a subset
 *                                           of SMARTS compiled on the host, matched by a depth-first search per (pattern, root
 *                                           atom).  The language and the rule stated below are this project's own, NOT RDKit's
 *                                           matcher
 *   dl_stereo_perceive                   <- (no reference counterpart: the reference calls Chem.RemoveStereochemistry before
 *                                           it compares strings, src/metrics.py) tetrahedral centres and stereo double bonds
 *                                           read off the 3D sample, with labels relative to the colour classes of
 *                                           dl_canonical_ranks.  The rule stated below is this project's own, NOT RDKit's
 *                                           stereo perception and NOT CIP
 *   dl_size_train_forward / dl_size_train_backward
 *                                        <- SizeClassifier.forward in training mode + loss.backward()
 *                                           (src/linker_size_lightning.py:83-117, :163-167)
 *
 * Conventions
 *   - every pointer marked "device" is a HIP device pointer owned by the caller (PyTorch-ROCm
 *     tensors' data_ptr()); `stream` is a hipStream_t passed as void* (0 = default stream); calls are
 *     asynchronous on that stream.
 *   - the library allocates NOTHING after dl_model_create (which uploads the packed weights): every compute entry
 *     point takes its scratch memory from the caller - `workspace` / `workspace_bytes`, sized by the matching
 *     dl_*_workspace_bytes query, 16-byte aligned, free to reuse once the launch has completed on `stream`.  Two
 *     launches that run concurrently need two workspaces; a dl_model itself is immutable after creation and may be
 *     shared by any number of streams.
 *   - STREAMS AND THREADS: an entry point reads its inputs and writes its outputs and workspace in the order of `stream`
 *     alone (the memsets that clear arrival, join and flag words included), from whichever thread it is called.  Calls with
 *     distinct workspaces and outputs may be issued on any streams and threads at once, on one dl_model or several.  The
 *     Python layer is narrower: one Dynamics / EDM / SizeClassifier object caches one workspace of each kind and is used on
 *     one stream at a time (it may move to a stream that waits on the previous one); distinct objects are independent
 *     (tests/test_gpu_streams.py).
 *   - THE WORKSPACE CONTRACT (every entry point that takes `workspace`): the contents of the workspace on entry are
 *     unspecified - stale bytes of any earlier use, NaN, inf and huge integers included; the library initialises what it
 *     needs (arrival words, counters, flag words) on `stream` before the kernels that read it; the contents on return are
 *     unspecified.  The same holds for every output buffer: the defined part of every result, and every status flag, is
 *     a function of the inputs alone, bit for bit, whatever workspace and outputs held on entry.  Outputs are written in
 *     full unless their description says "up to" a returned count or "rows of real atoms" (tests/test_gpu_scratch.py
 *     runs every entry point and launch route on buffers pre-filled with NaN, inf and 3.4e38 bit patterns).
 *   - all floating point is fp32; masks are int8 (node_mask, edge_mask) or fp32 (fragment /
 *     linker masks, context) exactly as the reference's collate produces them.
 *   - return value: 0 on success, a negative dl_status otherwise; dl_error_string() names it.
 *     There is NO CPU fallback: on a machine without a gfx950 device the compute entry points
 *     return DL_ERR_NO_DEVICE / a HIP error.
 */
#ifndef DIFFLINKER_HIP_H
#define DIFFLINKER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DL_ABI_VERSION 7

typedef enum dl_status {
    DL_OK = 0,
    DL_ERR_BAD_ARG = -1,        /* null pointer / inconsistent sizes                       */
    DL_ERR_UNSUPPORTED = -2,    /* hyper-parameter outside the HIP path (see dl_config)    */
    DL_ERR_TOO_MANY_ATOMS = -3, /* a molecule has more real atoms than dl_max_atoms()      */
    DL_ERR_HIP = -4,            /* a HIP runtime call failed (see dl_last_hip_error())     */
    DL_ERR_NO_DEVICE = -5,      /* no gfx950 device visible                                */
    DL_ERR_ALLOC = -6
} dl_status;

/* Arithmetic of the 128-wide contractions (edge/node/coordinate MLP layers).  Everything else
 * (distances, SiLU, masks, aggregation, sampler algebra) is fp32 in both modes.
 *   DL_PRECISION_FP32   v_mfma_f32_32x32x2_f32: exact fp32 FMA chains (runs at the fp32 vector rate)
 *   DL_PRECISION_F16X3  each fp32 operand is scaled by a power of two into the fp16 range and split into
 *                       fp16 hi+lo (~21 significant bits); a*w = hi*hi'+hi*lo'+lo*hi' on
 *                       v_mfma_f32_32x32x16_f16 with fp32 accumulation, rescaled exactly; ~1e-6 relative
 *                       per product (fp32-class), 2x faster than the fp32 MFMA on this workload
 *   DL_PRECISION_F16X2  (round 4, opt-in) F16X3 everywhere except the second layer of the GCL edge model (src/egnn.py:19-30,45-59),
 *                       where the first layer's activation enters as ONE fp16 rounded to nearest: a_rn*(hi'+lo'), 64 instead of
 *                       96 MFMAs per 32 pairs and no lo split (+9..11 % molecules/s).  Measured against the fp32 oracle: node
 *                       features 3e-6..9e-6 rel-L2 per forward (F16X3: 2e-7..5e-7), velocities and sampled coordinates
 *                       unchanged (<= 1e-6; the coordinate model stays F16X3) - inside the 1e-4 bar, outside fp32 class       */
typedef enum dl_precision { DL_PRECISION_FP32 = 0, DL_PRECISION_F16X3 = 1, DL_PRECISION_F16X2 = 2 } dl_precision;

/* Dynamics.__init__ hyper-parameters (src/egnn.py:324-329).  The HIP path implements model='egnn_dynamics' with SiLU on 128-wide
 * kernels: the released-config surface plus the optional attention, tanh, aggregation_method='mean' (every kernel family),
 * sin_embedding (HBM-resident kernels), 1..4 GCLs per block and an optional time feature (ABI v7).  A narrower network
 * (hidden_nf < 128; the reference's default is 64) is handed over ZERO-PADDED to 128 - the extra hidden features get zero weights
 * in and out and zero biases (SiLU(0) = 0): exactly the same function; difflinker_amd/egnn.py: pad_to_kernel_width does it. */
typedef struct dl_config {
    int32_t n_dims;               /* 3                                              */
    int32_t in_node_nf;           /* atom-type channels nf (8 ZINC, 9 GEOM/pockets) */
    int32_t context_node_nf;      /* 1..4                                           */
    int32_t hidden_nf;            /* must be 128 (narrower networks: zero-padded, above) */
    int32_t n_layers;             /* EquivariantBlocks (6 GEOM, 8 ZINC)             */
    int32_t inv_sublayers;        /* GCLs per EquivariantBlock, 1..4 (2 in every released configuration) */
    int32_t condition_time;       /* 1: the node inputs are [h, t, context] (released configurations); 0: [h, context] */
    float norm_constant;          /* 1e-6 in the released configs                   */
    float normalization_factor;   /* 100                                            */
    int32_t precision;            /* dl_precision: arithmetic of the 128-wide GEMMs */
    /* optional hyper-parameters of the reference no released configuration uses (every entry point carries them; round 3:
     * dl_egnn_forward_pocket and dl_egnn_forward_fc_large too): */
    int32_t attention;            /* GCL edge attention: m_ij *= sigmoid(w_att . m_ij + b_att)   src/egnn.py:42-43,52-54  */
    int32_t tanh;                 /* coordinate head: cdiff * tanh(s) * coords_range             src/egnn.py:104-105      */
    float coords_range;           /* 15 for Dynamics (EGNN hands its undivided default to the blocks, src/egnn.py:183,213) */
    int32_t aggregation_mean;     /* 0: sum / normalization_factor; 1: / number of edges of the row, masked ones included
                                   * (= the padded width N on the fully-connected graph, the atom's degree on a radius
                                   * graph)                                                        src/egnn.py:315-319      */
    int32_t sin_embedding;        /* 1: 24 sinusoidal edge attributes (src/egnn.py:281-292); the weights' edge-MLP input rows are
                                   * then [128][280].  HBM-resident entry points only (dl_egnn_forward_fc_large,
                                   * dl_egnn_forward_pocket); the LDS-resident ones answer DL_ERR_UNSUPPORTED               */
} dl_config;

typedef struct dl_model dl_model; /* opaque: packed, pre-scaled weights resident in HBM */

/* Number of weight tensors dl_model_create expects: 4 + n_layers * (inv_sublayers*(8 + 2*attention) + 5); with attention every GCL
 * appends att_mlp.0.weight [1,128] and att_mlp.0.bias [1] after its node_mlp tensors. */
int32_t dl_model_num_tensors(const dl_config* cfg);

/* Pack the reference's nn.Linear tensors ([out,in] row-major fp32, HOST pointers) into the
 * kernel layout and upload them.  `weights` lists the tensors in the reference state_dict
 * order of the `Dynamics.dynamics` (EGNN) module:
 *   embedding.weight, embedding.bias, embedding_out.weight, embedding_out.bias, then per block i:
 *   gcl_0.edge_mlp.0.{weight,bias}, gcl_0.edge_mlp.2.{weight,bias}, gcl_0.node_mlp.0.{weight,bias},
 *   gcl_0.node_mlp.2.{weight,bias}, (same for gcl_1 .. gcl_{inv_sublayers-1}),
 *   gcl_equiv.coord_mlp.0.{weight,bias}, gcl_equiv.coord_mlp.2.{weight,bias}, gcl_equiv.coord_mlp.4.weight */
int32_t dl_model_create(const dl_config* cfg, const float* const* weights, int32_t n_tensors, dl_model** out);
void dl_model_destroy(dl_model* m);

/* Largest number of REAL atoms per molecule the LDS-resident fully-connected kernels take with ONE workgroup per molecule
 * (a team of workgroups: dl_team_max_atoms). */
int32_t dl_max_atoms(void);

/* Dynamics.forward, fully-connected graph (src/egnn.py:374-447).
 *   xh          device [B,N,3+nf]   noisy state z_t (masked by node_mask inside, like the reference)
 *   t           device [B] (t_is_scalar=0) or [1] (t_is_scalar=1, the numel==1 branch :397-399)
 *   node_mask   device int8 [B,N]
 *   linker_mask device f32 [B,N] or NULL (NULL = no masking of the coordinate update, :113-114); the coordinate head
 *               (EquivariantUpdate, :101-125) is evaluated only for receiving atoms with linker_mask != 0: the
 *               reference multiplies every other atom's sum by zero (:113-116), so the outputs are the same
 *   edge_mask   device int8 [B,N,N] ({0,-1,-2} from collate; multiplies every message as-is) or NULL
 *               contract: edge_mask must be 0 wherever an endpoint has node_mask 0 (datasets.py:366-369).  A zero byte
 *               BETWEEN TWO REAL ATOMS (collate never writes one: every real pair is -1, the diagonal -2) removes that
 *               message like the reference's `* edge_mask` does, exactly in DL_PRECISION_FP32 and in the coordinate head of
 *               every mode; the f16 modes' GCL messages fold the mask into the SiLU reciprocal and apply such a byte as a
 *               factor 2^-100 instead of 0 - below one ulp of any fp32 sum while the message's pre-activation stays under
 *               the f16-range limit of bit4 below (2^75): not observable, but not bit-zero either
 *   context     device f32 [B,N,ctx] or NULL when ctx == 0
 *   out         device [B,N,3+nf]   eps_hat = cat[vel, h_final]; padded rows are written as 0
 *   nan_flags   device int32 [B]    bit0: NaN in vel, bit1: NaN in h_final, bit2: too many atoms
 *                                   (the caller raises FoundNaNException, src/egnn.py:441-442);
 *                                   bit4 (f16 modes only, always with bit0 | bit1): a magnitude bound of this molecule's
 *                                   activations reached 2^75 (3.8e22) - beyond the scales' range the fp16 operands would
 *                                   saturate silently, so `out` is void; DL_PRECISION_FP32 has no such limit.  The radius-graph
 *                                   kernels scale per tile, and a tile belongs to one molecule: they too report that molecule alone */
int32_t dl_egnn_forward_fc(const dl_model* m, int32_t B, int32_t N,
                           const float* xh, const float* t, int32_t t_is_scalar,
                           const int8_t* node_mask, const float* linker_mask, const int8_t* edge_mask,
                           const float* context, float* out, int32_t* nan_flags,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Scratch of dl_egnn_forward_fc / dl_egnn_forward_fc_team / dl_sample_chain_fc for a batch of B molecules with `team`
 * compute units per molecule (0 or 1: one): per workgroup the node features and the pre-computed half of the node MLP that
 * cross the O(n^2) edge passes through L2 (124 KB: the T0 and residual tiles in accumulator order, the h fragment rows of a
 * 56..110-atom molecule across a coordinate pass), plus, for team > 1, the exchange buffers (116 KB per molecule) and arrival words.
 * Contents on entry unspecified (the entry points zero the arrival words on `stream`; the tile columns of padding atoms are
 * never written and never read for a result), contents on return unspecified.  `out` and `nan_flags` are written in full. */
size_t dl_workspace_bytes(int32_t B, int32_t team);

/* DynamicsWithPockets.forward (src/egnn.py:470-552): radius graph rebuilt on the GPU every call
 * (ligand-ligand fully connected, pocket-pocket <= 4 A, ligand-pocket <= 10 A [4 A for 'FC-4A'], everything
 * <= 4 A for '4A'; no self loops; :554-596), EGNN with edge_mask = None.
 *   graph_type  0: '4A', 1: 'FC-4A', 2: 'FC-10A-4A'
 *   linker_mask device f32 [B,N] (required: it defines the ligand atoms together with context[..., -2])
 *   context     device f32 [B,N,ctx], last two channels = fragment-only / pocket-only masks (:486-487)
 *   workspace   device scratch of at least dl_pocket_workspace_bytes(B, N) bytes, caller-owned; contents on entry
 *               unspecified (the entry point zeroes its counters and batch-wide maxima on `stream`), contents on return
 *               unspecified.  `out` (padded rows 0) and `nan_flags` are written in full
 * Molecule membership is positional (atom v belongs to molecule v / N), which is what the reference's batch-index
 * "edge_mask" vector encodes (src/datasets.py:359-364).  Both precisions are supported.
 * The rows of molecule b in `out` and nan_flags[b] are a function of molecule b's inputs and N alone, bit for bit: not of B, of
 * the molecule's position in the batch or of the other molecules (edge and row tiles are cut per molecule; the workspace holds
 * up to 3 padding quads of 8 edge slots per molecule for it).  The same holds for dl_egnn_forward_fc_large. */
size_t dl_pocket_workspace_bytes(int32_t B, int32_t N);
int32_t dl_egnn_forward_pocket(const dl_model* m, int32_t B, int32_t N, int32_t graph_type,
                               const float* xh, const float* t, int32_t t_is_scalar,
                               const int8_t* node_mask, const float* linker_mask, const float* context,
                               float* out, int32_t* nan_flags, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Dynamics.forward (src/egnn.py:374-447) for fully-connected graphs of ANY size: the HBM-resident per-pass kernels of
 * the pocket path run on the reference's own dense edge list — every pair whose int8 edge_mask value is non-zero, the
 * diagonal included (value -2, src/datasets.py:366-369), each message weighted by that value.  Use it for batches with a
 * molecule of more than dl_max_atoms() atoms (dl_egnn_forward_fc flags those with bit 2); several times slower than
 * the LDS-resident kernel.  Arguments as dl_egnn_forward_fc (edge_mask required, linker_mask may be NULL);
 * workspace: dl_pocket_workspace_bytes(B, N), contents on entry and on return unspecified (initialised on `stream` as in
 * dl_egnn_forward_pocket); `out` and `nan_flags` are written in full. */
int32_t dl_egnn_forward_fc_large(const dl_model* m, int32_t B, int32_t N, const float* xh, const float* t,
                                 int32_t t_is_scalar, const int8_t* node_mask, const float* linker_mask,
                                 const int8_t* edge_mask, const float* context, float* out, int32_t* nan_flags,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Per-step scalars of the reverse process, computed by the host exactly as the reference does
 * (src/edm.py:180-185,199,202): one row per reverse step, in execution order (s = T-1 ... 0). */
typedef struct dl_step_coef {
    float t;            /* time feature (s+1)/T fed to the denoiser        */
    float alpha_ts;     /* alpha_{t|s}                                      */
    float c_eps;        /* sigma2_{t|s} / alpha_{t|s} / sigma_t             */
    float sigma;        /* sigma_{t|s} * sigma_s / sigma_t                  */
} dl_step_coef;

/* Fused tail of sample_p_zs_given_zt_only_linker (src/edm.py:196-206):
 *   z_s = z_t*frag + ((z_t/alpha_ts - c_eps*(eps_hat*lm)) + sigma*(noise*lm)) * lm
 * z_t, eps_hat, noise, z_s: device [B,N,D]; fragment_mask/linker_mask: device f32 [B,N]. */
int32_t dl_sampler_step(int32_t B, int32_t N, int32_t D, const float* z_t, const float* eps_hat,
                        const float* noise, const float* fragment_mask, const float* linker_mask,
                        dl_step_coef coef, float* z_s, void* stream);

/* EDM.sample_chain (src/edm.py:126-176) as ONE launch: every molecule runs its T reverse steps
 * and the final decode on one compute unit with its state resident in LDS. */
typedef struct dl_chain_args {
    int32_t B, N, T, keep_frames;
    const float* x;             /* device [B,N,3]   fragment-centred coordinates               */
    const float* h;             /* device [B,N,nf]  one-hot atom types (un-normalised)         */
    const int8_t* node_mask;    /* device [B,N]                                                */
    const float* fragment_mask; /* device [B,N]                                                */
    const float* linker_mask;   /* device [B,N]                                                */
    const int8_t* edge_mask;    /* device [B,N,N]                                              */
    const float* context;       /* device [B,N,ctx]                                            */
    const float* noise_x;       /* device [T+2,B,N,3]  standard normal draws, reference order: */
    const float* noise_h;       /* device [T+2,B,N,nf] draw 0 = initial z, 1..T = steps, T+1 = decode */
                                /* both NULL: the draws are generated inside the kernel (dl_philox_fill's stream) */
    uint64_t noise_seed;        /* key of the in-kernel generator                                          */
    int32_t mol_offset;         /* global index of molecule 0 of this batch (shards of one logical batch)  */
    int32_t team;               /* compute units per molecule: 0 or 1 = one (default); 2, 4 or 8 = a team, see below */
    const dl_step_coef* coefs;  /* device [T]       execution order (s = T-1 first)            */
    float inv_alpha0, sigma0, sigma_x;      /* final decode scalars (src/edm.py:213-216,237-242) */
    float norm_x, norm_h, bias_h;           /* norm_values[0], norm_values[1], norm_biases[1]    */
    float* chain;               /* device [keep_frames,B,N,3+nf]; frame 0 = final [x, one_hot(h)].  The rows of REAL atoms are
                                 * written; padding rows (and the frames of a molecule that ended flagged) stay as the caller
                                 * left them - EDM.sample_chain passes zeros */
    int32_t* nan_flags;         /* device [B]  bit0/bit1 as above (first offending forward only) */
    int32_t* nan_step;          /* device [B]  forward index (0..T) at which the flag was raised, or -1 */
    const int32_t* order;       /* device [B] or NULL: workgroup k samples molecule order[k].  One molecule occupies one
                                 * compute unit for the whole chain and workgroups are dispatched in index order, so a
                                 * batch larger than the chip finishes sooner when the big molecules go first
                                 * (longest-processing-time order); results are written at the molecule's own index. */
    void* workspace;            /* device scratch of dl_workspace_bytes(B, team) bytes, 16-byte aligned; contents on entry
                                 * unspecified (arrival words zeroed on `stream` by the entry point), on return unspecified.
                                 * nan_flags and nan_step are written for every molecule of the launch; z_state for those that stop early */
    size_t workspace_bytes;
    const int32_t* mol_index;   /* device [B] or NULL: entry b of this batch is molecule mol_offset + mol_index[b] of the
                                 * logical batch (NULL: mol_offset + b) - the key of the in-kernel noise; lets a caller
                                 * sample a non-contiguous part of a batch (e.g. only the molecules that fit this kernel) */
    int32_t order_first, order_count;   /* (ABI v7) this launch samples the molecules order[order_first .. order_first + order_count)
                                 * only (order_count = 0: all B; otherwise `order` must be given): every array keeps the extent
                                 * and the indexing of the whole batch, the workspace is sized for order_count molecules.  Lets a
                                 * caller put the few molecules beyond one-per-compute-unit on TEAMS in a second launch on another
                                 * stream - they take the compute units the smallest molecules of the first launch leave early -
                                 * instead of waiting for a whole second round (EDM.sample_chain, batches of 257..320 on 256 CUs) */
    /* (ABI v7) a chain in TWO launches - the static hand-over of compute units inside a ragged batch: molecule b runs the denoiser
     * calls q_begin[b] .. q_end[b]-1 of the T+1 (NULL: 0 / T+1).  A launch that stops a molecule early (q_end[b] <= T) writes its
     * state z (normalised, fp32, exactly as the kernel holds it) to z_state[b]; a launch that resumes one (q_begin[b] > 0) starts
     * from there instead of from x, h and draw 0.  The noise is a function of (molecule, atom, draw) - resuming needs no generator
     * state; frames are written by step index, frame 0 by the launch that runs the decode.  skip_flags (NULL or device [B]): a
     * molecule with a non-zero word is left alone (it ended - NaN - in the first launch).  EDM.sample_chain: the small molecules
     * of a batch finish in the first launch, the big ones stop where the small ones end and finish on TEAMS OF TWO in the second,
     * which uses the compute units the small ones left. */
    const int32_t* q_begin;
    const int32_t* q_end;
    float* z_state;             /* device [B,N,3+nf]; required when q_begin or q_end is given */
    const int32_t* skip_flags;
} dl_chain_args;

int32_t dl_sample_chain_fc(const dl_model* m, const dl_chain_args* args, void* stream);

/* The hand-over of a ragged batch inside ONE launch (additive to ABI v7: dl_chain_args is unchanged).  Every molecule b of the
 * batch (B <= compute units; workgroup k samples order[k], or k) starts on its own compute unit.  A molecule with
 * args->q_end[b] <= T is an OWNER: after q_end[b] denoiser calls it leaves its state in z_state and finishes the chain on a
 * team of two with a HELPER - a molecule whose own chain (q_end = T+1) is over, a NaN included - that joins it there; the
 * others run their whole chain alone.  team_of [B]: the team a molecule owns or helps, or -1; team_mol [teams]: the owner
 * molecule of each team (each team has exactly one owner and one helper).  A team molecule gets exactly the numbers of the
 * two-launch hand-over at the same q_end (dl_sample_chain_fc twice, team = 2 for the second); every other molecule those of
 * the single launch.  An owner that ends in a NaN before its switch call releases its helper.  Owner and helper wait for each
 * other for at most 20 s; a member that gives up sets nan_flags bit 3 on the team's molecule (as a team that does not assemble).
 * args: team 0 or 1, q_end and z_state given, q_begin / skip_flags NULL, order_first = order_count = 0, workspace of
 * dl_workspace_bytes(B, 1).  The launch is cooperative.  wait_ticks (device [teams][2] or NULL): how long the owner / the
 * helper of each team waited for the other, in ticks of the 100 MHz wall clock (diagnostics). */
typedef struct dl_join_args {
    int32_t teams;
    const int32_t* team_of;     /* device [B]                                            */
    const int32_t* team_mol;    /* device [teams]                                        */
    void* workspace;            /* device scratch of dl_join_workspace_bytes(teams) bytes, 16-byte aligned; contents on entry
                                 * unspecified (arrival and join words zeroed on `stream` by the entry point), on return
                                 * unspecified - as those of args->workspace */
    size_t workspace_bytes;
    uint64_t* wait_ticks;       /* device [teams][2] or NULL                             */
} dl_join_args;

size_t dl_join_workspace_bytes(int32_t teams);
int32_t dl_sample_chain_fc_join(const dl_model* m, const dl_chain_args* args, const dl_join_args* join, void* stream);

/* Teams.  A batch smaller than the chip leaves compute units idle when every molecule sits on one of them (the reference's
 * default sampling batch is 64, generate.py:145), and a molecule of more than dl_max_atoms() atoms does not fit one compute
 * unit's LDS at all.  With team = 2, 4 or 8 that many workgroups share a molecule: its atoms are dealt round-robin, a member
 * keeps the state of its own atoms only and runs the per-atom phases (node MLP, projections, sampler algebra) for them alone;
 * its O(n^2) pair loops take its own atoms as receivers and every atom as sender, for which the members exchange the sender
 * rows and coordinates of their atoms once per pass through the workspace (release / acquire hand-off inside the launch,
 * placement-independent).  A team takes molecules of up to dl_team_max_atoms(team) = 110 atoms.
 * All team * ceil(B / 8) * 8 workgroups must be resident at once: dl_team_max(B) is the largest team the current device
 * holds for a batch of B (1, 2, 4 or 8), a larger request returns DL_ERR_BAD_ARG, and the launch is cooperative (the runtime
 * rejects a grid the device cannot hold).  Results agree with team = 1 to fp32 rounding (the order in which an atom's
 * messages are summed depends on the team size) and are bitwise repeatable for a given team size.
 * nan_flags bit 3: the members of a team did not all show up within the spin limit (another kernel held compute units for
 * seconds); every member gives up together, the sample is void and the caller re-runs the batch with team = 1 (or
 * dl_egnn_forward_fc_large).  With team > 1 the entry points zero nan_flags (and set nan_step to -1) on `stream` themselves. */
int32_t dl_team_max(int32_t B);
int32_t dl_team_max_atoms(int32_t team);
#ifdef DL_TEST_HOOKS
/* TEST BUILDS ONLY (-DDL_TEST_HOOKS: difflinker_amd/libdifflinker_hip_testhooks.so, built beside the product library and loaded
 * by the fault-injection tests alone; the product library does not export it).  Member 1 of every team of the NEXT `launches`
 * team launches gives up at its first exchange (exercises the fail-together path above); the count runs down by itself - the
 * switch cannot stay on by accident - and 0 clears it */
void dl_debug_team_fault(int32_t launches);
/* receiver_major != 0: the pair loops of every later launch number their slots receiver by receiver again, as they did before the
 * short last chunks were gathered into the last waves (csrc/slot_order.h) - the order the tests compare the product's bit for
 * bit with; 0 restores the product's order.  Synchronises the device; stays as set until it is called again */
int32_t dl_debug_slot_order(int32_t receiver_major);
#endif
/* dl_egnn_forward_fc with a team per molecule (team = 1: identical to dl_egnn_forward_fc) */
int32_t dl_egnn_forward_fc_team(const dl_model* m, int32_t B, int32_t N, const float* xh, const float* t,
                                int32_t t_is_scalar, const int8_t* node_mask, const float* linker_mask,
                                const int8_t* edge_mask, const float* context, float* out, int32_t* nan_flags,
                                int32_t team, void* workspace, size_t workspace_bytes, void* stream);

/* One step of InpaintingEDM.sample_chain after the denoiser call (src/edm.py:568-596), or its final decode
 * (:599-610, :674-713), for one batch: the linker atoms take the p(z_s|z_t) sample, the fragment atoms are re-drawn from
 * q(z_s|z_t,x), the position noise is centre-of-gravity free (utils.py:158-168), the denoiser's velocity is centred
 * (egnn.py:444-445) and the centre of gravity of z_s is projected out. */
typedef struct dl_inpaint_coef {
    float alpha_ts, c_eps, sigma;           /* p: mu = z/alpha_ts - c_eps*eps_hat;  sigma of both draws   */
    float a_q, b_q;                         /* q: mu = a_q*z + b_q*(xh*fragment_mask)                     */
    int32_t decode;                         /* 0: reverse step, 1: final decode                           */
    float inv_alpha0, sigma0, sigma_x;      /* decode scalars                                             */
    float norm_x, norm_h, bias_h;           /* decode: un-normalisation, then one-hot of the features     */
} dl_inpaint_coef;
/*   z_t, eps_hat, xh_frag, z_s  device f32 [B,N,3+nf]   (eps_hat: raw denoiser output, centred here)
 *   noise_p*, noise_q*          device f32 [B,N,3] / [B,N,nf]: the four torch.randn draws of the step, unmasked
 *   node_mask, fragment_mask, linker_mask  device f32 [B,N] */
int32_t dl_inpaint_step(int32_t B, int32_t N, int32_t nf, const float* z_t, const float* eps_hat, const float* xh_frag,
                        const float* noise_px, const float* noise_ph, const float* noise_qx, const float* noise_qh,
                        const float* node_mask, const float* fragment_mask, const float* linker_mask,
                        dl_inpaint_coef coef, float* z_s, void* stream);

/* The in-kernel noise stream as a bank (for host-driven loops and tests): Philox4x32-10, key = seed, counter =
 * (mol_offset + m(b), atom position n, draw0 + k, component / 4) with m(b) = mol_index[b] (device int32 [B]) or b when mol_index
 * is NULL - the same keying as dl_chain_args.mol_offset / mol_index, so a part of a batch gets exactly its own rows;
 * four outputs -> four standard normals by Box-Muller; component d < 3 is noise_x[k][b][n][d], d >= 3 is noise_h[k][b][n][d-3].
 * Independent of the batch split. */
int32_t dl_philox_fill(uint64_t seed, int32_t mol_offset, const int32_t* mol_index, int32_t B, int32_t N, int32_t nf, int32_t draw0,
                       int32_t n_draws, float* noise_x, float* noise_h, void* stream);

/* ---- loss / VLB of held-out data (EDM.forward; edm_loss.hip) ------------------------------------------
 * Two launches around the unchanged denoiser forward (one workgroup per molecule each):
 *   dl_edm_loss_prologue  t_int (read, or drawn), t = t_int / T, (gamma_t, gamma_s) from the schedule's table, eps (read, or
 *                         drawn) and z_t;
 *   dl_edm_loss_epilogue  one row of DL_LOSS_ROW floats per molecule from xh, z_t, eps (read, or drawn again) and eps_hat.
 * In-kernel draws (noise_x = noise_h = NULL, t_given = 0): Philox4x32-10, key = noise_seed, counter = (mol_offset + b, atom,
 * draw word, component / 4) with draw word 0x80000000 for eps (components as in dl_philox_fill) and 0x80000001 for t_int
 * (atom 0, component 0: t_int = mulhi(r[0], T + 1), uniform on 0 .. T) - disjoint from every draw of a sampling chain.
 * Deterministic: fixed reduction order, no atomics. */
#define DL_LOSS_ROW 8               /* error_t, |eps_hat|_F, kl_prior, log p(x|z0) w/o constants, log p(h|z0), log constant
                                       of p(x|z0), SNR(gamma_s - gamma_t) - 1, atoms under the noise mask */
typedef struct dl_loss_args {
    int32_t B, N, nf;
    int32_t T;                      /* EDM.T: t = t_int / T */
    int32_t timesteps;              /* the table has timesteps + 1 entries: gamma(t) = table[round(t * timesteps)] */
    int32_t inpainting;             /* 0: EDM (noise on linker_mask, fragments kept); 1: InpaintingEDM (noise on node_mask,
                                       centre of gravity of the x-noise removed, eps_hat unmasked) */
    const float* xh;                /* device f32 [B,N,3+nf]: normalised x, h */
    const float* node_mask;         /* device f32 [B,N] */
    const float* fragment_mask;     /* device f32 [B,N] (may be NULL for inpainting) */
    const float* linker_mask;       /* device f32 [B,N] (may be NULL for inpainting) */
    const float* gamma_table;       /* device f32 [timesteps + 1] */
    const float* noise_x;           /* device f32 [B,N,3], unmasked, or NULL (drawn) */
    const float* noise_h;           /* device f32 [B,N,nf], unmasked, or NULL (drawn); NULL exactly when noise_x is */
    uint64_t noise_seed;
    int32_t mol_offset;             /* global index of molecule 0 (a shard of a batch) */
    int32_t t_given;                /* 1: t_int is read; 0: it is drawn and written */
    int32_t* t_int;                 /* device int32 [B] */
    float* t;                       /* device f32 [B] out (prologue): the denoiser's t */
    float* gamma;                   /* device f32 [B,2] out (prologue), in (epilogue): gamma_t, gamma_s */
    float* z_t;                     /* device f32 [B,N,3+nf] out (prologue), in (epilogue) */
    const float* eps_hat;           /* device f32 [B,N,3+nf] (epilogue): the raw denoiser output */
    float norm_h, bias_h;           /* norm_values[1], norm_biases[1] */
    const float* prior;             /* device f32 [B,3] (epilogue): alpha_T, sigma_T, log(1 / sigma_T) of gamma(1) per molecule,
                                       evaluated by the caller as the reference evaluates them (the KL prior cancels to a few
                                       ulp of these per entry, so they are inputs rather than kernel-side transcendentals) */
    float* rows;                    /* device f32 [B,DL_LOSS_ROW] out (epilogue) */
} dl_loss_args;
int32_t dl_edm_loss_prologue(const dl_loss_args* args, void* stream);
int32_t dl_edm_loss_epilogue(const dl_loss_args* args, void* stream);

/* d eps_hat of the loss terms (training; edm_loss.hip): for molecule b, atom i, component c, with m the noise mask,
 * lm the linker mask (1 for inpainting), eh = eps_hat lm and d = eps - eh (eps read or drawn again as in the epilogue),
 *   d_eps_hat = lm (-2 d w_err + eh w_noise / |eh|_F + [c < 3] d w_logpx)
 * where (w_err, w_noise, w_logpx) = weights[b] are the upstream gradients of error_t, |eps_hat|_F and log p(x | z_0) (the
 * row of dl_edm_loss_epilogue, whose |eps_hat|_F it reads from `rows`).  A zero w_noise adds nothing. */
int32_t dl_edm_loss_grad(const dl_loss_args* args, const float* weights /* device f32 [B,3] */, float* d_eps_hat /* [B,N,3+nf] */,
                         void* stream);

/* ---- backward of the fully-connected denoiser (training; egnn_backward.hip) -------------------------------
 * Gradient of sum(grad_out * Dynamics.forward(...)) with respect to every parameter of a fully-connected Dynamics
 * (egnn_dynamics, hidden_nf = 128, SiLU, sum aggregation, no attention / tanh / sin_embedding; any n_layers, inv_sublayers
 * 1..4, context width, norm_constant, normalization_factor, condition_time; centering = the velocity's mean removal of
 * InpaintingEDM).  Parameters and gradient are ONE flat fp32 buffer each, in Dynamics.parameters() order (the raw, unpadded
 * tensors of the state_dict; n_params must be dl_egnn_backward_fc_num_params).  The forward is recomputed in fp32 inside
 * (x, h of every sublayer saved to the workspace, pair activations recomputed per tile, never stored).  Deterministic: per
 * molecule partial gradients in the workspace, summed over molecules in a fixed order; no atomics.  The callee allocates
 * nothing; argument checks (DL_ERR_BAD_ARG, DL_ERR_UNSUPPORTED) come before any device work; runs on `stream`. */
typedef struct dl_backward_args {
    int32_t B, N;
    int32_t in_node_nf, context_node_nf, condition_time, hidden_nf, n_layers, inv_sublayers;
    int32_t centering;              /* 1: d eps_hat passes through the velocity's mean removal (InpaintingEDM) */
    float norm_constant, normalization_factor;
    const float* params;            /* device f32 [n_params] */
    int64_t n_params;
    const float* xh;                /* device f32 [B,N,3+nf]: the denoiser's input z_t */
    const float* t;                 /* device f32 [B] or [1] (t_is_scalar) */
    int32_t t_is_scalar;
    const float* node_mask;         /* device f32 [B,N] */
    const float* linker_mask;       /* device f32 [B,N] or NULL */
    const int8_t* edge_mask;        /* device int8 [B,N,N] as collate builds it (0 / -1 / -2, multiplied as-is) */
    const float* context;           /* device f32 [B,N,context_node_nf] or NULL */
    const float* grad_out;          /* device f32 [B,N,3+nf]: d eps_hat */
    float* grad_params;             /* device f32 [n_params] out */
    void* workspace;                /* device, >= dl_egnn_backward_fc_workspace_bytes; contents on entry unspecified (every saved
                                     * activation and per-molecule partial is written before it is read, nothing accumulates
                                     * across calls), on return unspecified; grad_params is written in full */
    size_t workspace_bytes;
} dl_backward_args;
int64_t dl_egnn_backward_fc_num_params(const dl_backward_args* args);          /* -1 outside the scope */
size_t dl_egnn_backward_fc_workspace_bytes(const dl_backward_args* args);      /* reads B, N and the hyper-parameters; 0 outside */
int32_t dl_egnn_backward_max_atoms(void);
int32_t dl_egnn_backward_fc(const dl_backward_args* args, void* stream);

/* ---- backward of the pocket-conditioned denoiser (training; egnn_backward_sparse.hip) --------------------------
 * Gradient of sum(grad_out * DynamicsWithPockets.forward(...)) with respect to every parameter, on the radius graph of
 * dl_egnn_forward_pocket (`graph_type` 0: '4A', 1: 'FC-4A', 2: 'FC-10A-4A'; the EGNN runs without an edge mask).  Same
 * hyper-parameter scope, the same dl_backward_args and the same flat parameter layout as dl_egnn_backward_fc
 * (dl_egnn_backward_fc_num_params answers for it), with these differences: `edge_mask` is ignored and may be NULL;
 * `context` is required (context_node_nf >= 2) and its last two channels are the fragment-only and pocket-only masks;
 * membership is positional (atom v belongs to molecule v / N).  The graph is rebuilt on the GPU from the masked coordinates
 * of `xh` by the rule and the fp32 arithmetic of dl_egnn_forward_pocket, so it is the forward's edge set; the distance test
 * carries no gradient.  All pair work follows the edge list in tiles of 32 edges spread over the chip; the pair GEMMs run on
 * v_mfma_f32_32x32x2_f32 with fp32 accumulation.  Deterministic: no float atomics; node gradients are summed receiver-side
 * over the neighbour lists, weight gradients through per-workgroup partials summed in a fixed order; a molecule's part of
 * the gradient depends on that molecule alone.  An atom without neighbours and an empty molecule are legal.
 * Limits: N <= 2048 padded atoms per molecule and B * N * N < 2^31; beyond them DL_ERR_TOO_MANY_ATOMS (workspace_bytes: 0).
 * The workspace holds per-edge buffers sized for B * N * (N - 1) edges (520 bytes each) of which only the graph's edges are
 * touched; its contents on entry are unspecified, grad_params is written in full.  The callee allocates nothing; argument
 * checks (DL_ERR_BAD_ARG, DL_ERR_UNSUPPORTED, DL_ERR_TOO_MANY_ATOMS) come before any device work; B == 0 returns DL_OK
 * without a launch; runs on `stream`. */
size_t dl_egnn_backward_pocket_workspace_bytes(const dl_backward_args* args, int32_t graph_type);   /* 0 outside the scope */
int32_t dl_egnn_backward_pocket(const dl_backward_args* args, int32_t graph_type, void* stream);

/* Diagnostics (libraries built with -DDL_PROFILE only; dl_profile_max_events() returns 0 otherwise): when set
 * (device uint64 [8 waves][dl_profile_max_events()][2], or NULL to disable), the first workgroup of the next
 * launches logs (phase tag, shader clock) pairs of its first forward. */
void dl_set_profile_buffer(void* device_buf);
int32_t dl_profile_max_events(void);

/* ---- linker-size predictor -------------------------------------------------------------------------
 * SizeGNN hyper-parameters (src/linker_size.py:46); hidden_nf must be 128.  nn.BatchNorm1d
 * (normalization='batch_norm') is an affine map in eval mode: the caller folds it into the adjacent
 * Linear before handing the tensors over. */
typedef struct dl_size_config {
    int32_t in_node_nf;
    int32_t hidden_nf;
    int32_t out_node_nf;
    int32_t n_layers;
} dl_size_config;

typedef struct dl_size_model dl_size_model;

/* tensors (host fp32, nn.Linear [out,in] row-major), 4 + 8 * n_layers of them:
 *   embedding_in.weight, .bias,
 *   per GCL (gcl1, gcl_layers.0, ...): edge_mlp.0.weight [128,257], .bias, edge_mlp.2.weight, .bias,
 *                                      node_mlp.0.weight [128,256], .bias, node_mlp.<last>.weight, .bias,
 *   embedding_out.weight [out,128], .bias */
int32_t dl_size_model_num_tensors(const dl_size_config* cfg);
int32_t dl_size_model_create(const dl_size_config* cfg, const void* const* tensors, int32_t n_tensors,
                             dl_size_model** out);
void dl_size_model_destroy(dl_size_model* m);
int32_t dl_size_max_fragment_atoms(void);

/* logits[b] = mean over the N padded nodes of embedding_out(GCL^n(embedding_in(one_hot * fragment_mask)))
 *   one_hot        device f32 [B,N,in_node_nf]
 *   positions      device f32 [B,N,3]   (may be NULL when `distances` is given)
 *   fragment_mask  device f32 [B,N]     node mask of the GNN (fragment atoms; 'fragment_only_mask' with pockets)
 *   edge_mask      device f32 [B,N,N]   e = b*N*N + i*N + j; an edge is kept where edge_mask != 0 and, when
 *                                       `distances` is NULL, the squared distance |x_i - x_j|^2 < 6
 *                                       (src/linker_size_lightning.py:106-107: coord2diff returns the SQUARED
 *                                       distance and that is what is compared with 6 and fed to the edge MLP)
 *   distances      device f32 [B,N,N] or NULL: precomputed edge attribute (SizeGNN.forward's own signature,
 *                                       src/linker_size.py:83); edge_mask is then taken as final
 *   logits         device f32 [B,out_node_nf]
 *   flags          device int32 [B]     bit0: NaN in the logits, bit2: more fragment atoms than
 *                                       dl_size_max_fragment_atoms() */
int32_t dl_size_gnn_forward(const dl_size_model* m, int32_t B, int32_t N, const float* one_hot,
                            const float* positions, const float* fragment_mask, const float* edge_mask,
                            const float* distances, float* logits, int32_t* flags, void* stream);


/* ---- training of the linker-size predictor (size_gnn_train.hip) -----------------------------------------
 * SizeClassifier.forward in training mode (src/linker_size_lightning.py:83-117: BatchNorm1d normalising over ALL B*N rows,
 * padding and linker rows included) and the gradient of sum(grad_logits * logits) with respect to every parameter.  Scope:
 * hidden_nf = 128, normalization None (batch_norm = 0) or 'batch_norm' (1, eps 1e-5), any n_layers, in_node_nf <= 16,
 * out_node_nf <= 64, at most dl_size_max_fragment_atoms() fragment atoms per molecule.  params / grad_params are ONE flat fp32
 * buffer each in SizeGNN.parameters() order: the raw weights, BatchNorm affine weight and bias included (n_params must be
 * dl_size_train_num_params).  The forward saves its state in the workspace; the backward reads the workspace of the matching
 * forward (same args, same params, the workspace untouched in between).  Deterministic: fixed-order reductions, no atomics.
 * The callee allocates nothing; null pointers, a wrong n_params, a too-small workspace and B*N < 2 with BatchNorm return
 * DL_ERR_BAD_ARG, hyper-parameters outside the scope DL_ERR_UNSUPPORTED, all before any device work. */
typedef struct dl_size_train_args {
    int32_t B, N;
    int32_t in_node_nf, hidden_nf, out_node_nf, n_layers;
    int32_t batch_norm;             /* 0: normalization None, 1: 'batch_norm' */
    const float* params;            /* device f32 [n_params] */
    int64_t n_params;
    const float* one_hot;           /* device f32 [B,N,in_node_nf] */
    const float* positions;         /* device f32 [B,N,3] */
    const float* fragment_mask;     /* device f32 [B,N]: the GNN's node mask */
    const float* edge_mask;         /* device f32 [B,N,N]: an edge is kept where != 0 and |x_i - x_j|^2 < 6 */
    float* logits;                  /* device f32 [B,out_node_nf] out (forward) */
    float* batch_stats;             /* device f32 [n_layers][2: node_mlp.1, node_mlp.4][2: mean, biased var][128] out
                                       (forward, batch_norm = 1 only) */
    int32_t* flags;                 /* device int32 [B] out (forward): 4 = more fragment atoms than
                                       dl_size_max_fragment_atoms() (that molecule's results are meaningless) */
    const float* grad_logits;       /* device f32 [B,out_node_nf] (backward) */
    float* grad_params;             /* device f32 [n_params] out (backward) */
    void* workspace;                /* device, >= dl_size_train_workspace_bytes; contents unspecified on entry of the forward (it
                                     * writes all the backward reads), the matching backward needs them untouched, unspecified
                                     * after it; logits and grad_params are written in full */
    size_t workspace_bytes;
} dl_size_train_args;
int64_t dl_size_train_num_params(const dl_size_train_args* args);        /* -1 outside the scope */
size_t dl_size_train_workspace_bytes(const dl_size_train_args* args);    /* reads B and the hyper-parameters; 0 outside */
int32_t dl_size_train_forward(const dl_size_train_args* args, void* stream);
int32_t dl_size_train_backward(const dl_size_train_args* args, void* stream);

/* ---- bond perception of a sampled batch (bonds.hip) ----------------------------------------------------
 * build_xae_molecule / get_bond_order (src/molecule_builder.py:44-102) for every molecule of a batch in ONE launch, one
 * workgroup per molecule, plus the connected components of the bond graph (what metrics.is_connected asks of the molecule
 * built from the same bonds).  Real atoms are the rows with node_mask != 0; atom k of every output is the k-th real row
 * (the reference masks a molecule before it builds it); its type is the first maximum of its one-hot row.  For each pair
 * j < i: d = 100 |x_i - x_j| in fp32, and with t = table[type_i][type_j]
 *     order = d < t[0] ? (d < t[1] ? (d < t[2] ? 3 : 2) : 1) : 0
 * `table` holds upper bounds in pm, symmetric in the two types; a negative entry means "no such order".  A non-finite
 * coordinate bonds to nothing.  Deterministic: no global atomics, the same bits on every run.  The callee allocates nothing;
 * N < 1, N > 1024, nf > 16 or table_len != nf * nf * 3 return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch (and
 * without looking at the pointers); null pointers or a workspace below dl_bonds_workspace_bytes return DL_ERR_BAD_ARG, all
 * before any device work. */
#define DL_BONDS_OVERFLOW 1         /* status bit: n_bonds > capacity, the list holds the first `capacity` bonds */
#define DL_BONDS_NONFINITE 2        /* status bit: a real atom has a NaN / inf coordinate */
typedef struct dl_bonds_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* node_mask;         /* device f32 [B,N] */
    const float* table;             /* device f32 [nf,nf,3] */
    int32_t table_len;              /* number of floats in `table` */
    int32_t capacity;               /* bonds the list holds per molecule */
    int32_t* n_bonds;               /* device int32 [B] out: the true count, also beyond the capacity */
    int32_t* bonds;                 /* device int32 [B,capacity,3] out: (i, j, order), j < i, row-major in (i, j); entries
                                       from n_bonds on are not written */
    int32_t* valence;               /* device int32 [B,N] out: sum of the bond orders of atom k; 0 from the atom count on */
    int32_t* n_components;          /* device int32 [B] out */
    int32_t* component;             /* device int32 [B,N] out: smallest atom index of atom k's component; -1 from the atom
                                       count on */
    int32_t* status;                /* device int32 [B] out: DL_BONDS_* bits */
    void* workspace;                /* device, >= dl_bonds_workspace_bytes (may be NULL when that is 0); contents on entry and
                                     * on return unspecified.  Every output is written in full except `bonds`: up to n_bonds */
    size_t workspace_bytes;
} dl_bonds_args;
size_t dl_bonds_workspace_bytes(int32_t B, int32_t N);      /* 0 today: every intermediate fits in LDS */
int32_t dl_perceive_bonds(const dl_bonds_args* args, void* stream);

/* ---- molecule keys of a perceived batch (mol_keys.hip) ---------------------------------------------------
 * Scores of the bond graph dl_perceive_bonds left on the device, one workgroup per molecule, ONE launch per batch, no host
 * round trip between the two launches.  Atoms are numbered as dl_perceive_bonds numbers them (the k-th row with
 * node_mask != 0 is atom k).  `drop_mask` (may be NULL; the reference's pocket_mask) removes atoms AFTER that numbering: a
 * dropped atom and every bond that touches it are ignored; the atoms that stay are the "kept" atoms.
 *
 *   n_atoms       kept atoms
 *   n_over        kept atoms whose valence (sum of the orders of their bonds to kept atoms) exceeds max_valence[type]
 *   n_components  pieces of the graph over the kept atoms (recomputed when drop_mask is given, else `n_components_in`)
 *   n_bonds       bonds between kept atoms (of the list as given: at most `capacity`)
 *   colour        colour refinement (1-WL) with 64-bit integers, all arithmetic modulo 2^64:
 *                     mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                               z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31          (splitmix64)
 *                     mix2(a, b) = mix64(a + b * 0xD6E8FEB86659FD93)
 *                     c_0[i]   = mix2(0x243F6A8885A308D3, type_i + 1)
 *                     c_r+1[i] = mix2(c_r[i], sum over the kept bonds (i, j, order) of mix2(c_r[j], order))
 *                 for exactly n_atoms rounds (a partition of n atoms settles within n rounds; the count depends on nothing
 *                 but n_atoms, so it is the same under every renumbering).  colour[b][k] is the final colour of atom k, 0 for
 *                 a dropped atom and from the atom count on.
 *   key           mix2(mix2(mix2(0x13198A2E03707344, n_atoms), n_bonds), sum over the kept atoms of mix64(colour))
 *   status        the DL_BONDS_* bits of `status_in`, plus DL_KEYS_TOO_LARGE and DL_KEYS_BAD_BOND.  Any bit but
 *                 DL_BONDS_NONFINITE means that key and colour do not describe the molecule (a cut list, an entry that is
 *                 not a bond); with DL_KEYS_TOO_LARGE they are 0.
 *
 * An entry of the list is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3; any other entry is skipped and sets
 * DL_KEYS_BAD_BOND.  Sums are commutative and integer: the same bits on every run and under every order of the list.  Global
 * memory is written with plain stores only.  Argument errors (null pointers, N < 1, nf < 1 or > 16, max_valence_len != nf,
 * capacity < 0) return DL_ERR_BAD_ARG before any device work; B == 0 returns DL_OK without a launch. */
#define DL_KEYS_TOO_LARGE 4         /* status bit: more than 1024 real atoms, or more kept bonds than the workgroup's LDS holds */
#define DL_KEYS_BAD_BOND 8          /* status bit: a list entry that is not a bond of this molecule was skipped */
typedef struct dl_mol_keys_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: dl_bonds_args.bonds (may be NULL when capacity is 0) */
    const int32_t* valence_in;      /* device int32 [B,N]: dl_bonds_args.valence (used when drop_mask is NULL) */
    const int32_t* n_components_in; /* device int32 [B]: dl_bonds_args.n_components (used when drop_mask is NULL) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    const int32_t* max_valence;     /* device int32 [nf]: most bonds an atom of each type may carry */
    int32_t max_valence_len;
    int32_t* n_atoms;               /* device int32 [B] out */
    int32_t* n_over;                /* device int32 [B] out */
    int32_t* n_components;          /* device int32 [B] out */
    int32_t* n_bonds;               /* device int32 [B] out */
    uint64_t* key;                  /* device 64-bit [B] out */
    uint64_t* colour;               /* device 64-bit [B,N] out */
    int32_t* status;                /* device int32 [B] out */
} dl_mol_keys_args;
int32_t dl_molecule_keys(const dl_mol_keys_args* args, void* stream);

/* ---- symmetry-aware RMSD of a list of pairs (rmsd.hip) ------------------------------------------------------
 * compute_metrics.py:366-402 scores every recovered sample with rdMolAlign.GetBestRMS(pred, true): the smallest RMSD after
 * a rigid alignment (proper rotations only, no reflection) over all atom correspondences that are isomorphisms of the two
 * graphs.  Here the host enumerates the correspondences ("maps", metrics.isomorphisms) and ONE launch scores the whole list,
 * one 256-thread workgroup per pair.
 *
 * Atoms are the kept atoms of a molecule renumbered from 0, exactly as metrics.to_host numbers a Graph.  A map of pair p is a
 * bijection image[0 .. n_atoms[p]): atom k of `xa` corresponds to atom image[k] of `xb`.
 *
 * LAYOUT OF THE MAP TABLE.  `maps` holds `maps_capacity` maps' worth of 16-bit atom indices, n_max to a map.  The maps of
 * pair p are the m_p = map_offsets[p + 1] - map_offsets[p] maps from map_offsets[p] on, and their block starts at element
 * map_offsets[p] * n_max.  INSIDE a block the entries are atom-major: image[k] of the pair's j-th map is
 *     maps[map_offsets[p] * n_max + k * m_p + j],      0 <= k < n_atoms[p], 0 <= j < m_p
 * so the 64 lanes of a wave, one map each, read 64 consecutive 16-bit words for every atom.  The rest of a block (from element
 * n_atoms[p] * m_p on) is never read.
 *
 *   rmsd     sqrt(min over the maps of min over rotations R and translations t of mean_k |R a_k + t - b_image[k]|^2); the
 *            factor sqrt(n_atoms / n_linker) of the reference is the caller's.  NaN when status is not 0.
 *   best     index, within the pair, of the map that gives it; of equal candidates the lowest, so the same on every run;
 *            -1 when status is not 0.
 *   status   0, or DL_RMSD_* bits.  A pair with a bit set does not touch the other pairs of the launch.
 *
 * Candidates are compared as Ga + Gb - 2 lambda with lambda the largest eigenvalue of Horn's 4x4 quaternion matrix (cyclic
 * Jacobi, fp64: safe for n = 1, 2, collinear, planar and coinciding sets); the winner's residual is then summed directly as
 * sum |R a_k - b_image[k]|^2 in fp64, which does not cancel when the structures coincide.  Coordinates are centred in fp64 and
 * held in fp32.  An index beyond the atom count is clamped (no fault; that map's value means nothing).
 *
 * Global memory is written with plain stores only; the callee allocates nothing.  A null `args`, P < 0, n_max < 1 or > 65536
 * or maps_capacity < 0 return DL_ERR_BAD_ARG; then P == 0 returns DL_OK without a launch (and without looking at the
 * pointers); then null pointers (`maps` may be NULL when maps_capacity is 0) return DL_ERR_BAD_ARG, all before any device
 * work. */
#define DL_RMSD_NONFINITE 1         /* status bit: a coordinate of the pair is NaN or infinite */
#define DL_RMSD_NO_MAP 2            /* status bit: no map for this pair (or no atom, or offsets that leave the table) */
#define DL_RMSD_TOO_LARGE 4         /* status bit: n_atoms above n_max or above the 1024 atoms the workgroup's LDS holds */
typedef struct dl_rmsd_args {
    int32_t P, n_max;               /* pairs; atoms per padded molecule */
    const float* xa;                /* device f32 [P,n_max,3]: the predictions */
    const float* xb;                /* device f32 [P,n_max,3]: the true molecules */
    const int32_t* n_atoms;         /* device int32 [P] */
    const int32_t* map_offsets;     /* device int32 [P+1]: first map of each pair, ascending */
    const uint16_t* maps;           /* device 16-bit [maps_capacity * n_max], layout above */
    int32_t maps_capacity;          /* maps the table holds (>= map_offsets[P]) */
    float* rmsd;                    /* device f32 [P] out */
    int32_t* best;                  /* device int32 [P] out */
    int32_t* status;                /* device int32 [P] out */
} dl_rmsd_args;
int32_t dl_best_rmsd(const dl_rmsd_args* args, void* stream);

/* ---- steric clashes of generated atoms with the protein (clash.hip) -------------------------------------------
 * Does the linker fit, or does it sit inside the protein?  The reference has no code for this question, so the rule is this
 * project's own; tests/clash_ref.py restates it in numpy float32 and gives the same bits as the kernel.
 *
 * THE RULE.  Atoms are heavy atoms of the project's vocabularies, hydrogens are implicit.  A pair is one QUERY atom (a
 * generated atom) and one TARGET atom (a protein atom).  The host builds threshold[a][b] in fp32 Angstrom, a the query's type
 * and b the target's (const.clash_threshold_table: scale * (r[a] + r[b]) - tolerance over Bondi's van der Waals radii,
 * computed in fp64 and rounded once; defaults scale 0.75, tolerance 0).  An atom's type is the index of the first largest
 * entry of its one-hot row, as dl_perceive_bonds reads it.  With dx = xq - xt (dy, dz alike)
 *     d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
 * every operation a separate fp32 round-to-nearest operation in exactly this order, no fused multiply-add, and the pair
 *     CLASHES       when d2 < t * t and t > 0, t = threshold[a][b]    (t * t one fp32 multiply; the comparison is strict)
 *     is a CONTACT  when d2 < c * c, c = contact_cutoff               (same arithmetic)
 *
 * A molecule's query atoms are its rows with query_mask != 0.  Its targets are its rows with target_mask != 0 that are not
 * query rows (a row set in both masks counts as a query only), followed by the SHARED list target_x / target_type, the same
 * for every molecule of the launch (the whole protein of `generate --protein`).  Masks may be interleaved with padding rows
 * in any order; rows in neither mask are never read.
 *
 *   n_query, n_target   atoms on either side (in-batch targets plus the shared atoms with a type in [0, nf))
 *   n_clashes           clashing pairs
 *   n_clash_atoms       query atoms with at least one clash
 *   n_contacts          contact pairs
 *   min_dist2           smallest d2 over the pairs, +inf without a pair (the caller takes the square root)
 *   atom_clashes        per row: clashing pairs of this query atom; 0 on non-query rows
 *   atom_min_dist2      per row: smallest d2 of this query atom; +inf on non-query rows and without targets
 *   status              0, or DL_CLASH_* bits.  A molecule with a bit set does not touch the other molecules of the launch.
 *
 * With DL_CLASH_NONFINITE or DL_CLASH_TOO_LARGE every integer output of the molecule but `status` is 0 (n_query and n_target
 * included), min_dist2 is NaN and atom_min_dist2 is NaN on its query rows.  DL_CLASH_TOO_LARGE is decided first and such a
 * molecule is not looked at further (its status is exactly that bit).  A shared atom with a type outside [0, nf) is skipped,
 * coordinates and all, and sets DL_CLASH_BAD_TYPE on every molecule; the other outputs stay valid.
 *
 * One 256-thread workgroup per molecule, ONE launch per batch.  Integer sums and minima only: no floating-point
 * accumulation, no atomics, the same bits on every run.  Global memory is written with plain stores only and every output is
 * written in full; the callee allocates nothing.  A null `args`, B < 0, N < 1, nf < 1 or > 16 or M < 0 return DL_ERR_BAD_ARG;
 * then B == 0 returns DL_OK without a launch (and without looking at the pointers); then null pointers (`target_mask` may
 * always be NULL: no in-batch targets; `target_x` and `target_type` may be NULL when M is 0) return DL_ERR_BAD_ARG, all before
 * any device work. */
#define DL_CLASH_NONFINITE 1        /* status bit: a query or target coordinate of the molecule or of the shared list is NaN or infinite */
#define DL_CLASH_TOO_LARGE 2        /* status bit: more than 1024 query atoms */
#define DL_CLASH_BAD_TYPE 4         /* status bit: a target_type outside [0, nf) was skipped */
typedef struct dl_clash_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* query_mask;        /* device f32 [B,N] */
    const float* target_mask;       /* device f32 [B,N] or NULL: in-batch targets (the reference's pocket_mask) */
    int32_t M;                      /* atoms of the shared target list, may be 0 */
    const float* target_x;          /* device f32 [M,3], in the frame of `x` */
    const int32_t* target_type;     /* device int32 [M] */
    const float* threshold;         /* device f32 [nf,nf]: [query type][target type], Angstrom */
    float contact_cutoff;           /* Angstrom */
    int32_t* n_query;               /* device int32 [B] out */
    int32_t* n_target;              /* device int32 [B] out */
    int32_t* n_clashes;             /* device int32 [B] out */
    int32_t* n_clash_atoms;         /* device int32 [B] out */
    int32_t* n_contacts;            /* device int32 [B] out */
    float* min_dist2;               /* device f32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    int32_t* atom_clashes;          /* device int32 [B,N] out */
    float* atom_min_dist2;          /* device f32 [B,N] out */
} dl_clash_args;
int32_t dl_clash_scores(const dl_clash_args* args, void* stream);

/* ---- contacts of generated atoms with the protein: interaction terms (interaction.hip) ------------------------------
 * Does the linker make contacts, and more or fewer than the data set's own linker in the same pocket?  dl_clash_scores
 * cannot say: a linker that runs out into the solvent is clash free.  These two entry points evaluate the empirical
 * intermolecular terms of Trott & Olson (AutoDock Vina, J. Comput. Chem. 31, 455 (2010)): two steric Gaussians, a
 * repulsion, a hydrophobic term and a hydrogen-bond term over surface distances.  THE RULE IS THIS PROJECT'S OWN after that
 * published functional form.  It is NOT AutoDock Vina's numbers: no hydrogens, no PDBQT typing, no search or pose
 * optimisation, no intramolecular term and no rotor normalisation (the published rotor weight is not used).
 * tests/interaction_ref.py restates both entry points in numpy.
 *
 * dl_interaction_types: TYPING from elements and geometry alone.  An atom's element is the index of the first largest
 * entry of its one_hot row, in the project's atom order C O N F S Cl Br I P (indices 0 to 8; further indices carry no flag).
 * `group` says which rows are typed together: 0 = the row is not typed and is never read; rows of one molecule with the
 * same non-zero id are typed among themselves (the callers use 1 for the ligand and 2 for the pocket; a whole protein is
 * B = 1, N = M, all in group 1).  Two rows i > j of a group are NEIGHBOURS when dl_perceive_bonds would give them an
 * order >= 1: d = 100 * sqrtf(dx*dx + dy*dy + dz*dz) in fp32 exactly as bonds.hip evaluates it (one shared device function),
 * and d < table[element of i][element of j], STRICTLY; `table` is the [nf][nf] single-bond bound in pm,
 * const.bond_threshold_table(...)[..., 0] (a negative entry: never neighbours).  deg is the number of neighbours of a row,
 * hetero says that some neighbour is not carbon.  xs_type = element | flags:
 *     C               DL_XS_HYDROPHOBIC when not hetero
 *     F, Cl, Br, I    DL_XS_HYDROPHOBIC
 *     N               DL_XS_DONOR when deg < 3; never an acceptor
 *     O               DL_XS_ACCEPTOR always; DL_XS_DONOR too when deg == 0 (a water), or when deg == 1 and its one
 *                     neighbour lies at d2 >= 1.6875 A^2, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32 as dl_clash_scores
 *                     computes it (27/16, 1.299 A: a hydroxyl, not a carbonyl or carboxylate oxygen)
 *     S, P            no flag
 * Rows of group 0 get -1.  KNOWN MISREADINGS: a pyridine or nitrile N is typed a donor; both N of a histidine ring are
 * donors; pocket residues cut at the pocket boundary lose a neighbour (the peptide bond to a residue outside the pocket
 * is missing, so a proline N there has two neighbours and is typed a donor).  A molecule with a typed row whose coordinates are not finite gets
 * status DL_INTERACT_NONFINITE and -1 on every row; the other molecules of the launch are not touched.  One 256-thread
 * workgroup per molecule, any N: candidates stream through a 256-entry LDS tile.
 *
 * dl_interaction_scores: THE PAIR TERMS.  Queries and targets as for dl_clash_scores: the query atoms of a molecule are its
 * rows with query_mask != 0, its targets the rows with target_mask != 0 that are not query rows, followed by the shared list
 * target_x / target_xs; rows in neither mask are never read.  xs_type [B,N] and target_xs [M] are what dl_interaction_types
 * wrote; radius[nf] is an fp64 table in Angstrom (const.XS_RADII).  For a query atom a and a target atom b, in fp64 with no
 * fused multiply-add, from the fp32 coordinates widened to fp64:
 *     dx = xq - xt (dy, dz alike);  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
 *     the pair counts when d2 < 64.0            (8 A, strict)
 *     r = sqrt(d2);  s = r - (radius[a] + radius[b])
 *     gauss1      = exp(-((s / 0.5) * (s / 0.5)))
 *     gauss2      = exp(-(((s - 3.0) / 2.0) * ((s - 3.0) / 2.0)))
 *     repulsion   = s < 0 ? s * s : 0
 *     hydrophobic = both DL_XS_HYDROPHOBIC ? (s < 0.5 ? 1 : s < 1.5 ? 1.5 - s : 0) : 0
 *     hbond       = (a donor and b acceptor) or (a acceptor and b donor) ? (s < -0.7 ? 1 : s < 0 ? -s / 0.7 : 0) : 0
 * Every pair term becomes a signed 64-bit fixed point, llrint(term * 2^32), and ALL sums are integer sums: the same bits on
 * every run and under every mapping of pairs to lanes.  THE RANGE: a term is below 20 (the repulsion at s = -4.4, the
 * largest radius sum), so 1024 queries x 65536 targets x 20 x 2^32 stays below 2^63 - and only pairs inside 8 A add anything.
 *
 *   n_query, n_target   atoms on either side (in-batch targets plus the shared atoms that have a type)
 *   n_pairs             pairs inside the cut
 *   n_hbonds            pairs with hbond > 0
 *   n_hydrophobic       pairs with hydrophobic > 0
 *   terms               [B,5] fixed point: gauss1, gauss2, repulsion, hydrophobic, hbond summed over the pairs
 *   atom_terms          [B,N,5] fixed point: the same per query row; 0 on non-query rows
 *   status              0, or DL_INTERACT_* bits.  A molecule with a bit set does not touch the other molecules of the launch.
 * The host forms the weighted score in fp64, sum(w_k * terms_k) / 2^32 with the published weights
 * (const.INTERACTION_WEIGHTS).
 *
 * With DL_INTERACT_NONFINITE (a query or target coordinate is NaN or infinite), DL_INTERACT_TOO_LARGE (more than 1024
 * query atoms; decided first, the molecule is not looked at further) or DL_INTERACT_UNTYPED (a query row or in-batch target
 * row whose xs_type is negative or whose element is not below nf) every output of the molecule but `status` is 0.  A shared
 * atom whose target_xs is negative or whose element is not below nf is skipped, coordinates and all, and sets
 * DL_INTERACT_BAD_TYPE on every molecule; the other outputs stay valid.
 *
 * Both take their struct alone, with the stream as its last field, as dl_fingerprints does.  Global memory is written with plain stores only, no atomics, every output element is written; the callee allocates
 * nothing.  A null `args`, B < 0, N < 1, nf < 1 or > 16 (or M < 0) return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a
 * launch; then null pointers (`target_mask` may always be NULL; `target_x` and `target_xs` may be NULL when M is 0) return
 * DL_ERR_BAD_ARG, all before any device work. */
#define DL_XS_HYDROPHOBIC 16        /* xs_type bit 4 (bits 0-3: the element index) */
#define DL_XS_DONOR 32              /* xs_type bit 5 */
#define DL_XS_ACCEPTOR 64           /* xs_type bit 6 */
#define DL_INTERACT_TERMS 5         /* gauss1, gauss2, repulsion, hydrophobic, hbond */
#define DL_INTERACT_NONFINITE 1     /* status bit: a typed row, a query or a target coordinate is NaN or infinite */
#define DL_INTERACT_TOO_LARGE 2     /* status bit: more than 1024 query atoms */
#define DL_INTERACT_BAD_TYPE 4      /* status bit: a shared atom without a usable target_xs was skipped */
#define DL_INTERACT_UNTYPED 8       /* status bit: a query or in-batch target row without a usable xs_type */
typedef struct dl_interact_types_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const int32_t* group;           /* device int32 [B,N]: 0 = not typed */
    const float* table;             /* device f32 [nf,nf]: single-bond upper bounds, pm */
    int32_t* xs_type;               /* device int32 [B,N] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_interact_types_args;
int32_t dl_interaction_types(const dl_interact_types_args* args);

typedef struct dl_interact_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const int32_t* xs_type;         /* device int32 [B,N] */
    const float* query_mask;        /* device f32 [B,N] */
    const float* target_mask;       /* device f32 [B,N] or NULL: in-batch targets (the reference's pocket_mask) */
    int32_t M;                      /* atoms of the shared target list, may be 0 */
    const float* target_x;          /* device f32 [M,3], in the frame of `x` */
    const int32_t* target_xs;       /* device int32 [M] */
    const double* radius;           /* device f64 [nf], Angstrom */
    int32_t* n_query;               /* device int32 [B] out */
    int32_t* n_target;              /* device int32 [B] out */
    int32_t* n_pairs;               /* device int32 [B] out */
    int32_t* n_hbonds;              /* device int32 [B] out */
    int32_t* n_hydrophobic;         /* device int32 [B] out */
    int64_t* terms;                 /* device int64 [B,5] out */
    int32_t* status;                /* device int32 [B] out */
    int64_t* atom_terms;            /* device int64 [B,N,5] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_interact_args;
int32_t dl_interaction_scores(const dl_interact_args* args);

/* ---- gridded shape overlap of two molecules in one frame (shape.hip) ---------------------------------------------
 * Where does a sample lie in space, compared with the molecule it was sampled for?  The reference answers with SC-RDKit; half
 * of that is 1 - ShapeProtrudeDist(pred, true), a gridded van der Waals volume overlap.  RDKit is absent here and its numbers
 * cannot be pinned, so spacing, scale and layering follow RDKit's defaults (gridSpacing 0.5, vdwScale 0.8, stepSize 0.25, two
 * bits per point, ignoreHs) and past that THE RULE IS THIS PROJECT'S OWN: not RDKit's grid, not RDKit's numbers, and not
 * "SC-RDKit" (no pharmacophore features, no alignment).  tests/shape_ref.py restates it in numpy float32 and gives the same
 * integers as the kernel.  DiffLinker's samples share the fragments' coordinates with the data set's molecule, so the two
 * molecules are compared in place.
 *
 * THE RULE.  A launch scores B pairs.  Pair b is molecule A (x_a [B,Na,3], one_hot_a [B,Na,nf], mask_a [B,Na]) and molecule
 * B (x_b [B,Nb,3], one_hot_b, mask_b); Na and Nb are independent.  A row takes part when its mask is non-zero; its type is
 * the index of the first largest entry of its one-hot row, as dl_perceive_bonds and dl_clash_scores read it.  Rows that do not
 * take part are never read, whatever they hold.
 *   Radii.     The host builds r2[type][k], k = 0, 1, 2 (const.shape_radius_table): r_k = scale * vdw[type] + k * step in fp64
 *              over Bondi's radii (const.VDW_RADII), defaults scale 0.8 and step 0.25; r_k is rounded to fp32 once and
 *              r2 = r_k * r_k is one fp32 multiplication.  scale and step are arguments of the table, not of the kernel.
 *   Lattice.   Points sit at p = (0.5f*i, 0.5f*j, 0.5f*k) for ALL integers i, j, k, in the frame of the input coordinates
 *              (exact in fp32).  The lattice is fixed in that frame: moving both molecules by a multiple of 0.5 A changes
 *              nothing, moving them by less does (one C at the origin has volume 431, at (0.25, 0, 0) 460).
 *   Distance.  dx = px - xa (dy, dz alike),  d2 = ((dx*dx) + (dy*dy)) + (dz*dz), every operation a separate fp32
 *              round-to-nearest operation in exactly this order, no fused multiply-add.  Comparisons are strict.
 *   Level.     An atom of type t gives a point (d2 < r2[t][0]) + (d2 < r2[t][1]) + (d2 < r2[t][2]); the LEVEL of a point for
 *              a molecule is the maximum of that over the molecule's participating atoms: 3 inside the scaled van der Waals
 *              sphere, 2 and 1 in the two layers around it, 0 outside.
 *   Outputs    per pair, all int32, sums over the whole lattice (only finitely many points are non-zero, so which box an
 *              implementation walks is not part of the rule, and no output depends on the order of anything):
 *                vol_a = sum level_A      vol_b = sum level_B      vol_min = sum min(level_A, level_B)
 *                core_a = #{level_A = 3}  core_b = #{level_B = 3}  core_both = #{level_A = 3 and level_B = 3}
 *                n_a, n_b   participating rows of either molecule
 *                status     0 or ONE DL_SHAPE_* flag
 *   Flags.     Decided in this order, the first that holds is the status and the pair is not looked at further; a flagged
 *              pair has every integer output except `status` set to 0 (n_a and n_b included) and leaves the other pairs of
 *              the launch alone.
 *                DL_SHAPE_NONFINITE     a participating coordinate is NaN or infinite
 *                DL_SHAPE_OUT_OF_RANGE  a participating |coordinate| > 4096
 *                DL_SHAPE_TOO_LARGE     with lo = floor(2*min) and hi = floor(2*max) per axis over the participating atoms of
 *                                       BOTH molecules (2*x and floor are exact in fp32): hi - lo > 240 on any axis, about 120 A
 *              A pair with n_a = 0 or n_b = 0 is not an error: its sums are what the rule gives.
 * The score the callers form: vol_min / vol_a is 1 - (protrude distance of A from B), the term SC-RDKit weighs by 0.5;
 * vol_min / (vol_a + vol_b - vol_min) is a Tanimoto overlap.
 *
 * One 256-thread workgroup per pair, ONE launch per batch; the levels live as bit planes in LDS (shape.hip).  Integer sums
 * only, the same bits on every run.  Global memory is written with plain stores only, no global atomics, and every output
 * element is written; the callee allocates nothing.  Every r2 entry must be finite and at most 400 (a 20 A radius): the host
 * wrapper checks it; the kernel stays inside its memory with any table, but its sums are the rule's only within that limit.
 * A null `args`, B < 0, Na < 1, Nb < 1, nf < 1 or > 16 return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch (and
 * without looking at the pointers); then a null pointer returns DL_ERR_BAD_ARG, all before any device work. */
#define DL_SHAPE_NONFINITE 1        /* status: a participating coordinate is NaN or infinite */
#define DL_SHAPE_OUT_OF_RANGE 2     /* status: a participating |coordinate| > 4096 */
#define DL_SHAPE_TOO_LARGE 4        /* status: the two molecules together span more than 240 lattice steps on an axis */
typedef struct dl_shape_args {
    int32_t B, Na, Nb, nf;
    const float* x_a;               /* device f32 [B,Na,3], Angstrom */
    const float* one_hot_a;         /* device f32 [B,Na,nf] */
    const float* mask_a;            /* device f32 [B,Na] */
    const float* x_b;               /* device f32 [B,Nb,3], in the frame of x_a */
    const float* one_hot_b;         /* device f32 [B,Nb,nf] */
    const float* mask_b;            /* device f32 [B,Nb] */
    const float* r2;                /* device f32 [nf,3]: squared radii of the three levels, Angstrom^2 */
    int32_t* vol_a;                 /* device int32 [B] out */
    int32_t* vol_b;                 /* device int32 [B] out */
    int32_t* vol_min;               /* device int32 [B] out */
    int32_t* core_a;                /* device int32 [B] out */
    int32_t* core_b;                /* device int32 [B] out */
    int32_t* core_both;             /* device int32 [B] out */
    int32_t* n_a;                   /* device int32 [B] out */
    int32_t* n_b;                   /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
} dl_shape_args;
int32_t dl_shape_scores(const dl_shape_args* args, void* stream);

/* ---- ring perception of a perceived batch (rings.hip) -------------------------------------------------------
 * Ring topology of the bond graph dl_perceive_bonds left on the device: one workgroup per molecule, ONE launch per batch, no
 * host round trip.  The list is read with the conventions of dl_molecule_keys: atom k is the k-th row with node_mask != 0;
 * `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with every bond that touches them; an entry
 * (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation; any other entry is
 * skipped and sets DL_RINGS_BAD_BOND.  `mark_mask` (may be NULL; [B,N] by row like drop_mask) marks atoms; the callers pass
 * the linker mask.  Everything below is over the SIMPLE graph of the kept atoms and the distinct kept pairs; orders play no
 * part beyond the validity of an entry.
 *
 *   n_atoms       kept atoms
 *   n_bonds       distinct kept pairs
 *   n_components  pieces of that graph
 *   n_rings       n_bonds - n_atoms + n_components: the cyclomatic number, the size of a smallest set of smallest rings.
 *                 It equals RDKit's ring count (CalcNumRings, RingInfo.NumRings) except for cages such as cubane, where
 *                 RDKit's symmetrised set has more rings (6 for cubane; 5 here).
 *   bond_ring     [B,capacity], written in full.  For list entry e that is a kept bond (u, v): the number of atoms of the
 *                 smallest cycle through that bond, that is 1 + the length in bonds of the shortest path from u to v that
 *                 does not use the bond itself; 0 when there is none (a bridge).  0 for every skipped entry, every entry
 *                 with a dropped end, and every e >= min(n_bonds_in, capacity).  Repeated entries of one pair (in either
 *                 orientation) all get that pair's value and set DL_RINGS_BAD_BOND; dl_perceive_bonds never emits them.
 *   atom_ring     [B,N] by atom number: the smallest non-zero bond_ring over atom k's kept bonds; 0 when the atom is in no
 *                 ring, when it is dropped, and from the atom count on.
 *   ring_hist     [B,2,DL_RING_BINS].  Row 0 counts the list entries that are kept bonds by the bin of their bond_ring
 *                 (bin 0: in no ring; bins 1..5: smallest ring of 3..7 atoms; bin 6: of 8 or more); row 1 counts the same
 *                 only for bonds with at least one marked end, and is all zero when mark_mask is NULL.
 *   status        the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative n_bonds_in counts
 *                 as 0), DL_RINGS_BAD_BOND, and DL_RINGS_TOO_LARGE for more than DL_RINGS_MAX_ATOMS KEPT atoms: every
 *                 output of that molecule except `status` and `n_atoms` is then 0 (its list is not looked at) and the other
 *                 molecules of the launch are untouched.  N itself may be up to 1024: pockets are dropped, not counted.
 *
 * Integer work only: the same bits on every run and under every order of the list (bond_ring permuted with it).  Global
 * memory is written with plain stores only, every output element is written, the callee allocates nothing.  A null `args`,
 * B < 0, N < 1, N > 1024 or capacity < 0 return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null
 * pointer (other than drop_mask, mark_mask, and `bonds` / `bond_ring` when capacity is 0) returns DL_ERR_BAD_ARG, all before
 * any device work.
 * Not here: enumerating the rings or counting them by size, fused / spiro / bridged classes.  Aromaticity: dl_aromatic_rings
 * below. */
#define DL_RINGS_MAX_ATOMS 256      /* kept atoms per molecule */
#define DL_RING_BINS 7              /* 0: in no ring; 1..5: smallest ring of 3..7 atoms; 6: of 8 or more */
#define DL_RINGS_TOO_LARGE 4        /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_RINGS_BAD_BOND 8         /* status bit, same value as DL_KEYS_BAD_BOND */
typedef struct dl_rings_args {
    int32_t B, N;
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: dl_bonds_args.bonds (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    int32_t* n_atoms;               /* device int32 [B] out */
    int32_t* n_bonds;               /* device int32 [B] out */
    int32_t* n_components;          /* device int32 [B] out */
    int32_t* n_rings;               /* device int32 [B] out */
    int32_t* bond_ring;             /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
    int32_t* atom_ring;             /* device int32 [B,N] out */
    int32_t* ring_hist;             /* device int32 [B,2,DL_RING_BINS] out */
    int32_t* status;                /* device int32 [B] out */
} dl_rings_args;
int32_t dl_ring_scores(const dl_rings_args* args, void* stream);

/* ---- matched-pair double cuts: linker-design examples from molecules (fragment.hip) --------------------------
 * Every way to cut a molecule at two bonds into fragment 1, linker and fragment 2: one workgroup per molecule, ONE launch
 * per batch.  This project's statement of DeLinker's preparation rule, after RDKit's FragmentMol with minCuts = maxCuts = 2
 * and the pattern [#6+0;!$(*=,#[!#6])]!@!=!#[*], over heavy atoms.
 *
 * INPUT.  Atom k is the k-th row with node_mask != 0; its type is the FIRST largest entry of its one_hot row; `charge`
 * ([B,N] by row; NULL: 0 everywhere) is its formal charge.  The bond list has the layout of dl_perceive_bonds: an entry
 * (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 4 (4: aromatic), in either orientation; any
 * other entry is skipped and sets DL_FRAG_BAD_BOND.  A repeated pair counts once, as its FIRST entry (position and order),
 * and sets DL_FRAG_BAD_BOND.  Entries from min(n_bonds_in, capacity) on are not read.
 *
 * CUTTABLE.  A bond is cuttable when (1) its order is 1, (2) it lies in no ring: removing it disconnects its ends, and
 * (3) at least one end is a carbon (type == carbon_type) with charge 0 that has no order-2 or order-3 bond to a non-carbon
 * atom.  The other end is any atom.  So C(=O)-N and C(=O)-O are not cuttable, C(=O)-C is (through its other end), and N-O
 * never is.
 *
 * CUTS.  The molecule must be one piece, otherwise DL_FRAG_DISCONNECTED and no cuts (a molecule without atoms is no piece
 * and has no cuts either).  Every unordered pair of cuttable bonds e1 < e2 (list positions of their first entries) splits it
 * into three pieces: the LINKER touches both bonds, fragment 1 lies beyond e1, fragment 2 beyond e2.  anchor_k is the
 * fragment atom of bond e_k, exit_k its linker atom.  path_atoms is the number of atoms on the shortest path from exit_1 to
 * exit_2, both counted (1 when they are one atom); both bonds are bridges, so that path stays inside the linker.  A pair is
 * KEPT when n_linker >= min_linker, n_frag_1 >= min_fragment, n_frag_2 >= min_fragment, path_atoms >= min_path_atoms and,
 * when linker_leq_frags != 0, n_linker <= min(n_frag_1, n_frag_2).  DeLinker's values are 3, 5, 2, 1.  Kept pairs are
 * numbered in lexicographic order of (e1, e2).
 *
 *   n_atoms     atoms (real rows)
 *   n_bonds     distinct pairs of the list
 *   n_cuttable  cuttable bonds (also reported for a molecule of several pieces)
 *   n_cuts      ALL kept pairs, also those beyond R
 *   bond_side   [B,capacity], written in full: for the first entry of a cuttable bond the number of atoms on the side of its
 *               atom i; 0 for every other entry
 *   cuts        [B,R,DL_FRAG_CUT_FIELDS]: the first min(n_cuts, R) records (e1, e2, anchor_1, exit_1, anchor_2, exit_2,
 *               n_frag_1, n_frag_2, n_linker, path_atoms); zeros after them
 *   labels      uint8 [B,R,N] by atom number: 0 fragment 1, 1 fragment 2, 2 linker; 255 from the atom count on and in
 *               every unused record
 *   status      the bits of `status_in` (NULL: none), plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative
 *               n_bonds_in counts as 0), DL_FRAG_BAD_BOND, DL_FRAG_DISCONNECTED, DL_FRAG_TRUNCATED (n_cuts > R) and
 *               DL_FRAG_TOO_LARGE for more than DL_FRAG_MAX_ATOMS atoms: every count of that molecule except n_atoms is
 *               then 0, its bond_side and cuts are 0 and its labels 255 (no record is used; its list is not looked at),
 *               and the other molecules of the launch are untouched.
 *
 * Integer work only: the same bits on every run.  Global memory is written with plain stores only, every output element is
 * written, the callee allocates nothing.  A null `args`, B < 0, N < 1, N > 1024, nf < 1, carbon_type outside [0, nf),
 * capacity < 0 or R < 0 return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer (other than
 * charge, status_in, `bonds` / `bond_side` when capacity is 0 and `cuts` / `labels` when R is 0) returns DL_ERR_BAD_ARG, all
 * before any device work.
 * Not here: SMILES (so symmetric cuts are not merged), conformers, BRICS, aromaticity perception beyond the list's orders,
 * hydrogens.  Cuts at three to five bonds: dl_fragment_multicuts below.  Pockets: dl_pocket_select below. */
#define DL_FRAG_MAX_ATOMS 256       /* atoms per molecule */
#define DL_FRAG_CUT_FIELDS 10       /* int32 values per record of `cuts` */
#define DL_FRAG_TOO_LARGE 4         /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_FRAG_BAD_BOND 8          /* status bit, same value as DL_KEYS_BAD_BOND */
#define DL_FRAG_DISCONNECTED 16     /* status bit: the molecule is not one piece; no cuts */
#define DL_FRAG_TRUNCATED 32        /* status bit: n_cuts > R; `cuts` and `labels` hold the first R */
typedef struct dl_fragment_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const int32_t* charge;          /* device int32 [B,N] by row, or NULL */
    int32_t carbon_type;            /* index of carbon in the type table */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B] */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status, or NULL */
    int32_t min_linker, min_fragment, min_path_atoms, linker_leq_frags;
    int32_t R;                      /* records `cuts` and `labels` hold per molecule */
    int32_t* n_atoms;               /* device int32 [B] out */
    int32_t* n_bonds;               /* device int32 [B] out */
    int32_t* n_cuttable;            /* device int32 [B] out */
    int32_t* n_cuts;                /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    int32_t* bond_side;             /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
    int32_t* cuts;                  /* device int32 [B,R,DL_FRAG_CUT_FIELDS] out (may be NULL when R is 0) */
    uint8_t* labels;                /* device uint8 [B,R,N] out (may be NULL when R is 0) */
} dl_fragment_args;
int32_t dl_fragment_cuts(const dl_fragment_args* args, void* stream);

/* ---- multi-cuts: one linker joined to three, four or five fragments (fragment.hip) ----------------------------
 * Every way to cut a molecule at k = 3, 4 or 5 bonds into ONE linker and k fragments, the examples a multi-fragment data set is
 * made of: one workgroup per molecule, ONE launch per batch.  This project's statement of what the reference asks of RDKit's
 * FragmentMol with minCuts = 3, maxCuts = 5 (data/geom/generate_geom_multifrag.py:227-231), over heavy atoms.  No run of the
 * reference pins it (RDKit is no dependency of this project): this text is the authority, restated in tests/multicut_ref.py.
 *
 * Atoms, bond entries, DL_FRAG_BAD_BOND, "first entry of a repeated pair", CUTTABLE, "one piece" (DL_FRAG_DISCONNECTED: no
 * cuts) and DL_FRAG_TOO_LARGE are exactly those of dl_fragment_cuts above.  Cuttable bonds are numbered in list order.
 *
 * GATES.  A molecule is cut only when n_atoms <= max_atoms and n_bonds - n_atoms + 1 >= min_rings (the cyclomatic number
 * of dl_ring_scores; the reference asks NumRings() >= 3 of at most 40 atoms, the same except for cages).  A molecule that
 * fails a gate has no cuts, and the gate sets no status bit; its other outputs are what they would be without the gates.
 *
 * MANY.  A molecule that passes the gates and has more than DL_FRAG_MULTI_MAX_CUTTABLE cuttable bonds sets
 * DL_FRAG_MANY_CUTTABLE and has no cuts (a molecule of 40 atoms has at most 39; the reference itself stops at 100).
 *
 * STARS.  Removing a set of k cuttable bonds e_1 < ... < e_k (list positions) leaves k + 1 pieces.  The set is a STAR when one
 * piece touches all k bonds: that piece is the LINKER, fragment q is the piece beyond e_q, anchor_q is the fragment atom of
 * e_q and exit_q its linker atom (exits may coincide).  A star is KEPT when n_linker >= min_linker and every fragment has at
 * least min_fragment atoms; the reference's values are 3 and 3.  There is no path rule and no linker-versus-fragments rule.
 * Kept stars are numbered by k ascending, min_cuts <= k <= max_cuts, and within a k in lexicographic order of (e_1, ..., e_k).
 *
 *   n_atoms, n_bonds, n_cuttable   as dl_fragment_cuts (n_cuttable is the whole count, also beyond 64 and behind a gate)
 *   n_cuts      ALL kept stars, also those beyond R
 *   n_cuts_k    [B,3]: the kept stars of 3, 4 and 5 bonds (0 for a k outside min_cuts..max_cuts)
 *   cuts        [B,R,DL_FRAG_MULTI_FIELDS]: the first min(n_cuts, R) records (k, n_linker, e[5], anchor[5], exit[5],
 *               n_frag[5]), the slots q >= k of every row of five hold -1; unused records are all 0
 *   labels      uint8 [B,R,N] by atom number: q for fragment q (0..4), DL_FRAG_MULTI_LINKER for the linker; 255 from the atom
 *               count on and in every unused record
 *   status      as dl_fragment_cuts, plus DL_FRAG_MANY_CUTTABLE; DL_FRAG_TRUNCATED when n_cuts > R.  DL_FRAG_TOO_LARGE: every
 *               count except n_atoms is 0, cuts 0, labels 255.
 *
 * Integer work only: the same bits on every run.  Global memory is written with plain stores only, every output element is
 * written, the callee allocates nothing.  Arguments are checked as by dl_fragment_cuts, and min_cuts < 3, max_cuts > 5 or
 * min_cuts > max_cuts return DL_ERR_BAD_ARG as well; n_cuts_k may not be null.  max_atoms and min_rings are any integers
 * (256 and 0 switch the gates off).
 * Not here: SMILES (symmetric cuts are not merged), conformers, BRICS, hydrogens, pockets. */
#define DL_FRAG_MULTI_FIELDS 22         /* int32 values per record of `cuts`: k, n_linker, 4 x 5 */
#define DL_FRAG_MULTI_MIN_CUTS 3
#define DL_FRAG_MULTI_MAX_CUTS 5
#define DL_FRAG_MULTI_MAX_CUTTABLE 64   /* cuttable bonds of a molecule that is cut */
#define DL_FRAG_MULTI_LINKER 5          /* value of `labels` for a linker atom */
#define DL_FRAG_MANY_CUTTABLE 64        /* status bit: more than DL_FRAG_MULTI_MAX_CUTTABLE cuttable bonds; no cuts */
typedef struct dl_fragment_multi_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const int32_t* charge;          /* device int32 [B,N] by row, or NULL */
    int32_t carbon_type;            /* index of carbon in the type table */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B] */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status, or NULL */
    int32_t min_cuts, max_cuts;     /* 3 <= min_cuts <= max_cuts <= 5 */
    int32_t min_linker, min_fragment;
    int32_t max_atoms, min_rings;   /* the gates */
    int32_t R;                      /* records `cuts` and `labels` hold per molecule */
    int32_t* n_atoms;               /* device int32 [B] out */
    int32_t* n_bonds;               /* device int32 [B] out */
    int32_t* n_cuttable;            /* device int32 [B] out */
    int32_t* n_cuts;                /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    int32_t* n_cuts_k;              /* device int32 [B,3] out */
    int32_t* cuts;                  /* device int32 [B,R,DL_FRAG_MULTI_FIELDS] out (may be NULL when R is 0) */
    uint8_t* labels;                /* device uint8 [B,R,N] out (may be NULL when R is 0) */
} dl_fragment_multi_args;
int32_t dl_fragment_multicuts(const dl_fragment_multi_args* args, void* stream);

/* ---- aromatic rings from 3D geometry, and Kekule bond orders for them (aromatic.hip) ---------------------------
 * The distance table of dl_perceive_bonds calls a C-C bond double below 1.39 A and single from there on, so an aromatic ring
 * (1.36 - 1.45 A) gets an arbitrary mix of orders.  This entry point finds the planar five- and six-rings of every molecule of
 * a batch, gives their bonds alternating orders and says which rings are aromatic: one workgroup per molecule, ONE launch per
 * batch, no host round trip.  THE RULE BELOW IS THIS PROJECT'S OWN.  It is NOT RDKit's aromaticity model and NOT OpenBabel's
 * bond typing (the reference hands its .xyz files to `obabel`); tests/aromatic_ref.py restates it in plain Python and the
 * kernel agrees with that bit for bit.
 *
 * CONVENTIONS, those of dl_ring_scores.  Atom k is the k-th row with node_mask != 0; its type is the FIRST largest entry of
 * its one_hot row (finite values expected) and its class is ring_class[type]: 1 carbon, 2 nitrogen, 3 oxygen and sulphur,
 * anything else counts as 0.  `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with their bonds.  An
 * entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation; any other entry is
 * skipped and sets DL_AROM_BAD_BOND.  A repeated pair sets DL_AROM_BAD_BOND, and the order of its FIRST entry is the pair's
 * input order.  Entries from min(n_bonds_in, capacity) on are not read.  "Kept" means: not dropped, both ends for a bond.
 *
 * 1. ELIGIBLE.  Degree is counted over the simple graph of the kept atoms.  Class 1 and class 2 atoms are eligible with
 *    degree 2 or 3, class 3 atoms with degree exactly 2, class 0 atoms never.
 * 2. CANDIDATE RINGS.  Every chordless simple cycle of 5 or 6 kept atoms, all eligible, once, in canonical order: from its
 *    smallest atom number, in the direction whose second atom is smaller than its last.
 * 3. PLANAR RINGS.  fp64, contraction off, every operation rounded on its own in the order written.  p_k = (double) x of the
 *    cycle's atoms in canonical order; c = (((p_0 + p_1) + ...) + p_{n-1}) / (double) n by component; q_k = p_k - c;
 *    m = ((q_0 x q_1) + (q_1 x q_2)) + ... + (q_{n-1} x q_0), a cross product being (a_y*b_z - a_z*b_y, a_z*b_x - a_x*b_z,
 *    a_x*b_y - a_y*b_x); mm = (m_x*m_x + m_y*m_y) + m_z*m_z; a dot product v . m is (v_x*m_x + v_y*m_y) + v_z*m_z.
 *    The ring is planar iff mm > 0, and d*d <= tol2_ring * mm with d = q_k . m for every ring atom, and d*d <= tol2_sub * mm
 *    with d = (p_s - c) . m for every kept neighbour s of a ring atom that is not in the ring.  A NaN or inf coordinate
 *    makes a comparison false: the ring is not planar.  tol2_ring and tol2_sub are squares of lengths in A; 0.1^2 and 0.5^2
 *    sit between the aromatic rings of crystal ligands (ring atoms within 0.025 A, substituents within 0.15 A of this plane)
 *    and saturated rings (chair cyclohexane: 0.25 A; a substituent on a tetrahedral ring carbon: about 1.26 A).
 * 4. RING BONDS AND SYSTEMS.  A ring bond joins cyclically consecutive atoms of a planar ring; a system is a connected
 *    component of the graph of ring bonds.
 * 5. ROLES of system atoms, by the first rule that applies.  D (donor of two electrons, takes no ring double bond): class 3,
 *    and class 2 of degree 3.  X (no electron): any other atom with a bond of input order 2 or 3 that is not a ring bond.
 *    P: class 1.  F (flexible): class 2 of degree 2.
 * 6. KEKULE ASSIGNMENT per system.  M is a set of ring bonds whose ends all have role P or F, no atom in two of them.  Among
 *    all such sets M covers the most P atoms; among those, the most F atoms; among those, its sorted list of
 *    (min(u,v), max(u,v)) pairs is lexicographically smallest.  A definition: the result does not depend on the list's order.
 * 7. NEW ORDERS.  A ring bond gets order 2 if it is in M, else 1 (every entry of its pair); every other entry keeps its own
 *    input order.
 * 8. AROMATIC RINGS.  A planar ring is aromatic iff every P atom of it is covered by M and its contributions sum to exactly
 *    6: 2 for D, 0 for X, 1 for a covered P or F, 2 for an uncovered F.  A bond is aromatic when it is a ring bond of an
 *    aromatic ring, an atom when it lies in one.
 *
 *   order_out          [B,capacity], written in full: the new order of every entry that is a bond (an entry with a dropped
 *                      end keeps its input order); 0 for skipped entries and from min(n_bonds_in, capacity) on.  Always 0..3
 *   bond_aromatic      [B,capacity]: 1 for the entries of aromatic bonds, else 0
 *   atom_aromatic      [B,N] by atom number: 1 for aromatic atoms; 0 for dropped atoms and from the atom count on
 *   valence_out        [B,N] by atom number: the sum of the new orders over the distinct kept pairs of the atom (a pair
 *                      outside the rings counts with its input order); 0 for dropped atoms and from the atom count on
 *   n_planar_rings     planar rings
 *   n_aromatic_rings   aromatic rings
 *   n_aromatic_marked  aromatic rings whose atoms are all marked by `mark_mask` ([B,N] by row); 0 when mark_mask is NULL
 *   status             the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative n_bonds_in
 *                      counts as 0), DL_AROM_BAD_BOND, and the limits.  None disturbs the other molecules of the launch.
 *                      DL_AROM_TOO_LARGE: more than DL_AROM_MAX_ATOMS KEPT atoms (N itself may be 1024): order_out holds
 *                        the input orders, everything else is 0, and the list is not searched for repeated pairs.
 *                      DL_AROM_MANY_RINGS: more than DL_AROM_MAX_RINGS planar rings: order_out holds the input orders,
 *                        valence_out their sums, the flags and the three counts are 0.
 *                      DL_AROM_BIG_SYSTEM: a system of more than DL_AROM_MAX_SYSTEM atoms: its bonds keep their input
 *                        orders and its rings count as planar but not aromatic; the other systems are treated as usual.
 *
 * Integer work apart from step 3, which is exact in the order given: the same bits on every run and under every order of the
 * list (order_out and bond_aromatic permuted with it).  Global memory is written with plain stores only, every output
 * element is written, the callee allocates nothing.  A null `args`, B < 0, N < 1, N > 1024, nf < 1, capacity < 0, or a
 * tolerance that is negative or NaN return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer
 * (other than drop_mask, mark_mask, and `bonds` / `order_out` / `bond_aromatic` when capacity is 0) returns DL_ERR_BAD_ARG,
 * all before any device work.
 * Limits of the rule: there are no hydrogens, so N-H and =N- are told apart only by the matching; no formal charges; only
 * rings of 5 and 6 atoms; a planar saturated ring is misread as conjugated; orders outside planar rings stay the distance
 * table's.  Not here: aromatic order 4 in the output, rings of other sizes, the cutting rules of dl_fragment_cuts. */
#define DL_AROM_MAX_ATOMS 256       /* kept atoms per molecule */
#define DL_AROM_MAX_RINGS 64        /* planar rings per molecule */
#define DL_AROM_MAX_SYSTEM 32       /* atoms per ring system */
#define DL_AROM_TOO_LARGE 4         /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_AROM_BAD_BOND 8          /* status bit, same value as DL_KEYS_BAD_BOND */
#define DL_AROM_MANY_RINGS 16       /* status bit: more than DL_AROM_MAX_RINGS planar rings; orders pass through */
#define DL_AROM_BIG_SYSTEM 32       /* status bit: a system of more than DL_AROM_MAX_SYSTEM atoms kept its input orders */
typedef struct dl_aromatic_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* ring_class;      /* device int32 [nf]: 1 C, 2 N, 3 O and S, 0 anything else */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: dl_bonds_args.bonds (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    double tol2_ring;               /* square of the ring atoms' distance from the plane, A^2 (0.1 * 0.1) */
    double tol2_sub;                /* square of the substituents' distance from the plane, A^2 (0.5 * 0.5) */
    int32_t* order_out;             /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
    int32_t* bond_aromatic;         /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
    int32_t* atom_aromatic;         /* device int32 [B,N] out */
    int32_t* valence_out;           /* device int32 [B,N] out */
    int32_t* n_planar_rings;        /* device int32 [B] out */
    int32_t* n_aromatic_rings;      /* device int32 [B] out */
    int32_t* n_aromatic_marked;     /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
} dl_aromatic_args;
int32_t dl_aromatic_rings(const dl_aromatic_args* args, void* stream);

/* ---- pockets: the protein atoms around every ligand of a batch (pocket.hip) -----------------------------------
 * For every (ligand, protein) pair the protein atoms whose GROUP holds an atom within `cutoff` of some ligand atom: one
 * workgroup per pair, ONE launch per batch.  With the residue number as the group and cutoff 6 this is get_pocket of the
 * reference's data/pocket/prepare_dataset.py and generate_with_protein.py (:85-148).
 *
 * INPUT.  Proteins are concatenated: protein p owns the atoms protein_offset[p] .. protein_offset[p + 1] - 1 of protein_x
 * and protein_group, in file order; protein_group holds dense ids 0 .. G_p - 1 within its protein, assigned by the host.
 * Pair b is the protein pair_protein[b] (one protein serves any number of pairs) and the ligand rows i with
 * ligand_mask[b, i] != 0; rows with mask 0 are never read, whatever they hold.
 *
 * THE RULE.  For protein atom j and ligand atom i:  dx = (double)xp - xl (dy, dz alike),
 * d2 = ((dx*dx) + (dy*dy)) + (dz*dz), each operation a separate fp64 round-to-nearest operation in this order.  Atom j is a
 * CONTACT atom when d2 <= cutoff * cutoff for some i (one fp64 multiply, the comparison not strict); a group is SELECTED
 * when it holds a contact atom; atom j is a POCKET atom when its group is selected.
 *
 *   n_ligand            real ligand rows
 *   n_contact_atoms     contact atoms
 *   n_groups_selected   selected groups
 *   n_pocket            ALL pocket atoms, also those beyond `capacity`
 *   member              uint8 [B,Mmax] by position within the protein: bit 0 contact atom, bit 1 pocket atom; 0 from the
 *                       protein's size on
 *   index               [B,capacity]: the positions within the protein of the first min(n_pocket, capacity) pocket atoms, in
 *                       file order; -1 after them
 *   status              DL_POCKET_TRUNCATED (n_pocket > capacity), or the reasons a pair has no answer:
 *                       DL_POCKET_TOO_LARGE (more than DL_POCKET_MAX_LIGAND ligand atoms; alone, nothing else is looked at),
 *                       DL_POCKET_BAD_PROTEIN (pair_protein outside [0, P), offsets that do not ascend inside [0, M_total],
 *                       or a protein of more than Mmax atoms; alone, no atom is looked at), DL_POCKET_TOO_MANY_GROUPS (a
 *                       group id < 0 or >= DL_POCKET_MAX_GROUPS) and DL_POCKET_NONFINITE (a non-finite coordinate among the
 *                       protein's atoms or the real ligand rows).  Such a pair has n_ligand, every other count 0, member 0
 *                       and index -1; the other pairs of the launch are untouched.
 *
 * The same bits on every run.  Global memory is written with plain stores only, every output element is written, the callee
 * allocates nothing.  A null `args`, a negative B, L, P, M_total, Mmax or capacity, or a cutoff that is not >= 0 return
 * DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer (other than protein_x / protein_group when
 * M_total is 0, ligand_x / ligand_mask when L is 0, `member` when Mmax is 0 and `index` when capacity is 0) returns
 * DL_ERR_BAD_ARG, all before any device work.
 * Not here: parsing, hydrogens, protein cleaning, and the choice of the atoms a data set keeps (pocket.py does that). */
#define DL_POCKET_MAX_LIGAND 256    /* ligand atoms per pair */
#define DL_POCKET_MAX_GROUPS 32768  /* groups per protein */
#define DL_POCKET_NONFINITE 1       /* status bit, same value as DL_CLASH_NONFINITE */
#define DL_POCKET_TOO_LARGE 2       /* status bit, same value as DL_CLASH_TOO_LARGE */
#define DL_POCKET_TOO_MANY_GROUPS 4 /* status bit */
#define DL_POCKET_BAD_PROTEIN 8     /* status bit */
#define DL_POCKET_TRUNCATED 32      /* status bit, same value as DL_FRAG_TRUNCATED */
typedef struct dl_pocket_args {
    int32_t B, L;                   /* pairs; ligand rows per pair */
    int32_t P, M_total;             /* proteins; atoms of all proteins together */
    const float* protein_x;         /* device f32 [M_total,3] (may be NULL when M_total is 0) */
    const int32_t* protein_group;   /* device int32 [M_total] (may be NULL when M_total is 0) */
    const int32_t* protein_offset;  /* device int32 [P+1] */
    const int32_t* pair_protein;    /* device int32 [B] */
    const double* ligand_x;         /* device f64 [B,L,3] (may be NULL when L is 0) */
    const float* ligand_mask;       /* device f32 [B,L] (may be NULL when L is 0) */
    double cutoff;                  /* Angstrom */
    int32_t Mmax;                   /* row width of `member`: at least the largest protein of the launch */
    int32_t capacity;               /* R: positions `index` holds per pair */
    int32_t* n_ligand;              /* device int32 [B] out */
    int32_t* n_contact_atoms;       /* device int32 [B] out */
    int32_t* n_groups_selected;     /* device int32 [B] out */
    int32_t* n_pocket;              /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    uint8_t* member;                /* device uint8 [B,Mmax] out (may be NULL when Mmax is 0) */
    int32_t* index;                 /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
} dl_pocket_args;
int32_t dl_pocket_select(const dl_pocket_args* args, void* stream);

/* ---- circular fingerprints and their Tanimoto similarity (fingerprint.hip) -------------------------------------
 * THE CALLING FORM.  These two entry points take their args struct ALONE, and the stream is the LAST FIELD of the struct
 * (`stream`: a hipStream_t as void*, NULL = the default stream).  The contract is that of every other entry point: inputs
 * are read and outputs written in the order of that stream and of no other (tests/test_gpu_fingerprint.py holds both to
 * it).  Moving the two into the (args, stream) form of the rest of this header, together with their cases in the stream
 * table of tests/test_gpu_streams.py, is a follow-up for whoever next edits that table.
 *
 * FINGERPRINTS.  One workgroup per molecule, ONE launch per batch, on the list dl_perceive_bonds (or dl_aromatic_rings'
 * order_out spliced into it) left on the device.  The list is read with the conventions of dl_molecule_keys: atom k is the
 * k-th row with node_mask != 0; `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with every bond that
 * touches them; an entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation;
 * any other entry is skipped and sets DL_FP_BAD_BOND; entries from min(n_bonds_in, capacity) on are never read (a negative
 * n_bonds_in counts as 0).  `centre_mask` (may be NULL; [B,N] by row like drop_mask) chooses the CENTRES: with it only
 * environments centred on a marked kept atom set bits, while the environments themselves still see the whole kept molecule.
 * The callers pass the linker mask: all samples of one input share their fragments.
 *
 * With mix64 and mix2 as stated at dl_molecule_keys, all arithmetic modulo 2^64:
 *     c_0[i]   = mix2(0x243F6A8885A308D3, type_i + 1)            type: the first largest entry of the one-hot row
 *     c_r+1[i] = mix2(c_r[i], sum over the kept bonds (i, j, order) of mix2(c_r[j], order))
 *     on-bits  = { c_r[i] mod n_bits : 0 <= r <= radius, i kept and a centre }
 * radius is 0 .. DL_FP_MAX_RADIUS (2 is the neighbourhood of ECFP4), n_bits 512, 1024 or 2048, W = n_bits / 32.
 *
 *   bits        uint32 [B,W]: bit k of a fingerprint is bit k % 32 of word k / 32
 *   n_on        bits set
 *   n_atoms     kept atoms
 *   n_centres   kept atoms that are centres
 *   status      the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity, DL_FP_BAD_BOND, and
 *               DL_FP_TOO_LARGE for more than DL_FP_MAX_ATOMS KEPT atoms: bits, n_on and n_centres of that molecule are
 *               then 0 (its list is not looked at) and the other molecules of the launch are untouched.  N itself may be up
 *               to 1024: pockets are dropped, not counted.  The list may be of any length.
 *
 * Integer work only: the same bits on every run, under every order of the list and every renumbering of the atoms.  Global
 * memory is written with plain stores only, every output element is written, the callee allocates nothing.  A null `args`,
 * B < 0, N < 1, N > 1024, nf < 1 or > 16, capacity < 0, a radius outside 0 .. DL_FP_MAX_RADIUS or another n_bits return
 * DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer (other than drop_mask, centre_mask, and
 * `bonds` when capacity is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * What this is NOT: RDKit's Morgan / ECFP fingerprint.  Other invariants (the element and the bond orders only: no charge,
 * hydrogen count, ring membership or isotope), another hash, no removal of duplicate environments, no counts.  Numbers are
 * comparable within this project only. */
#define DL_FP_MAX_ATOMS 256         /* kept atoms per molecule */
#define DL_FP_MAX_RADIUS 4
#define DL_FP_TOO_LARGE 4           /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_FP_BAD_BOND 8            /* status bit, same value as DL_KEYS_BAD_BOND */
typedef struct dl_fingerprint_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* centre_mask;       /* device f32 [B,N] or NULL */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: dl_bonds_args.bonds (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    int32_t radius;                 /* 0 .. DL_FP_MAX_RADIUS */
    int32_t n_bits;                 /* 512, 1024 or 2048 */
    uint32_t* bits;                 /* device uint32 [B,n_bits/32] out */
    int32_t* n_on;                  /* device int32 [B] out */
    int32_t* n_atoms;               /* device int32 [B] out */
    int32_t* n_centres;             /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_fingerprint_args;
int32_t dl_fingerprints(const dl_fingerprint_args* args);

/* TANIMOTO.  Segmented all-pairs similarity of two fingerprint sets, reduced per row of the first: a_bits uint32 [Ma,W]
 * and b_bits uint32 [Mb,W] (W = 16, 32 or 64; 16-byte aligned; they may be the same buffer), G groups given by the device
 * arrays a_offsets[G+1] and b_offsets[G+1].  Row i of A belongs to the group g with a_offsets[g] <= i < a_offsets[g+1];
 * a_offsets must not decrease (the kernel finds g by bisection), and a row in no group has no candidates.  Row i's
 * CANDIDATES are the rows b_offsets[g] <= j < b_offsets[g+1] of B, without j == i when `exclude_diagonal` is set.  Every
 * offset is clamped to [0, M] first, so no offset can make the kernel read outside the two sets; an empty or inverted B
 * range has no candidates.  G = 1 with the whole ranges is plain all-pairs.
 *
 * For a pair c = popcount(a & b) and u = popcount(a) + popcount(b) - c; the similarity is the exact fraction c / u, and
 * 1 / 1 when u is 0 (two empty fingerprints are equal).
 *
 *   nn_index    the candidate of the greatest similarity, fractions compared exactly by cross-multiplication in integers;
 *               of equal ones the lowest j; -1 without candidates
 *   nn_common, nn_union   that pair's c and u (u == 0 is reported as it is); 0 and 0 without candidates
 *   n_pairs     candidates
 *   sum_q20     (may be NULL: then nothing is summed and no division is issued) the sum over the candidates of
 *               u == 0 ? 2^20 : (c << 20) / u, in unsigned integer division
 *
 * Integers throughout: the same bits on every run and for every tiling.  Plain stores only, every output element is
 * written, the callee allocates nothing; the B range of a row is never split, so nothing is combined across workgroups.  A
 * null `args`, a negative Ma, Mb or G, another W, a null or misaligned a_bits (unless Ma is 0) or b_bits (unless Mb is 0),
 * or null offsets (unless G is 0) return DL_ERR_BAD_ARG; then Ma == 0 returns DL_OK without a launch; then a null output
 * other than sum_q20 returns DL_ERR_BAD_ARG, all before any device work.  G == 0 or Mb == 0 still write every row's "no
 * candidates" values.
 * Not here: the dense similarity matrix.  Clusters and diverse subsets: dl_tanimoto_cluster, dl_tanimoto_pick below. */
#define DL_TANIMOTO_TILE 128        /* rows of B a workgroup stages in LDS at a time */
typedef struct dl_tanimoto_args {
    int32_t Ma, Mb, W, G;
    const uint32_t* a_bits;         /* device uint32 [Ma,W] (may be NULL when Ma is 0) */
    const uint32_t* b_bits;         /* device uint32 [Mb,W] (may be NULL when Mb is 0) */
    const int32_t* a_offsets;       /* device int32 [G+1], not decreasing (may be NULL when G is 0) */
    const int32_t* b_offsets;       /* device int32 [G+1] (may be NULL when G is 0) */
    int32_t exclude_diagonal;
    int32_t* nn_index;              /* device int32 [Ma] out */
    int32_t* nn_common;             /* device int32 [Ma] out */
    int32_t* nn_union;              /* device int32 [Ma] out */
    int32_t* n_pairs;               /* device int32 [Ma] out */
    uint64_t* sum_q20;              /* device 64-bit [Ma] out, or NULL */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_tanimoto_args;
int32_t dl_tanimoto_nearest(const dl_tanimoto_args* args);

/* ---- clusters and diverse subsets of fingerprint sets (select.hip) -----------------------------------------------
 * Two sequential-greedy selections over the rows dl_fingerprints wrote, with the similarity of dl_tanimoto_nearest.  Both
 * read a fingerprint set the same way: bits uint32 [M,W] (W = 16, 32 or 64; 16-byte aligned) and the device array
 * offsets[G+1], which does not decrease and splits the rows into G contiguous groups, group g the rows
 * offsets[g] <= i < offsets[g+1].  Every offset is clamped to [0, M] first, so no offset can make a kernel read or write
 * outside the set.  ONE workgroup handles one group, ONE launch takes all groups; there are no atomics and nothing depends
 * on the order in which anything lands; all arithmetic is integer: the same bits on every run.  For a pair of rows
 * c = popcount(a & b) and u = popcount(a | b); the similarity is the exact fraction c / u, and 1 / 1 when u is 0; fractions
 * are compared by cross-multiplication in integers.
 *
 * A group of more than DL_SELECT_MAX_ROWS rows sets DL_SELECT_TOO_LARGE in its status and gets the "nothing" values below,
 * for the group and for each of its rows.  A row in no group (before offsets[0] or from offsets[G] on) gets the "nothing"
 * values too.  Every element of every output is written: the caller may hand over uninitialised memory.  The callee
 * allocates nothing.
 *
 * CLUSTER.  Taylor-Butina sphere exclusion in a fixed order, THIS PROJECT'S OWN statement of the rule after RDKit's
 * Butina.ClusterData(reordering=False); it is NOT promised to reproduce RDKit's output on ties.  The threshold is the
 * rational num / den, 1 <= num <= den <= 65536.  Row j != i of the same group is a NEIGHBOUR of row i when
 * c * den >= num * u (u == 0 included: two empty rows are neighbours).
 *   n_neighbours[i]   the number of such rows; 0 for nothing
 *   The group's rows are walked by n_neighbours descending, among equals by row index ascending.  A row that is not yet
 *   assigned becomes the CENTROID of the next cluster (ids 0, 1, ... in order of creation) and takes every neighbour of its
 *   own that is not yet assigned: a row that neighbours two centroids belongs to the earlier one.
 *   cluster[i]        the group-local id of row i's cluster; -1 for nothing
 *   centroid[i]       the global row index of that cluster's centroid; -1 for nothing
 *   n_clusters[g]     clusters of group g; 0 for nothing
 *   status[g]         0 or DL_SELECT_TOO_LARGE
 *
 * PICK.  MaxMin picking of up to K rows per group, 1 <= K <= DL_SELECT_MAX_ROWS, with THIS PROJECT'S tie rules (NOT
 * RDKit's MaxMinPicker, which starts from a random row).  `first` (may be NULL) is int32 [G], the global row index of each
 * group's first pick; without it the first pick is the group's lowest row.  A first[g] outside its non-empty group sets
 * DL_SELECT_BAD_FIRST and gives that group nothing; an empty group does not look at its first[g].  Every unpicked row i keeps
 * m(i), the greatest similarity to any pick so far, as the (c, u) of that pick, of equal ones the earliest pick.  The next
 * pick is the unpicked row of the SMALLEST m(i), of equal ones the lowest row index.  Picking stops after K picks or when
 * the group is used up.
 *   picks [G,K]                      global row indices in pick order; -1 from n_picked on
 *   pick_common, pick_union [G,K]    the (c, u) of m at the moment of picking (u == 0 is reported as it is); -1 and -1 for
 *                                    the first pick and from n_picked on
 *   n_picked [G]                     picks made; 0 for nothing
 *   status [G]                       0, DL_SELECT_TOO_LARGE or DL_SELECT_BAD_FIRST
 *   pick_rank [M]                    the row's position in its group's pick order; -1 when it was not picked, and for nothing
 *
 * Both: a null `args`, a negative M or G, another W, a threshold or K outside its range, a null or misaligned bits (unless M
 * is 0) or null offsets (unless G is 0) return DL_ERR_BAD_ARG; then M == 0 and G == 0 returns DL_OK without a launch; then a
 * null per-row output (unless M is 0) or per-group output (unless G is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * M == 0 or G == 0 alone still write the outputs there are (every group empty; every row in no group).
 * Not here: groups split over several workgroups, clustering across groups, picking against a reference set, leader,
 * hierarchical and k-medoid clustering, scaffold grouping. */
#define DL_SELECT_MAX_ROWS 4096     /* rows per group */
#define DL_SELECT_TOO_LARGE 4       /* status bit */
#define DL_SELECT_BAD_FIRST 16      /* status bit */
typedef struct dl_cluster_args {
    int32_t M, W, G;
    const uint32_t* bits;           /* device uint32 [M,W] (may be NULL when M is 0) */
    const int32_t* offsets;         /* device int32 [G+1], not decreasing (may be NULL when G is 0) */
    int32_t num, den;               /* the threshold num / den */
    int32_t* cluster;               /* device int32 [M] out */
    int32_t* centroid;              /* device int32 [M] out */
    int32_t* n_neighbours;          /* device int32 [M] out */
    int32_t* n_clusters;            /* device int32 [G] out */
    int32_t* status;                /* device int32 [G] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_cluster_args;
int32_t dl_tanimoto_cluster(const dl_cluster_args* args);

typedef struct dl_pick_args {
    int32_t M, W, G, K;
    const uint32_t* bits;           /* device uint32 [M,W] (may be NULL when M is 0) */
    const int32_t* offsets;         /* device int32 [G+1], not decreasing (may be NULL when G is 0) */
    const int32_t* first;           /* device int32 [G], or NULL: every group starts from its lowest row */
    int32_t* picks;                 /* device int32 [G,K] out */
    int32_t* pick_common;           /* device int32 [G,K] out */
    int32_t* pick_union;            /* device int32 [G,K] out */
    int32_t* n_picked;              /* device int32 [G] out */
    int32_t* status;                /* device int32 [G] out */
    int32_t* pick_rank;             /* device int32 [M] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_pick_args;
int32_t dl_tanimoto_pick(const dl_pick_args* args);

/* ---- pharmacophore features and their feature-map match (pharmacophore.hip) ------------------------------------
 * The reference scores every sample with SC-RDKit = 0.5 * feature-map score + 0.5 * (1 - ShapeProtrudeDist).
 * dl_shape_scores gives the shape half; these two entry points give the feature half: the pharmacophore features of every
 * molecule of a batch, and the Best-mode match of two feature lists.  Both take their arguments alone, the stream as the
 * last field.  THE RULE BELOW IS THIS PROJECT'S OWN, after RDKit's BaseFeatures.fdef and the FeatMapParams defaults.  It is
 * NOT RDKit's feature factory (no SMARTS is matched) and these are NOT RDKit's numbers; tests/pharmacophore_ref.py restates
 * it in plain Python and the kernels agree with that bit for bit.
 *
 * FEATURES.  One workgroup per molecule, ONE launch per batch.  CONVENTIONS, those of dl_aromatic_rings.  Atom k is the k-th
 * row with node_mask != 0; its type is the FIRST largest entry of its one_hot row, its class is feature_class[type]
 * (1 C, 2 N, 3 O, 4 S, 5 P, 6 F, 7 Cl / Br / I, anything else counts as 0) and its default valence default_valence[type].
 * `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with their bonds; `mark_mask` (may be NULL) marks
 * atoms by row.  An entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either
 * orientation; any other entry is skipped and sets DL_PHARM_BAD_BOND.  A repeated pair sets DL_PHARM_BAD_BOND, and its FIRST
 * entry gives the pair its order and its aromatic flag (bond_aromatic[entry] != 0; the output of dl_aromatic_rings for the
 * same list).  Entries from min(n_bonds_in, capacity) on are not read.  "Kept" means: not dropped, both ends for a bond.
 *
 * Per kept atom u, over the distinct kept pairs: deg; val, the sum of the orders; h = max(0, default_valence - val);
 * arom, u ends an aromatic pair; multi, u has a pair of order 2 or 3.  "Neighbour" means the other end of a kept pair.
 *
 *   0 Donor            class N or O with h >= 1
 *   1 Acceptor         class O with !arom and val <= 2; class N with h == 0, val <= 3 and either multi, or deg == 3, !arom
 *                      and no neighbour w with arom(w) or multi(w) (no amide, aniline, sulfonamide, enamine, N-substituted
 *                      pyrrole)
 *   2 PosIonizable     class N with !arom, !multi, val <= 3, deg >= 1, every neighbour of class C and none of them arom or
 *                      multi (an aliphatic amine); class C with !arom, exactly one pair of order 2, which goes to a class N
 *                      atom, no pair of order 3, at least one more class N neighbour by a pair of order 1, and no neighbour
 *                      of class O or S (amidine and guanidine, placed at the carbon)
 *   3 NegIonizable     with T the neighbours of class O and degree 1: at least one of T is joined by a pair of order 2, and
 *                      class C with |T| >= 2 (a carboxylate that the distance table reads as two C=O counts), class P with
 *                      |T| >= 2, class S with |T| >= 3 (a sulfone or sulfonamide does not count)
 *   4 Hydrophobe       class C with deg >= 1 and every neighbour of class C; class 7 with deg == 1; class S with deg == 2,
 *                      !multi, !arom and both neighbours of class C
 *   5 Aromatic         every chordless simple cycle of 5 or 6 kept atoms whose cyclically consecutive pairs are all aromatic
 *                      (chordless: no kept pair, aromatic or not, between two atoms of the cycle that are not consecutive),
 *                      once, in the canonical order of dl_aromatic_rings step 2: from its smallest atom, in the direction
 *                      whose second atom is smaller than its last.  RING ATOMS have two or three aromatic pairs: an atom
 *                      with one, or with more than three, lies in no ring here (dl_aromatic_rings never writes more than
 *                      three; the limit bounds the search).  The position is the centroid
 *                      (((p_0 + p_1) + ...) + p_{n-1}) / (double) n by component, p_k = (double) x in canonical order, fp64,
 *                      contraction off, every operation rounded on its own, then rounded to fp32 once
 *   6 LumpedHydrophobe an Aromatic ring whose atoms are all of class C, at the same position
 *
 * THE LIST.  Atom features first, sorted by (atom number, family): position is the atom's x as given (bit for bit), anchor
 * the atom number.  Ring features follow, the rings sorted lexicographically by their canonical atom sequence, each giving
 * Aromatic and then, if it applies, LumpedHydrophobe: anchor is the ring's smallest atom.  An atom feature is marked when its
 * anchor's row is marked, a ring feature when every atom of the ring is.
 *
 *   family        [B,Fcap]: 0..6; -1 from min(n_features, Fcap) on
 *   anchor        [B,Fcap]: atom number; -1 from there on
 *   position      [B,Fcap,3] f32; 0 from there on
 *   marked        [B,Fcap]: 0 or 1; 0 from there on
 *   n_features    [B]: the true count, which may exceed Fcap
 *   family_count  [B,DL_PHARM_FAMILIES]: the true count of every family
 *   status        [B]: the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative n_bonds_in
 *                 counts as 0), DL_PHARM_BAD_BOND, and the limits.  None disturbs the other molecules of the launch.
 *                 DL_PHARM_TOO_LARGE: more than DL_PHARM_MAX_ATOMS KEPT atoms (N itself may be 1024): nothing is listed,
 *                   every count is 0 and the list of bonds is not read.
 *                 DL_PHARM_MANY_RINGS: more than DL_PHARM_MAX_RINGS rings: the ring features are left out and their two
 *                   counts are 0; the atom features stay.
 *                 DL_PHARM_OVERFLOW: n_features > Fcap; the list holds the first Fcap.
 *                 DL_PHARM_NONFINITE: a kept atom has a NaN or inf coordinate; the features are listed as they are.
 *
 * Integer work apart from the centroid, which is exact in the order given: the same bits on every run and under every order
 * of the list.  Global memory is written with plain stores only, every output element is written, the callee allocates
 * nothing.  A null `args`, B < 0, N < 1, N > 1024, nf < 1, capacity < 0 or Fcap < 0 return DL_ERR_BAD_ARG; then B == 0
 * returns DL_OK without a launch; then a null pointer (other than drop_mask, mark_mask, `bonds` / `bond_aromatic` when
 * capacity is 0, and the four lists when Fcap is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * Limits of the rule: no hydrogens, so h is a count of open valences; no formal charges, so a quaternary N or an N-oxide is
 * not told apart; no SMARTS.  Not here: RDKit's ZnBinder, its alkyl-group lumps (iPr, tBu, chains), feature directions. */
#define DL_PHARM_MAX_ATOMS 256      /* kept atoms per molecule */
#define DL_PHARM_MAX_RINGS 64       /* aromatic rings per molecule */
#define DL_PHARM_FAMILIES 7         /* Donor, Acceptor, PosIonizable, NegIonizable, Hydrophobe, Aromatic, LumpedHydrophobe */
#define DL_PHARM_AROMATIC 5         /* the family of a ring; DL_PHARM_AROMATIC + 1 is LumpedHydrophobe */
#define DL_PHARM_TOO_LARGE 4        /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_PHARM_BAD_BOND 8         /* status bit, same value as DL_KEYS_BAD_BOND */
#define DL_PHARM_MANY_RINGS 16      /* status bit, same value as DL_AROM_MANY_RINGS */
#define DL_PHARM_OVERFLOW 32        /* status bit: n_features > Fcap */
#define DL_PHARM_NONFINITE 64       /* status bit: a kept atom has a NaN / inf coordinate */
typedef struct dl_pharm_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* feature_class;   /* device int32 [nf]: 1 C, 2 N, 3 O, 4 S, 5 P, 6 F, 7 Cl / Br / I, 0 anything else */
    const int32_t* default_valence; /* device int32 [nf]: C 4, N 3, O 2, F 1, S 2, Cl 1, Br 1, I 1, P 3 */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: the list with dl_aromatic_args.order_out as orders (may be NULL when capacity is 0) */
    const int32_t* bond_aromatic;   /* device int32 [B,capacity]: dl_aromatic_args.bond_aromatic (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_aromatic_args.status */
    int32_t Fcap;                   /* features the list holds per molecule */
    int32_t* family;                /* device int32 [B,Fcap] out (may be NULL when Fcap is 0, as the next three) */
    int32_t* anchor;                /* device int32 [B,Fcap] out */
    float* position;                /* device f32 [B,Fcap,3] out */
    int32_t* marked;                /* device int32 [B,Fcap] out */
    int32_t* n_features;            /* device int32 [B] out */
    int32_t* family_count;          /* device int32 [B,DL_PHARM_FAMILIES] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_pharm_args;
int32_t dl_pharmacophore_features(const dl_pharm_args* args);

/* FEATURE MATCH.  For every pair (A = the sample, B = the true molecule) of two feature lists of dl_pharmacophore_features
 * the Best-mode match of RDKit's feature maps: one workgroup per pair.  The lists' capacities Fa and Fb may differ; the counts
 * n_features_a and n_features_b are clamped to [0, Fa] and [0, Fb].  A feature TAKES PART when it lies below its clamped
 * count, its family is 0 .. DL_PHARM_FAMILIES - 1 and, with `marked_only`, its `marked` is not 0.
 *
 * For every B feature j that takes part, over the A features i of the same family that take part:
 * dx = a_x - b_x (dy, dz alike), d2 = ((dx*dx) + (dy*dy)) + (dz*dz), every operation a separate fp32 round-to-nearest
 * operation in exactly this order (as dl_clash_scores computes it).  i is a candidate when d2 < radius2, STRICTLY; the best
 * candidate has the smallest d2 and, of equal ones, the smallest i.  A NaN position is no candidate of anything.
 *
 *   best_index  [B,Fb]: the best candidate of feature j; -1 for none, for a feature that takes no part and from the count on
 *   best_d2     [B,Fb] f32: its d2; +inf wherever best_index is -1
 *   n_a, n_b    [B]: the features of A and of B that take part
 *   n_matched   [B]: the features of B with a candidate
 *
 * The Gaussian is NOT taken on the device, so that the contract stays bit-exact: the caller computes
 * sum_j exp(-best_d2_j) / min(n_a, n_b) in fp64, which is RDKit's width 1, radius 2.5 (radius2 = 6.25) and
 * FeatMapScoreMode.Best divided as the reference's get_FeatureMapScore divides - on this project's features, NOT RDKit's.
 * Plain stores only, every output element is written, the callee allocates nothing.  A null `args`, a negative B, Fa or Fb,
 * or a radius2 that is negative or NaN return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer
 * (other than A's lists when Fa is 0, and B's lists and the two per-feature outputs when Fb is 0) returns DL_ERR_BAD_ARG,
 * all before any device work.
 * Not here: the other score modes (All, Closest), feature directions, any alignment of the two molecules. */
typedef struct dl_feature_match_args {
    int32_t B, Fa, Fb;
    const int32_t* family_a;        /* device int32 [B,Fa] (may be NULL when Fa is 0, as the next two) */
    const float* position_a;        /* device f32 [B,Fa,3] */
    const int32_t* marked_a;        /* device int32 [B,Fa] */
    const int32_t* n_features_a;    /* device int32 [B] */
    const int32_t* family_b;        /* device int32 [B,Fb] (may be NULL when Fb is 0, as the next two) */
    const float* position_b;        /* device f32 [B,Fb,3] */
    const int32_t* marked_b;        /* device int32 [B,Fb] */
    const int32_t* n_features_b;    /* device int32 [B] */
    float radius2;                  /* square of the cut-off, A^2 (2.5 * 2.5) */
    int32_t marked_only;
    int32_t* best_index;            /* device int32 [B,Fb] out (may be NULL when Fb is 0) */
    float* best_d2;                 /* device f32 [B,Fb] out (may be NULL when Fb is 0) */
    int32_t* n_a;                   /* device int32 [B] out */
    int32_t* n_b;                   /* device int32 [B] out */
    int32_t* n_matched;             /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_feature_match_args;
int32_t dl_feature_match(const dl_feature_match_args* args);

/* ---- explicit hydrogens with 3D positions (hydrogens.hip) --------------------------------------------------------
 * Every molecule this project writes is a heavy-atom skeleton: the models have no hydrogen type.  This entry point turns
 * the open valences of a bond graph with orders (dl_perceive_bonds, or the Kekule orders of dl_aromatic_rings) into
 * hydrogen atoms with coordinates: one workgroup per molecule, ONE launch per batch, no host round trip.  It takes its
 * arguments alone, the stream as the last field, as dl_pharmacophore_features does.  THE RULE BELOW IS THIS PROJECT'S OWN.  It is NOT RDKit's AddHs with addCoords and NOT OpenBabel's; tests/hydrogens_ref.py restates it in
 * plain Python and the kernel agrees with that bit for bit.
 *
 * CONVENTIONS, those of dl_aromatic_rings.  Atom k is the k-th row with node_mask != 0; its type t is the FIRST largest
 * entry of its one_hot row.  `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with their bonds.  An
 * entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation; any other entry
 * is skipped and sets DL_HYDRO_BAD_BOND.  A repeated pair sets DL_HYDRO_BAD_BOND too and counts once, with its FIRST
 * entry's order.  Entries from min(n_bonds_in, capacity) on are not read.  "Kept" means: not dropped, both ends for a bond;
 * a "neighbour" is the other end of a kept pair.
 *
 * Per kept atom a of type t:
 * 1. d is the number of its neighbours, vs the sum of the orders of those pairs.
 * 2. h0 = max(0, default_valence[t] - vs).  An over-valent atom (a sulfone S, a five-bonded C) gets none.
 * 3. GEOMETRY CLASS, by the first condition that holds.  T2 (linear, 2 sites): a pair of order 3, or two or more of order
 *    2.  T3 (trigonal, 3 sites): exactly one pair of order 2; or atom_planar[a] != 0 with d == 2 and h0 == 1 (`atom_planar`,
 *    by atom number, may be NULL: the atom_aromatic of dl_aromatic_rings puts a pyrrole N-H in plane).  T4 (tetrahedral,
 *    4 sites): otherwise.  The count is h = min(h0, max(0, sites - d)).
 * 4. L = xh_length[t], in A: C 1.09, N 1.01, O 0.96, F 0.92, S 1.34, Cl 1.27, Br 1.41, I 1.61, P 1.42.
 *
 * ARITHMETIC.  fp64 on (double) x, contraction off, every + - * / and sqrt rounded on its own in the order written, as
 * step 3 of dl_aromatic_rings.  v . w is (v_x*w_x + v_y*w_y) + v_z*w_z; v x w is (v_y*w_z - v_z*w_y, v_z*w_x - v_x*w_z,
 * v_x*w_y - v_y*w_x); v / |v| is n = sqrt(v . v), then (v_x/n, v_y/n, v_z/n); -v / |v| negates those quotients; sums,
 * differences and products with a scalar go by component.  EPS = 1e-6.  u_k = (x_k - x_a) / |x_k - x_a| for the
 * neighbours k of a in increasing atom number.  perp(u): m is the axis with the smallest |u_m| (the lowest m of equal ones),
 * v = e_m - u_m * u (v_j = [j == m] - u_m * u_j), and perp(u) = v / |v|.  The constants are the doubles nearest to
 * sqrt(3) = 0x1.bb67ae8584caap+0, sqrt(2/3) = 0x1.a20bd700c2c3ep-1, sqrt(8)/3 = 0x1.e2b7dddfefa67p-1 and
 * sqrt(3)/2 = 0x1.bb67ae8584caap-1.
 *
 * DIRECTIONS.
 *   T4, d = 3   s = (u1 + u2) + u3.  If s . s > EPS: -s / |s|.  Otherwise w = (u2 - u1) x (u3 - u1), and w / |w| when
 *               w . w > EPS, else perp(u1).
 *   d = 2       s = u1 + u2, c = u1 x u2.  If s . s <= EPS (anti-parallel): b = perp(u1), n = u1 x b.  Otherwise
 *               b = -s / |s|, and n = c / |c| when c . c > EPS, else perp(u1).  T3: b.  T4: b / sqrt(3) + sqrt(2/3) * n,
 *               then b / sqrt(3) - sqrt(2/3) * n; the first h of them.
 *   d = 1       k is the neighbour, r the smallest-numbered neighbour of k other than a.  w = x_r - x_k,
 *               p = w - (w . u1) * u1.  e1 = -p / |p| when r exists and p . p > EPS * (w . w), else perp(u1) - negated
 *               when there is no r and a > k: perp(u) = perp(-u), so the two atoms of a molecule of two heavy atoms would
 *               choose the same e1 and eclipse each other; negated at the second of them, ethane comes out staggered.
 *               e2 = u1 x e1.
 *               T4: -(u1 / 3) + (sqrt(8)/3) * (cos * e1 + sin * e2) with (cos, sin) = (1, 0), (-0.5, sqrt(3)/2),
 *               (-0.5, -sqrt(3)/2), both products formed for each; the first h.  The first is anti to r (staggered).
 *               T3: -(u1 / 2) + (sqrt(3)/2) * e1, then -(u1 / 2) - (sqrt(3)/2) * e1; the first h.  The first is trans
 *               to r.  T2: -u1.
 *   T4, d = 0   g = 1 / sqrt(3); the first h of (g, g, g), (g, -g, -g), (-g, g, -g), (-g, -g, g).
 * A hydrogen sits at x_a + L * direction by component.  Two atoms at one point divide by zero: the positions that depend
 * on them are not finite, and nothing is flagged.
 *
 * THE LIST.  Hydrogens are listed by parent atom number, within a parent in the order above.
 *
 *   n_h       [B]: the true count, which may exceed Hcap
 *   h_count   [B,N] by atom number, written in full: h; 0 for dropped atoms and from the atom count on
 *   h_parent  [B,Hcap]: the parent's atom number; written up to min(n_h, Hcap) and left UNTOUCHED from there on
 *   h_x       [B,Hcap,3] f64, A: likewise
 *   status    [B]: the bits of `status_in` (may be NULL: none), plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative
 *             n_bonds_in counts as 0), DL_HYDRO_BAD_BOND, and the limits.  None disturbs the other molecules of the launch.
 *             DL_HYDRO_TOO_LARGE: more than DL_HYDRO_MAX_ATOMS KEPT atoms (N itself may be 1024): nothing is listed, every
 *               count is 0, and neither the list of bonds nor the coordinates are looked at.
 *             DL_HYDRO_OVERFLOW: n_h > Hcap; the list holds the first Hcap.
 *             DL_HYDRO_NONFINITE: a kept atom has a NaN or inf coordinate; the molecule gets no hydrogens (every count 0).
 *
 * The same bits on every run and under every order of the list.  Global memory is written with plain stores only; the callee
 * allocates nothing and needs no workspace.  A null `args`, B < 0, N < 1, N > 1024, nf < 1, capacity < 0 or Hcap < 0 return
 * DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer (other than drop_mask, atom_planar,
 * status_in, stream, `bonds` when capacity is 0, and the two lists when Hcap is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * Limits of the rule: an amide or aniline N comes out pyramidal; no formal charges, so a carboxylate is written as an acid and
 * an ammonium as an amine; P and S above their default valence get none; the torsions of -OH and -NH2 are the staggered
 * default, not oriented towards a pocket.  Not here: protonation states, energy minimisation, hydrogens in any score. */
#define DL_HYDRO_MAX_ATOMS 256      /* kept atoms per molecule */
#define DL_HYDRO_TOO_LARGE 4        /* status bit, same value as DL_PHARM_TOO_LARGE */
#define DL_HYDRO_BAD_BOND 8         /* status bit, same value as DL_PHARM_BAD_BOND */
#define DL_HYDRO_OVERFLOW 32        /* status bit, same value as DL_PHARM_OVERFLOW: n_h > Hcap */
#define DL_HYDRO_NONFINITE 64       /* status bit, same value as DL_PHARM_NONFINITE */
typedef struct dl_hydrogens_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const int32_t* atom_planar;     /* device int32 [B,N] by atom number, or NULL: dl_aromatic_args.atom_aromatic */
    const int32_t* default_valence; /* device int32 [nf]: C 4, N 3, O 2, F 1, S 2, Cl 1, Br 1, I 1, P 3 */
    const double* xh_length;        /* device f64 [nf]: the X-H bond lengths, A */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B] or NULL: dl_bonds_args.status or dl_aromatic_args.status */
    int32_t Hcap;                   /* hydrogens the list holds per molecule */
    int32_t* n_h;                   /* device int32 [B] out */
    int32_t* h_count;               /* device int32 [B,N] out */
    int32_t* h_parent;              /* device int32 [B,Hcap] out (may be NULL when Hcap is 0, as the next) */
    double* h_x;                    /* device f64 [B,Hcap,3] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_hydrogens_args;
int32_t dl_add_hydrogens(const dl_hydrogens_args* args);

/* ---- internal geometry of a molecule: bond lengths, bond angles, internal clashes (pose_checks.hip) ----------------
 * Is the molecule's own 3D geometry physically plausible?  One workgroup per molecule, ONE launch per batch, on the bond list
 * with orders that dl_perceive_bonds or dl_aromatic_rings left on the device; the entry point takes its arguments alone, the
 * stream as the last field, as dl_add_hydrogens does.  THE RULE BELOW IS THIS PROJECT'S OWN, after the idea of PoseBusters'
 * intramolecular checks (Buttenschoen, Morris & Deane, Chem. Sci. 2024).  It is NOT PoseBusters and gives NOT PoseBusters'
 * numbers: there is no RDKit distance-geometry bounds matrix, no hydrogens, no energy, no ring or double-bond flatness term.
 * tests/pose_checks_ref.py restates it in plain Python and the kernel agrees with that bit for bit.
 *
 * CONVENTIONS, those of dl_add_hydrogens.  Atom k is the k-th row with node_mask != 0; its type t is the FIRST largest
 * entry of its one_hot row.  `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with their bonds.  An
 * entry (i, j, order) is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation; any other entry
 * is skipped and sets DL_POSE_BAD_BOND.  A repeated pair sets DL_POSE_BAD_BOND too and counts once, with its FIRST
 * entry's order.  Entries from min(n_bonds_in, capacity) on are not read.  "Kept" means: not dropped, both ends for a bond;
 * a "neighbour" is the other end of a kept pair.  `mark_mask` (may be NULL: nothing is marked) marks atoms by row - the
 * linker; an item (a bond, an angle, a far pair) is MARKED when at least one of its atoms is.
 *
 * ARITHMETIC.  fp64 on (double) x, contraction off, every + - * / and sqrt rounded on its own in the order written, as in
 * dl_add_hydrogens: v = x_j - x_a by component, v . w = (v_x*w_x + v_y*w_y) + v_z*w_z.  Every threshold is formed by the host
 * in fp64 and passed as a table; the kernel only compares.
 *
 * 1. BOND LENGTHS.  For every kept pair (a, j) of order k with types (s, t): d2 = v . v with v = x_j - x_a, a < j.
 *    lo2 = length_bounds2[s][t][k-1][0] and hi2 = length_bounds2[s][t][k-1][1], in A^2: ((lo * L0)^2, (hi * L0)^2) of the typical
 *    length L0 of that order between those elements (the host's const.BOND_LENGTHS / 100; lo, hi = 0.75, 1.25 by default,
 *    PoseBusters' factors).  A pair with both bounds 0 has no typical length: it counts as UNTABLED and is not checked.
 *    Otherwise it is checked, SHORT when d2 < lo2 and LONG when d2 > hi2, both strict.
 * 2. BOND ANGLES.  The centre a is a kept atom with 2 <= d <= 4 neighbours; n2 and n3 count its pairs of order 2 and 3.  Its
 *    class is the first that holds.  LINEAR (0): d == 2, and n3 >= 1 or n2 == 2.  TRIGONAL (1): d <= 3 and n2 >= 1, or
 *    atom_planar[a] != 0 (by atom number, may be NULL: the atom_aromatic of dl_aromatic_rings).  TETRAHEDRAL (2): otherwise.
 *    This is not the class rule of dl_add_hydrogens: a sulfone S with four neighbours is tetrahedral here.  Atoms with d > 4
 *    are not checked.  Every pair of neighbours j < k of a is one angle, except when j and k are bonded (a three-ring) or
 *    share a neighbour other than a (a four-ring).  With u = x_j - x_a and v = x_k - x_a,
 *    c = (u . v) / sqrt((u . u) * (v . v)), and the angle is BAD when c < angle_cos[class][0] or c > angle_cos[class][1]:
 *    the host's cos(theta0 + tol) and cos(theta0 - tol) for theta0 = 180, 120 and acos(-1/3) degrees and tol = 25 by default,
 *    -2 where theta0 + tol reaches 180 (and 2 where theta0 - tol reaches 0), which never fires.  A zero-length u or v gives a
 *    NaN that no comparison flags: two atoms at one point are caught as a short bond or as a clash instead, not here.
 * 3. INTERNAL CLASHES.  The FAR PAIRS are the unordered pairs of kept atoms with NO path of three or fewer bonds between
 *    them: four or more bonds apart, or in different pieces.  A far pair (a, b), a < b, with types (s, t) CLASHES when
 *    d2 < clash2[s][t] and that entry is positive: the host's (scale * (R[s] + R[t]))^2 over Bondi's radii, scale 0.75 by
 *    default, in A^2.
 *
 *   counts      [B][2][8], written in full.  Row 0: all items; row 1: the marked ones.  The eight values: bonds checked, bonds
 *               untabled, short, long, angles checked, angles bad, far pairs checked, clashes.
 *   atom_flags  [B][N] by atom number, written in full: bit 1 an end of a short or long bond, bit 2 the centre of a bad angle,
 *               bit 4 in a clashing pair; 0 for dropped atoms and from the atom count on.
 *   status      [B]: the bits of `status_in` (may be NULL: none), plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative
 *               n_bonds_in counts as 0), DL_POSE_BAD_BOND, and the limits.  None disturbs the other molecules of the launch.
 *               DL_POSE_TOO_LARGE: more than DL_POSE_MAX_ATOMS KEPT atoms (N itself may be 1024): every count and flag is 0,
 *                 and neither the list of bonds nor the coordinates are looked at.
 *               DL_POSE_NONFINITE: a kept atom has a NaN or inf coordinate; every count and flag is 0.
 *
 * The same bits on every run and under every order of the list: every sum is a sum of integers.  Global memory is written
 * with plain stores only; the callee allocates nothing and needs no workspace.  A null `args`, B < 0, N < 1, N > 1024, nf < 1
 * or capacity < 0 return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without a launch; then a null pointer (other than drop_mask,
 * mark_mask, atom_planar, status_in, stream, and `bonds` when capacity is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * Limits of the rule: heavy atoms only; three- and four-ring angles are exempt, not checked against their own ideals; an
 * amide or aniline N is held to the tetrahedral angle (its 120 degrees are within the default tolerance); the typical
 * lengths know no aromatic order, so a Kekule ring bond is compared as the single or double bond its order says.  Not here:
 * flatness of rings and double bonds, torsions, strain energies, minimisation. */
#define DL_POSE_MAX_ATOMS 256       /* kept atoms per molecule */
#define DL_POSE_TOO_LARGE 4         /* status bit, same value as DL_HYDRO_TOO_LARGE */
#define DL_POSE_BAD_BOND 8          /* status bit, same value as DL_HYDRO_BAD_BOND */
#define DL_POSE_NONFINITE 64        /* status bit, same value as DL_HYDRO_NONFINITE */
#define DL_POSE_COUNTS 8            /* values per row of `counts` */
typedef struct dl_pose_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* atom_planar;     /* device int32 [B,N] by atom number, or NULL: dl_aromatic_args.atom_aromatic */
    const double* length_bounds2;   /* device f64 [nf,nf,3,2]: squared lower and upper bond length, A^2; 0, 0: no entry */
    const double* angle_cos;        /* device f64 [3,2]: lowest and highest cosine of the classes LINEAR, TRIGONAL, TETRAHEDRAL */
    const double* clash2;           /* device f64 [nf,nf]: squared clash distance, A^2 */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B] or NULL: dl_bonds_args.status or dl_aromatic_args.status */
    int32_t* counts;                /* device int32 [B,2,8] out */
    int32_t* atom_flags;            /* device int32 [B,N] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_pose_args;
int32_t dl_pose_checks(const dl_pose_args* args);

/* ---- restrained clean-up of the marked atoms: a FIRE minimisation in fp64 (relax.hip) ----------------------------------
 * Moves the MOVABLE atoms of every molecule - the linker - down a restraint energy for a fixed number of FIRE steps (Bitzek,
 * Koskinen, Gaehler, Moseler & Gumbsch, PRL 97, 170201 (2006)) with the topology frozen at the bond list it is given.  One
 * 256-thread workgroup per molecule, ONE launch per batch, the stream as the last field, as dl_pose_checks.  THE RULE BELOW IS
 * THIS PROJECT'S OWN.  It is NOT UFF, NOT MMFF and NOT RDKit's or OpenBabel's optimiser, its energies are in units of its own
 * and compare runs of this project with each other only.  tests/relax_ref.py restates it in numpy and the kernel agrees with
 * that in every output bit.
 *
 * CONVENTIONS: atoms, kept atoms, bonds (first entry of a repeated pair, DL_POSE_BAD_BOND), drop_mask, mark_mask,
 * atom_planar and status_in exactly as for dl_pose_checks; at most DL_RELAX_MAX_ATOMS kept atoms, N <= 1024.  Kept atoms are
 * numbered among themselves in row order (the KEPT INDEX); "lower" and "ascending" below mean by kept index.
 * `bond_aromatic` ([B,capacity], may be NULL: none) flags list entries, as dl_aromatic_rings writes it; the first entry of a
 * pair gives the pair its flag as it gives it its order.  MOVABLE: kept and marked; with mark_mask NULL every kept atom.
 * WALL atoms: the rows with node_mask != 0 and drop_mask != 0 in row order (their WALL RANK), when use_wall != 0; none
 * otherwise.  The type of an atom is the first largest entry of its one_hot row.
 *
 * ARITHMETIC.  fp64 on (double) x, contraction off, every + - * / and sqrt rounded on its own in the order written;
 * v . w = (v_x*w_x + v_y*w_y) + v_z*w_z; no transcendental function.  Products with a vector are by component.
 *
 * ENERGY.  Only items that touch a movable atom count, each once.
 * 1. BONDS.  A kept pair (a, j), a < j, types (s, t): L0 = aromatic_length0[s][t] when flagged, else
 *    length0[s][t][order-1]; L0 == 0: no term.  w = x_j - x_a, d = sqrt(w . w); d == 0: no term.
 *    e = k_bond * ((d - L0) * (d - L0)).  Force on a: g * w with g = ((2 * k_bond) * (d - L0)) / d; on j the same with
 *    w = x_a - x_j.
 * 2. ANGLES.  Centres, classes and the pairs (j, k), j < k, of a centre a as in dl_pose_checks rule 2, three- and four-rings
 *    exempt; exempt too when a neighbour of j other than a is bonded to a neighbour of k other than a (a five-ring).
 *    p = x_j - x_a, q = x_k - x_a; p . p == 0 or q . q == 0: no term.  den = sqrt((p . p) * (q . q)), c = (p . q) / den,
 *    c0 = ideal_cos[class], e = k_angle * ((c - c0) * (c - c0)).  With mg = (2 * k_angle) * (c0 - c), inv = 1 / den,
 *    pa = c / (p . p), pb = c / (q . q): F_j = mg * (q * inv - p * pa), F_k = mg * (p * inv - q * pb), F_a = -(F_j + F_k).
 * 3. INTERNAL REPULSION over the FAR PAIRS of dl_pose_checks rule 3.  For atom u and partner p: w = x_u - x_p, d2 = w . w,
 *    R2 = reach2[type of the lower][type of the higher]; when d2 < R2 (strict): s = 1 - d2 / R2, e = k_rep * (s * s), force
 *    on u: g * w with g = ((4 * k_rep) * s) / R2.
 * 4. WALL.  The same form between every movable atom u and every wall atom, with k_wall and wall_reach2[type of u][type of
 *    the wall atom].  A wall atom with a NaN or inf coordinate fails the comparison and contributes nothing.
 * 5. RESTRAINT.  Every movable atom: w = x - x0, e = k_pos * (w . w), force (2 * k_pos) * (x0 - x); x0 is its input position.
 *
 * FORCE ON A MOVABLE ATOM u, by component.  acc = +0.0; then, each as acc = acc + term: its bond terms by neighbour ascending;
 * the angle terms with u as centre in pair order (k ascending, then j ascending); the angle terms with u as an end, by centre
 * ascending, then by other end ascending.  The far-pair sum and the wall sum are each split into 64 partials: partner p (kept
 * index, or wall rank) belongs to partial p mod 64, and each partial sums its partners ascending from +0.0.  The 64 partials
 * are combined by the balanced tree over adjacent elements, T'[i] = T[2i] + T[2i+1].  F = (acc + (far + wall)) + restraint.
 * The sums over atoms (F . v, F . F, v . v and the energies) are the same tree over 256 slots by kept index, +0.0 in the slots
 * of atoms that do not contribute.
 *
 * ITERATION.  dt = dt0, alpha = alpha0, n_pos = 0, v = 0.  For `steps` steps: (1) the forces; a non-finite component ends the
 * run with DL_RELAX_DIVERGED.  (2) f = the largest |F| = sqrt(F . F) of a movable atom (a length: the
 * same in every frame, which a largest component is not; an F . F that overflows makes f +inf, no divergence); f < f_tol ends
 * the run.  (3) P = sum F . v, ff = sum F . F,
 * vv = sum v . v.  (4) P > 0: n_pos += 1, v = (1 - alpha) * v + ((alpha * sqrt(vv)) / sqrt(ff)) * F, and when n_pos > n_min:
 * dt = min(dt * f_inc, dt_max), alpha = alpha * f_alpha.  (5) otherwise n_pos = 0, v = 0, dt = dt * f_dec, alpha = alpha0.
 * (6) v = v + dt * F, s = dt * v.  (7) l = sqrt(s . s); when l > max_step: s = s * (max_step / l).  (8) x = x + s; one more
 * step is done.  A non-finite x after the last step is DL_RELAX_DIVERGED too.
 *
 *   x_out       [B][N][3], written in full: the bits of x, except the movable atoms of a molecule that ran, whose fp64
 *               positions are rounded to fp32 once.
 *   energy      [B][2][5]: bonds, angles, repulsion, wall, restraint at the input and at the final positions.  Per term: every
 *               OWNER's items summed from +0.0 in the force order (a bond is owned by its lower end, neighbours ascending; an
 *               angle by its centre; a far pair by its lower atom, in 64 partials as above; a wall pair and a restraint by
 *               the movable atom), then the tree over the 256 slots.
 *   steps_done  [B]: steps done; f_max [B]: the last f (0 when no step began); moved2 [B]: the largest |x - x0|^2 (fp64).
 *   status      [B]: the bits of status_in (may be NULL), DL_BONDS_OVERFLOW, DL_POSE_BAD_BOND, and
 *               DL_POSE_TOO_LARGE / DL_POSE_NONFINITE (values and meaning of dl_pose_checks): x_out = x, every other output
 *                 is 0, no coordinate (TOO_LARGE: nor the list) is looked at;
 *               DL_RELAX_DIVERGED: x_out = x; energy[0] and steps_done stand, energy[1], f_max and moved2 are 0.
 *               A molecule with no movable atom succeeds with steps_done 0.  None disturbs the other molecules.
 *
 * Global memory is written with plain stores only; the callee allocates nothing and needs no workspace.  A null `args`, B < 0,
 * N < 1, N > 1024, nf < 1, capacity < 0, steps < 0 or steps > DL_RELAX_MAX_STEPS return DL_ERR_BAD_ARG; then B == 0 returns
 * DL_OK without a launch; then a null pointer (other than drop_mask, mark_mask, atom_planar, bond_aromatic, status_in, stream,
 * and `bonds` when capacity is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * Limits: heavy atoms only, no hydrogens in the energy; no torsion, planarity or electrostatic term; the wall is the dropped
 * rows of the batch, not a whole protein; a planar ring that is not flagged aromatic keeps its Kekule lengths; the topology
 * is frozen during the run; at most 256 kept atoms. */
#define DL_RELAX_MAX_ATOMS 256      /* kept atoms per molecule */
#define DL_RELAX_MAX_STEPS 1000
#define DL_RELAX_DIVERGED 128       /* status bit: a force or a position turned non-finite */
#define DL_RELAX_TERMS 5            /* values per row of `energy` */
typedef struct dl_relax_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* atom_planar;     /* device int32 [B,N] by atom number, or NULL */
    const double* length0;          /* device f64 [nf,nf,3]: typical length per order, A; 0: no term */
    const double* aromatic_length0; /* device f64 [nf,nf]: length of a bond flagged aromatic, A; 0: no term */
    const double* ideal_cos;        /* device f64 [3]: ideal cosine of LINEAR, TRIGONAL, TETRAHEDRAL */
    const double* reach2;           /* device f64 [nf,nf]: squared reach of the internal repulsion, A^2 */
    const double* wall_reach2;      /* device f64 [nf,nf]: squared reach of the wall, [movable][wall], A^2 */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B] */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* bond_aromatic;   /* device int32 [B,capacity] or NULL: dl_aromatic_args.bond_aromatic */
    const int32_t* status_in;       /* device int32 [B] or NULL */
    int32_t use_wall, steps, n_min;
    double k_bond, k_angle, k_rep, k_wall, k_pos;
    double dt0, dt_max, alpha0, f_inc, f_dec, f_alpha, max_step, f_tol;
    float* x_out;                   /* device f32 [B,N,3] out */
    double* energy;                 /* device f64 [B,2,5] out */
    int32_t* steps_done;            /* device int32 [B] out */
    double* f_max;                  /* device f64 [B] out */
    double* moved2;                 /* device f64 [B] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_relax_args;
int32_t dl_relax_molecules(const dl_relax_args* args);

/* ---- canonical atom ranks and a canonical code of a perceived batch (canon.hip) -------------------------------------
 * A canonical labelling of the bond graph dl_perceive_bonds left on the device, by an individualisation-refinement search
 * over the colour refinement of dl_molecule_keys: one 256-thread workgroup per molecule, ONE launch per batch, everything per
 * molecule in LDS, the stream as the last field, as dl_relax_molecules.  The key of dl_molecule_keys is 1-WL and cannot tell cubane from cuneane; the code below is the hash of a
 * labelled form, so two molecules with equal codes are the same graph up to a 64-bit collision, and the ranks are the atom
 * order molecule_builder.smiles writes a string from.  THE RULE BELOW IS THIS PROJECT'S OWN: NOT RDKit's canonical ranks, and
 * the strings are NOT RDKit's canonical SMILES.  tests/canon_ref.py restates it in plain Python and numpy and the kernel agrees with
 * that in every output bit.  "Equal codes exactly for the same graph" is checked by the atlas sweep (tests/test_atlas_host.py,
 * tests/test_gpu_atlas.py) against networkx's isomorphism test: every graph of up to 7 atoms and seeded colourings of those of
 * up to 6, under renumbering, and vertex-transitive cage graphs, the 4x4 rook's graph and the Shrikhande graph among them.
 *
 * THE GRAPH is the one dl_molecule_keys reads: atom k is the k-th row with node_mask != 0; `drop_mask` (may be NULL) removes
 * atoms AFTER that numbering together with every bond that touches them; the kept atoms are numbered among themselves in row
 * order (the KEPT INDEX; "lowest" and "ascending" below mean by kept index).  The type of an atom is the first largest entry of
 * its one_hot row.  An entry (i, j, order) of the list is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either
 * orientation; any other entry is skipped and sets DL_CANON_BAD_BOND.  A pair that is listed more than once also sets
 * DL_CANON_BAD_BOND, and every one of its entries counts as a bond of its own wherever the rule sums over "the kept bonds" or
 * counts an atom's bonds (as in dl_molecule_keys).  n is the number of kept atoms.  mix64, mix2 and the two seeds are those of
 * dl_molecule_keys above (SEED_COLOUR = 0x243F6A8885A308D3, SEED_KEY = 0x13198A2E03707344); all arithmetic is modulo 2^64.
 *
 *   refine(c)   exactly n rounds of c'[i] = mix2(c[i], sum over the kept bonds (i, j, o) of mix2(c[j], o)).  The count
 *               depends on n alone; there is no settle test.
 *   ranks       rank[i] = the number of kept atoms whose colour is strictly smaller than c[i]: tied atoms share a rank.
 *   root        c[i] = mix2(SEED_COLOUR, type_i + 1); refine; rank.
 *   leaf        a node whose ranks are all distinct.
 *   branching   any other node takes the CELL of tied atoms with the smallest rank.  For each member v of the cell, in
 *               ascending order, the child is c[i] = mix2(SEED_COLOUR, 2 * rank[i] + (i == v ? 0 : 1)); refine; rank; the
 *               children are searched depth first.
 *   twins       when every member of the cell has exactly one kept bond, all to the same atom with the same order (the F of
 *               a CF3, the methyls of a tert-butyl, the O of an SO2), only the lowest member is taken: any two members are
 *               exchanged by an automorphism, so the other branches could only reproduce the same form.  A twin step is no
 *               branching level.
 *   depth       a path that already has DL_CANON_MAX_DEPTH (32) branching levels above it does not branch at a cell that
 *               is no twin cell: it takes the lowest member only, and sets DL_CANON_BUDGET.
 *   (guard)     every step down a path splits a cell, so a path has fewer than n steps.  Should two different 64-bit colours
 *               ever collide and merge cells again, a path ends after n steps as if it were a leaf and sets DL_CANON_BUDGET;
 *               the ranks are then no permutation.  No such input is known.
 *   leaf code   mix2(mix2(SEED_KEY, A), Bsum);  A = sum over the kept atoms of mix2(rank[i], type_i + 1);  Bsum = sum over
 *               the kept bonds of mix2(mix2(min(rank_i, rank_j), max(rank_i, rank_j)), order).
 *   best        the leaf with the smallest code, compared as unsigned integers, wins; on equal codes the earlier leaf stays.
 *   leaves      the search stops when `max_leaves` leaves have been evaluated and another one would be: that sets
 *               DL_CANON_BUDGET.  A search that ends by itself after exactly max_leaves leaves does not set it.
 *
 *   rank        [B,N] by atom number as `colour` of dl_molecule_keys: the best leaf's ranks, a permutation of 0..n-1 over
 *               the kept atoms; -1 for a dropped atom and from the atom count on.
 *   code        [B] the best leaf's code; n = 0 gives mix2(mix2(SEED_KEY, 0), 0), one leaf and no ranks.
 *   n_leaves    [B] leaves evaluated (at least 1).
 *   status      the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative n_bonds_in counts as
 *               0), DL_CANON_BAD_BOND, DL_CANON_BUDGET (ranks are still a valid permutation, merely not promised to be
 *               canonical), and DL_CANON_TOO_LARGE for more than DL_CANON_MAX_ATOMS kept atoms or more than
 *               DL_CANON_MAX_BONDS kept list entries: rank is then all -1, code 0 and n_leaves 0 (with too many
 *               atoms the list is not looked at and DL_CANON_BAD_BOND is not added; with too many entries it is added for
 *               an entry that is no bond, and repeated pairs are not looked for).
 *
 * Integer work only, commutative sums: the same bits on every run and under every order and orientation of the list.  Global
 * memory is written with plain stores only, every output element is written, the callee allocates nothing and needs no
 * workspace.  The work is bounded by max_leaves * (n + DL_CANON_MAX_DEPTH) refinements of n rounds each; molecule-like
 * graphs need a handful of leaves (profiles/canon/README.md).  A null `args`, B < 0, N < 1, N > 1024, nf < 1, nf > 256,
 * capacity < 0, max_leaves < 1 or max_leaves > DL_CANON_MAX_LEAVES return DL_ERR_BAD_ARG; then B == 0 returns DL_OK without
 * a launch; then a null pointer (other than drop_mask, stream, and `bonds` when capacity is 0) returns DL_ERR_BAD_ARG, all before any
 * device work.
 * Not here: stereo, charges, aromatic perception (orders are taken as the list has them, so two Kekule forms of one ring are
 * two graphs), hydrogens. */
#define DL_CANON_MAX_ATOMS 256      /* kept atoms per molecule */
#define DL_CANON_MAX_BONDS 2048     /* kept list entries per molecule */
#define DL_CANON_MAX_DEPTH 32       /* branching levels of a path */
#define DL_CANON_MAX_LEAVES 65536   /* largest max_leaves */
#define DL_CANON_TOO_LARGE 4        /* status bit, same value as DL_KEYS_TOO_LARGE */
#define DL_CANON_BAD_BOND 8         /* status bit, same value as DL_KEYS_BAD_BOND */
#define DL_CANON_BUDGET 256         /* status bit: the leaf or the depth budget ended or narrowed the search */
typedef struct dl_canon_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3]: dl_bonds_args.bonds (may be NULL when capacity is 0) */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    int32_t max_leaves;             /* 1..DL_CANON_MAX_LEAVES; the Python layer's default is 256 */
    int32_t* rank;                  /* device int32 [B,N] out */
    uint64_t* code;                 /* device 64-bit [B] out */
    int32_t* n_leaves;              /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_canon_args;
int32_t dl_canonical_ranks(const dl_canon_args* args);

/* ---- substructure search over a perceived batch: a SMARTS subset, structural alerts (substructure.hip) ----------------
 * For every molecule of a batch and every pattern of a compiled catalogue: is there an injective map of the pattern's atoms
 * to the molecule's kept atoms under which every atom predicate holds and every pattern bond falls on a kept bond whose
 * predicate holds (the match is not induced), and which original row roots the first one.  One 256-thread workgroup per
 * molecule, ONE launch per batch, the molecule in LDS, the compiled tables read-only in global memory, the stream as the last
 * field, as dl_canonical_ranks.  THE LANGUAGE AND THE RULE BELOW ARE THIS PROJECT'S OWN: NOT RDKit's SMARTS parser or matcher,
 * and these are NOT RDKit's numbers: no charges (every atom is neutral), no stereo, no isotopes, no explicit hydrogens in
 * molecules, no SSSR ring counts.  difflinker_amd/patterns.py compiles the tables; tests/substructure_ref.py restates the
 * search in plain Python and the kernel agrees with that in every output bit.
 *
 * THE GRAPH is the one dl_pharmacophore_features reads: atom k is the k-th row with node_mask != 0; `drop_mask` (may be NULL)
 * removes atoms AFTER that numbering together with every bond that touches them; the kept atoms are numbered among themselves
 * in row order (the KEPT INDEX).  `mark_mask` (may be NULL) marks atoms (the callers pass the linker).  The type of an atom is
 * the first largest entry of its one_hot row; Z = atomic_number[type] and dv = default_valence[type], both clamped to 0..255.
 * An entry (i, j, order) of the list is a bond when 0 <= i, j < atoms, i != j and 1 <= order <= 3, in either orientation; any
 * other entry is skipped and sets DL_SUB_BAD_BOND.  A pair listed more than once also sets DL_SUB_BAD_BOND, and its FIRST entry
 * gives the pair its order and its aromatic flag (bond_aromatic[entry] != 0; a NULL bond_aromatic flags nothing).  A bond is a
 * RING BOND when its ends are joined by another path; its ring size is the length of the shortest such path plus one.
 *
 * ATOM PROPERTIES, each saturating at 255:  D the kept neighbours;  S the sum of the orders of the kept bonds;
 * H = max(0, dv - S);  X = D + H;  V = S + H;  AROM: a kept bond of the atom is flagged aromatic;  XR the ring bonds of the
 * atom;  RS the smallest ring size over them (0 without one).
 *
 * THE TABLES (all int32, device): with Q = n_sub + n_top patterns, the n_sub sub-patterns (the bodies of $(...)) first,
 *   pat      [Q,8]   atom_off, n_atoms, level, screen[4], 0.  A pattern's atoms are rows atom_off .. atom_off + n_atoms - 1
 *                    of `atoms`; 1 <= n_atoms <= DL_SUB_MAX_PATTERN_ATOMS, any other pattern matches nothing.  A screen word
 *                    Z | count << 8 (0: unused) says the pattern needs `count` kept atoms of element Z; a pattern whose screen
 *                    fails, or with more atoms than the molecule has kept atoms, is not searched at all (no step is taken).
 *   atoms    [A,6]   parent (an earlier atom of the pattern; -1 for atom 0), the 12-bit mask of the bond to the parent,
 *                    pred_off, pred_len, closure_off, closure_len.
 *   closures [C,2]   an earlier atom of the pattern, the mask of the bond to it (the ring closures).
 *   preds    [T]     tokens op | arg << 8 | NEG << 24 | END_AND << 25 | END_OR << 26.  An atom's predicate is its pred_len
 *                    tokens: an AND of ORs of ANDs.  Each token's value (negated under NEG) is ANDed into the running
 *                    conjunction; END_AND ORs the conjunction into the running alternative and restarts it; END_OR ANDs the
 *                    alternative into the result and restarts it.  At most DL_SUB_MAX_PRED tokens.  ops: 0 TRUE, 1 Z == arg,
 *                    2 Z == arg and not AROM, 3 Z == arg and AROM, 4 AROM, 5 D == arg, 6 H == arg, 7 H >= arg, 8 X == arg,
 *                    9 V == arg, 10 XR > 0, 11 RS == arg, 12 XR == arg, 13 sub-pattern `arg` matches with its root here;
 *                    any other op is false.
 *   A bond's STATE is (order - 1) + 3 * aromatic + 6 * ring, and a bond predicate is the mask of the states it accepts.
 *   level_end[L] (in the struct, L < n_levels <= DL_SUB_MAX_LEVELS): sub-patterns [level_end[L-1], level_end[L]) have
 *   nesting level L and use sub-patterns of lower levels only; level_end[n_levels - 1] == n_sub <= DL_SUB_MAX_SUBPATTERNS.
 *
 * THE SEARCH of one pattern from one root (a kept atom), depth first, in the order the pattern's atoms are written: atom 0 is
 * tested on the root; the candidates for atom k > 0 are the kept neighbours of the image of its parent, in ascending kept
 * index; a candidate is taken when it is not yet an image, the bond from the parent's image is in the atom's mask, the atom's
 * predicate holds, and for every closure the candidate is bonded to the image of the closure's atom by a bond in the
 * closure's mask.  EVERY CANDIDATE TESTED IS ONE STEP, the root included.  A search that would take more than `max_steps`
 * steps stops: what it found stands, and DL_SUB_BUDGET is set.  Without mark_mask a search ends at its first complete map.
 * With mark_mask it goes on past complete maps that touch no marked atom (it backtracks as if the last candidate had failed)
 * until a complete map touches one or the search ends.  Every root is searched, independently of the others, so the result
 * and the status do not depend on how the work is spread over lanes.
 * Sub-patterns run first, level by level, from every root, without marks; op 13 reads their per-atom results.  A sub-pattern
 * root that runs out of budget counts as no match (and sets DL_SUB_BUDGET).
 *
 *   first_root         [B,n_top]: the lowest original ROW index (0 .. N-1) that roots a complete map of the pattern, -1: none
 *   first_root_marked  [B,n_top]: the same for complete maps that touch a marked atom; all -1 without mark_mask
 *   n_hits, n_hits_marked  [B]: the patterns with an entry >= 0
 *   status             [B]: the bits of `status_in`, plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a negative n_bonds_in
 *                      counts as 0), DL_SUB_BAD_BOND, DL_SUB_BUDGET, and DL_SUB_TOO_LARGE for more than DL_SUB_MAX_ATOMS kept
 *                      atoms or more than DL_SUB_MAX_BONDS kept list entries: every entry is then -1 and the counts are 0 (with
 *                      too many atoms the list is not looked at; with too many entries DL_SUB_BAD_BOND is added for an entry
 *                      that is no bond, and repeated pairs are not looked for).
 *
 * Integer work only; global memory is written with plain stores only, no atomics on global memory, every output element is
 * written, the callee allocates nothing and needs no workspace.  A null `args`, B < 0, N < 1, N > 1024, nf < 1, nf > 256,
 * capacity < 0, max_steps < 1, n_sub < 0, n_sub > DL_SUB_MAX_SUBPATTERNS, n_top < 0, n_levels < 0, n_levels >
 * DL_SUB_MAX_LEVELS, a level_end that decreases or does not end at n_sub, or a negative table length return DL_ERR_BAD_ARG;
 * then B == 0 or n_top == 0 returns DL_OK without a launch (nothing is written); then a null pointer (other than drop_mask,
 * mark_mask, bond_aromatic, stream, `bonds` when capacity is 0, and `closures` / `preds` of length 0) returns DL_ERR_BAD_ARG,
 * all before any device work. */
#define DL_SUB_MAX_ATOMS 256            /* kept atoms per molecule */
#define DL_SUB_MAX_BONDS 2048           /* kept list entries per molecule */
#define DL_SUB_MAX_PATTERN_ATOMS 48     /* atoms of a pattern, after the hydrogen merge */
#define DL_SUB_MAX_SUBPATTERNS 256      /* distinct $(...) bodies of a catalogue */
#define DL_SUB_MAX_LEVELS 4             /* nesting levels of $(...) */
#define DL_SUB_MAX_PRED 32              /* tokens of one atom's predicate */
#define DL_SUB_TOO_LARGE 4              /* status bit, same value as DL_CANON_TOO_LARGE */
#define DL_SUB_BAD_BOND 8               /* status bit, same value as DL_CANON_BAD_BOND */
#define DL_SUB_BUDGET 512               /* status bit: a root's search stopped at max_steps */
typedef struct dl_substructure_args {
    int32_t B, N, nf;
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* atomic_number;   /* device int32 [nf] */
    const int32_t* default_valence; /* device int32 [nf] */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* bond_aromatic;   /* device int32 [B,capacity] or NULL: dl_aromatic_args.bond_aromatic */
    const int32_t* status_in;       /* device int32 [B]: dl_bonds_args.status */
    int32_t n_sub, n_top, n_levels;
    int32_t level_end[DL_SUB_MAX_LEVELS];
    const int32_t* pat;             /* device int32 [n_sub + n_top, 8] */
    const int32_t* atoms;           /* device int32 [n_atoms_table, 6] */
    const int32_t* closures;        /* device int32 [n_closures, 2] */
    const int32_t* preds;           /* device int32 [n_preds] */
    int32_t n_atoms_table, n_closures, n_preds;
    int32_t max_steps;              /* >= 1; the Python layer's default is 4096 */
    int32_t* first_root;            /* device int32 [B,n_top] out */
    int32_t* first_root_marked;     /* device int32 [B,n_top] out */
    int32_t* n_hits;                /* device int32 [B] out */
    int32_t* n_hits_marked;         /* device int32 [B] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_substructure_args;
int32_t dl_substructure_match(const dl_substructure_args* args);

/* ---- stereo perception from 3D: tetrahedral centres and double bonds (stereo.hip) -----------------------------------
 * Which kept atoms are tetrahedral stereocentres and which double bonds are stereo double bonds, and which of their two
 * configurations the coordinates show: one 256-thread workgroup per molecule, ONE launch per batch, the molecule in LDS, the
 * stream as the last field, as dl_pose_checks and dl_canonical_ranks.  The reference removes stereo before it compares
 * strings (Chem.RemoveStereochemistry, src/metrics.py); this reads it off the sample.  THE RULE BELOW IS THIS PROJECT'S OWN:
 * NOT RDKit's stereo perception and NOT CIP.  The labels 1 and 2 are relative to this project's symmetry classes; they are
 * no R/S and no E/Z.  tests/stereo_ref.py restates the rule in plain Python and numpy and the kernel agrees with that in
 * every output bit.
 *
 * CONVENTIONS, those of dl_pose_checks.  Atom k is the k-th row with node_mask != 0; its type t is the FIRST largest entry
 * of its one_hot row.  `drop_mask` (may be NULL) removes atoms AFTER that numbering, together with their bonds; the kept atoms
 * are numbered among themselves in row order (the KEPT INDEX).  An entry (i, j, order) is a bond when 0 <= i, j < atoms,
 * i != j and 1 <= order <= 3, in either orientation; any other entry is skipped and sets DL_STEREO_BAD_BOND.  A repeated pair
 * sets DL_STEREO_BAD_BOND too and is ONE pair with its FIRST entry's order and bond_aromatic flag (in the classes below
 * every one of its entries counts, as in dl_canonical_ranks).  "Kept" means: not dropped, both ends for a bond; a
 * "neighbour" is the other end of a kept pair; d is the number of neighbours.  `mark_mask` (may be NULL) marks atoms by row.
 *
 * CLASSES.  The symmetry class of a kept atom is its tied rank after the ROOT refinement of dl_canonical_ranks:
 * c[i] = mix2(SEED_COLOUR, type_i + 1); n rounds of c'[i] = mix2(c[i], sum over the kept list entries (i, j, o) of
 * mix2(c[j], o)); class[i] = the number of kept atoms with a strictly smaller colour.  This is 1-WL: it does not see stereo,
 * and it can call two substituents equal that an orbit computation would separate (and the reverse never).  Centres and
 * double bonds whose substituents it ties are not perceived.  "The reverse never" is checked by the atlas sweep
 * (tests/test_atlas_host.py, tests/test_gpu_atlas.py): on every graph of up to 7 atoms and on vertex-transitive cage graphs,
 * two atoms that an automorphism found by networkx exchanges share their class.
 *
 * ARITHMETIC.  fp64 on (double) x, contraction off, every + - * / and sqrt rounded on its own in the order written;
 * v . w = (v_x*w_x + v_y*w_y) + v_z*w_z; v x w = (v_y*w_z - v_z*w_y, v_z*w_x - v_x*w_z, v_x*w_y - v_y*w_x);
 * det[a, b, c] = a . (b x c); unit(v) = (v_x/n, v_y/n, v_z/n) with n = sqrt(v . v).
 *
 * 1. TETRAHEDRAL CENTRES.  A kept atom a with atom_planar[a] == 0 (by atom number; NULL: none is planar) is a CENTRE when
 *    every one of its pairs has order 1, and, with vs the sum of its pairs' orders and h = max(0, default_valence[t] - vs),
 *    d == 4 and h == 0, or d == 3 and h == 1, and the classes of its neighbours are pairwise distinct (the implicit H is a
 *    class below all others).  So a trivalent N or P is no centre, a four-coordinate N is one.  Its neighbours sorted by
 *    ascending class are n0 < n1 < n2 < n3 (d == 3: n1 < n2 < n3, the H is n0).  u_k = unit(x_nk - x_a).
 *    d == 4: V = det[u1 - u0, u2 - u0, u3 - u0], T = flat * v_ideal4.  d == 3: V = det[u1, u2, u3], T = flat * v_ideal3.
 *    Label 1 when V > T, label 2 when V < -T, label 3 (UNDETERMINED) otherwise; a neighbour at zero distance gives label 3
 *    without the arithmetic.  The host passes v_ideal4 = 16/(3 sqrt 3) and v_ideal3 = 4/(3 sqrt 3), the values of V at
 *    the ideal tetrahedron.  A mirror image exchanges labels 1 and 2 exactly: negating one coordinate negates V bit for bit.
 * 2. STEREO DOUBLE BONDS.  A kept pair (a, b) of order 2, a < b by kept index, is a STEREO DOUBLE BOND when its first entry
 *    is not flagged in bond_aromatic (NULL: none is), it is in no ring of fewer than 8 atoms (the shortest path from a to b
 *    that does not use the pair has 7 or more bonds, or there is none), and each end has one or two OTHER neighbours, all
 *    through pairs of order 1, whose classes differ when there are two.  The REFERENCE neighbour of an end is the other
 *    neighbour with the highest class.  e = unit(x_b - x_a); w = x_ra - x_a for the reference ra of a, s = w . e,
 *    p = w - s * e by component; likewise q from x_rb - x_b.  lp = sqrt(p . p), lq = sqrt(q . q).  Label 3 when
 *    x_b - x_a has zero length, or lp < 0.1 or lq < 0.1 (A).  Otherwise c = (p . q) / (lp * lq): label 1 (cis: the two
 *    reference neighbours on one side) when c > twist, label 2 (trans) when c < -twist, label 3 otherwise.
 *
 *   atom_class   [B,N] by atom number, written in full: the class; -1 for a dropped atom and from the atom count on
 *   atom_stereo  [B,N] by atom number, written in full: 0 no centre, 1, 2 or 3; -1 where atom_class is -1
 *   bond_stereo  [B,capacity] by list entry, written in full: 0, 1, 2 or 3 on the first entry of a stereo double bond's pair,
 *                0 on every other entry
 *   counts       [B][2][4], written in full: centres with label 1 or 2, centres with label 3, double bonds with label 1 or 2,
 *                double bonds with label 3.  Row 0: all; row 1: the items with a marked atom among the centre and its
 *                neighbours, or among the bond's two ends and two reference neighbours.
 *   status       [B]: the bits of `status_in` (may be NULL: none), plus DL_BONDS_OVERFLOW when n_bonds_in > capacity (a
 *                negative n_bonds_in counts as 0), DL_STEREO_BAD_BOND, and the limits.  None disturbs the other molecules.
 *                DL_STEREO_TOO_LARGE: more than DL_STEREO_MAX_ATOMS KEPT atoms (N itself may be 1024; neither the list nor
 *                  the coordinates are looked at) or more than DL_STEREO_MAX_BONDS kept list entries (DL_STEREO_BAD_BOND is
 *                  then added for an entry that is no bond only): atom_class and atom_stereo are -1 everywhere, bond_stereo
 *                  and counts 0.
 *                DL_STEREO_NONFINITE: a kept atom has a NaN or inf coordinate: atom_class stands, every label and count is 0.
 *
 * Integer sums only, and every fp64 decision is made by one thread from LDS-resident data in the order written above (ends
 * ordered by kept index, neighbours by class): the same bits on every run and under every order and orientation of the list.
 * Global memory is written with plain stores only; the callee allocates nothing and needs no workspace.  A null `args`, B < 0,
 * N < 1, N > 1024, nf < 1, nf > 256, capacity < 0, a flat or twist that is negative or NaN, or a v_ideal4 or v_ideal3 that is
 * not positive (NaN included) return DL_ERR_BAD_ARG; then
 * B == 0 returns DL_OK without a launch; then a null pointer (other than drop_mask, mark_mask, atom_planar, bond_aromatic,
 * status_in, stream, and `bonds` / `bond_stereo` when capacity is 0) returns DL_ERR_BAD_ARG, all before any device work.
 * Not here: R/S and E/Z names; pseudo-asymmetric and stereo-dependent centres (the classes do not see stereo); trivalent N, P
 * and sulfoxide centres; allenes, cumulenes and atropisomers; amide bonds (order 1). */
#define DL_STEREO_MAX_ATOMS 256     /* kept atoms per molecule */
#define DL_STEREO_MAX_BONDS 2048    /* kept list entries per molecule */
#define DL_STEREO_TOO_LARGE 4       /* status bit, same value as DL_POSE_TOO_LARGE and DL_CANON_TOO_LARGE */
#define DL_STEREO_BAD_BOND 8        /* status bit, same value as DL_POSE_BAD_BOND and DL_CANON_BAD_BOND */
#define DL_STEREO_NONFINITE 64      /* status bit, same value as DL_POSE_NONFINITE */
#define DL_STEREO_COUNTS 4          /* values per row of `counts` */
typedef struct dl_stereo_args {
    int32_t B, N, nf;
    const float* x;                 /* device f32 [B,N,3], Angstrom */
    const float* one_hot;           /* device f32 [B,N,nf] */
    const float* node_mask;         /* device f32 [B,N] */
    const float* drop_mask;         /* device f32 [B,N] or NULL */
    const float* mark_mask;         /* device f32 [B,N] or NULL */
    const int32_t* atom_planar;     /* device int32 [B,N] by atom number, or NULL: dl_aromatic_args.atom_aromatic */
    const int32_t* default_valence; /* device int32 [nf]: the table of dl_add_hydrogens */
    int32_t capacity;               /* bonds the list holds per molecule */
    const int32_t* n_bonds_in;      /* device int32 [B]: dl_bonds_args.n_bonds */
    const int32_t* bonds;           /* device int32 [B,capacity,3] (may be NULL when capacity is 0) */
    const int32_t* bond_aromatic;   /* device int32 [B,capacity] or NULL: dl_aromatic_args.bond_aromatic */
    const int32_t* status_in;       /* device int32 [B] or NULL: dl_bonds_args.status or dl_aromatic_args.status */
    double flat, twist;             /* the rule's two parameters; the Python layer's defaults are 0.25 and 0.5 */
    double v_ideal4, v_ideal3;      /* 16/(3 sqrt 3) and 4/(3 sqrt 3), formed by the host */
    int32_t* atom_class;            /* device int32 [B,N] out */
    int32_t* atom_stereo;           /* device int32 [B,N] out */
    int32_t* bond_stereo;           /* device int32 [B,capacity] out (may be NULL when capacity is 0) */
    int32_t* counts;                /* device int32 [B,2,4] out */
    int32_t* status;                /* device int32 [B] out */
    void* stream;                   /* hipStream_t; NULL: the default stream */
} dl_stereo_args;
int32_t dl_stereo_perceive(const dl_stereo_args* args);

const char* dl_error_string(int32_t status);
int32_t dl_last_hip_error(void);
int32_t dl_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DIFFLINKER_HIP_H */
