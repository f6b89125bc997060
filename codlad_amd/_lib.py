"""ctypes binding of libcodlad_hip.so (include/codlad_hip.h).

There is no CPU fallback: if the library is missing or a call fails, this raises.
`import torch` happens first so that the library's libamdhip64.so.7 dependency resolves to the
HIP runtime PyTorch already loaded (same SONAME) - streams and device pointers are then shared.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 19   # CODLAD_ABI_VERSION of include/codlad_hip.h this binding was written against
# CODLAD_HIP_LIB: an alternative build of the same ABI (A/B measurements, tools/ablate_edge.py)
LIB_PATH = os.environ.get("CODLAD_HIP_LIB") or os.path.join(_HERE, "libcodlad_hip.so")

P = C.c_void_p


class EncLayer(C.Structure):
    _fields_ = [(n, P) for n in ("W1e", "W2", "W3", "W11e", "W12", "W13", "W1a", "W1c", "W11a", "W11c")] + \
               [("Win", P * 4), ("Wout", P * 4)] + \
               [(n, P) for n in ("b1", "b2", "b3", "b11", "b12", "b13", "b_in", "b_out")]


class DecLayer(C.Structure):
    _fields_ = [(n, P) for n in ("W1e", "W2", "W3", "W1a", "W1v", "TS")] + \
               [("Win", P * 4), ("Wout", P * 4)] + \
               [(n, P) for n in ("b1", "b2", "b3", "b_in", "b_out")]


class EncLayerH(C.Structure):
    _fields_ = [(n, P) for n in ("W1e", "W2", "W3", "W11e", "W12", "W13", "W1a", "W1c", "W11a", "W11c")] + \
               [("Win", P * 4), ("Wout", P * 4)] + \
               [(n, P) for n in ("b1", "b2", "b3", "b11", "b12", "b13", "b_in", "b_out")] + \
               [(n, C.c_int) for n in ("e1", "e2", "e3", "e11", "e12", "e13", "e_in", "e_out")]


class DecLayerH(C.Structure):
    _fields_ = [(n, P) for n in ("W1e", "W2", "W3", "W1a", "W1v")] + [("Win", P * 4), ("Wout", P * 4)] + \
               [(n, P) for n in ("TS", "b1", "b2", "b3", "b_in", "b_out")] + \
               [(n, C.c_int) for n in ("e1", "e2", "e3", "e_in", "e_out")]


class DenoiserWeights(C.Structure):
    _fields_ = [(n, P) for n in ("freqs", "rbf_mu", "t_w0", "t_b0", "t_w2", "t_b2")] + \
               [("ada_w", P * 7), ("ada_b", P * 7)] + \
               [(n, P) for n in ("x_in_w", "x_in_b", "pos_w", "pos_b", "edge_wT", "norm_w", "norm_b",
                                 "We_wT", "We_b", "out_w", "out_b")] + \
               [("enc", EncLayer * 3), ("dec", DecLayer * 3), ("precision", C.c_int),
                ("enc_h", EncLayerH * 3), ("dec_h", DecLayerH * 3), ("self_condition", C.c_int), ("out_dim", C.c_int)]


class Workspace(C.Structure):
    _fields_ = [(n, P) for n in ("hV", "hVenc", "S", "PQ", "hE", "status", "tile_list")] + [("n_tiles", C.c_int32), ("xcd_bounds", P)]


class JobDesc(C.Structure):
    """codlad_job: a job's node table, its structures' graph and edge terms, its workspace."""
    _fields_ = [("node_info", P), ("n_nodes", C.c_int), ("E_idx", P), ("h_E0", P), ("E1", P), ("n_snodes", C.c_int),
                ("ws", C.POINTER(Workspace))]


class DecoderWeights(C.Structure):
    _fields_ = [("angle", C.c_int), ("map_out_w", P), ("map_out_b", P), ("res_embed", P)] + \
               [(n, P * 4) for n in ("inv0_w", "inv0_b", "inv1_w", "inv1_b", "dist_w", "dist_b",
                                     "dense1_w", "dense1_b", "dense3_w", "dense3_b")] + \
               [(n, P) for n in ("bb_dist", "sc_dist", "bb_ang1_w", "bb_ang1_b", "bb_ang3_w", "bb_ang3_b",
                                 "sc_angle_emb", "sc_ang1_w", "sc_ang1_b", "sc_ang3_w", "sc_ang3_b",
                                 "bb_tor1_w", "bb_tor1_b", "bb_tor3_w", "bb_tor3_b")] + \
               [(n, P * 4) for n in ("tor1_w", "tor1_b", "tor3_w", "tor3_b")] + \
               [(n, P) for n in ("fin1_w", "fin1_b", "fin3_w", "fin3_b")]


class TpConvArgs(C.Structure):
    _fields_ = [("ptr", P), ("snd", P), ("n_recv", C.c_int32), ("xyz_recv", P), ("xyz_snd", P), ("typ_recv", P),
                ("typ_snd", P), ("r_sign", C.c_float), ("smear_stop", C.c_float), ("emb0_w", P), ("emb0_b", P),
                ("emb3_w", P), ("emb3_b", P), ("emb_in", C.c_int32), ("h_recv", P), ("d_recv", C.c_int32), ("h_snd", P),
                ("d_snd", C.c_int32), ("attr_recv_first", C.c_int32), ("fc0_w", P), ("fc0_b", P), ("fc3_w", P),
                ("fc3_b", P), ("depth", C.c_int32), ("out", P), ("accumulate", C.c_int32), ("group", C.c_int32),
                ("packed", P)]


class XyzGroup(C.Structure):
    _fields_ = [("ca_full", P), ("ic", P), ("orders", P), ("slot_to_out", P), ("xyz_out", P),
                ("B", C.c_int32), ("L", C.c_int32), ("n_atoms", C.c_int32), ("first_row", C.c_int32)]


class MetricInputs(C.Structure):
    _fields_ = [("xyz_recon", P), ("xyz", P), ("n_atoms", C.c_int64),
                ("edge_list", P), ("n_edges", C.c_int64), ("clash_list", P), ("n_clash", C.c_int64),
                ("bb_NO_list", P), ("n_bb", C.c_int64), ("interaction_list", P), ("n_inter", C.c_int64),
                ("pi_pi_list", P), ("n_pipi", C.c_int64),
                ("ic", P), ("ic_recon", P), ("ic_mask", P), ("n_ic", C.c_int64)]


class LossTerms(C.Structure):
    """codlad_loss_terms: the per-sample results of the loss kernels, each may be NULL."""
    _fields_ = [(n, P) for n in ("kl", "nll", "vb", "mse", "xstart_mse", "eps_mse", "pred_xstart")]


class FmLossOut(C.Structure):
    """codlad_fm_loss_out: the per-sample means of the flow-matching loss kernel, each may be NULL."""
    _fields_ = [(n, P) for n in ("l2", "l1", "huber", "smooth_l1", "log_cosh")]


class OdeState(C.Structure):
    """codlad_ode_state: the adaptive ODE method's device state block (read back after every attempt)."""
    _fields_ = [(n, C.c_double) for n in ("t", "h", "t_end", "ratio", "hh")] + \
               [(n, C.c_int32) for n in ("accepted", "n_accept", "n_reject", "clipped", "nonfinite", "status")] + \
               [("hh_f", C.c_float), ("tf", C.c_float * 6), ("pad_", C.c_float)]


class OdeDopri5Bufs(C.Structure):
    """codlad_ode_dopri5_bufs"""
    _fields_ = [("y", P), ("y1", P), ("xin", P), ("k", P * 7), ("mods", P), ("state", P), ("norm", P)]


FM_KINDS = {"icfm": 0, "target": 1, "vp": 2}           # CODLAD_FM_* of include/codlad_hip.h
FM_TARGET_FLOW = 3                                     # CODLAD_FM_TARGET_FLOW: the target matcher's flow of a given xt
ODE_METHODS = {"euler": 0, "midpoint": 1, "rk4": 2}    # CODLAD_ODE_* of include/codlad_hip.h
GEOM_BOND_FLAG = 1 << 30                               # CODLAD_GEOM_BOND_FLAG: an order-1 partner in the exclusion CSR
STEREO_COLUMNS, STEREO_N_COUNTS, STEREO_KIND_PRO = 9, 6, 1   # CODLAD_STEREO_COLUMNS, _COUNTS, _KIND_PRO
STEREO_FLAGS = {"inverted_ca": 1, "inverted_side": 2, "cis": 4, "twisted": 8, "undefined": 16}   # CODLAD_STEREO_* flag bits
SASA_MAX_POINTS = 1024                                 # CODLAD_SASA_MAX_POINTS
DSSP_MAX_RES = 4096                                    # CODLAD_DSSP_MAX_RES
DSSP_CODES = " HBEGITS"                                # CODLAD_DSSP_LOOP, _H, _B, _E, _G, _I, _T, _S = 0 .. 7; 255 = undefined
DSSP_KIND_PRO, DSSP_KIND_CHAIN_START, DSSP_GEOM_LINK, DSSP_GEOM_BEND, DSSP_UNDEFINED = 1, 2, 1, 2, 255   # CODLAD_DSSP_*
SAXS_MAX_Q, SAXS_MAX_TYPES, SAXS_Q_CHUNK = 512, 32, 16    # CODLAD_SAXS_MAX_Q, _MAX_TYPES, _Q_CHUNK
SAXS_X_MAX, SAXS_X_SMALL, SAXS_SIN_ULPS = 25600.0, 0.125, 5   # CODLAD_SAXS_X_MAX, _X_SMALL, _SIN_ULPS
SAXS_HYD_PARTIALS, SAXS_HYD_Q_CHUNK, SAXS_HYD_MAX_GRID = 6, 8, 4096   # CODLAD_SAXS_HYD_PARTIALS, _Q_CHUNK, _MAX_GRID
PAIR_HIST_MAX_BINS, PAIR_HIST_MAX_ATOMS, PAIR_HIST_ITEM_WORDS, PAIR_HIST_ROWS = 4096, 65535, 5, 64   # CODLAD_PAIR_HIST_*
REWEIGHT_LADDER, REWEIGHT_SCALARS, REWEIGHT_MAX_PROBLEMS, REWEIGHT_MAX_ITER = 16, 4, 4096, 1000   # CODLAD_REWEIGHT_*
CLUSTER_MAX_N, CLUSTER_MAX_ROUNDS, CLUSTER_STATE_WORDS = 65536, 4096, 8   # CODLAD_CLUSTER_MAX_N, _MAX_ROUNDS, _STATE_WORDS
CLUSTER_ST_PHASE, CLUSTER_ST_ACTIVE, CLUSTER_ST_CLUSTERS, CLUSTER_ST_ROUNDS = 0, 1, 2, 3   # CODLAD_CLUSTER_ST_*
PCA_MAX_N, PCA_MAX_DIM, PCA_MAX_COMPONENTS, PCA_MAX_ITER = 65536, 4096, 64, 4096   # CODLAD_PCA_MAX_*
PCA_STATE_WORDS, PCA_ST_PHASE, PCA_ST_ITER, PCA_ST_STATUS, PCA_ST_START = 8, 0, 1, 2, 3   # CODLAD_PCA_STATE_WORDS, _ST_*
PCA_SCALARS, PCA_SC_W, PCA_SC_STEP = 4, 0, 1           # CODLAD_PCA_SCALARS, _SC_*
PCA_STATUS = ("converged", "limit", "no_weight")       # CODLAD_PCA_CONVERGED, _LIMIT, _NO_WEIGHT = 0 .. 2
COMPARE_MAX_ROWS, COMPARE_MAX_BINS, DIST_HIST_MAX_SEL, DIVERGENCE_MAX_COLS = 1048576, 256, 2048, 4098   # CODLAD_COMPARE_MAX_*, ..
LDDT_MAX_THRESHOLDS, LDDT_MAX_ATOMS = 8, 46340         # CODLAD_LDDT_MAX_THRESHOLDS, _MAX_ATOMS
POLYMER_MAX_SEL, POLYMER_SPLIT_MAX_N, POLYMER_SPLIT_MIN_SEL = 8192, 256, 512   # CODLAD_POLYMER_MAX_SEL, _SPLIT_MAX_N, _SPLIT_MIN_SEL
DRMSD_MAX_SEL, DRMSD_WINDOW, DRMSD_SLAB_TILES, DRMSD_SPLIT_MAX_BLOCKS = 8192, 16, 64, 256   # CODLAD_DRMSD_MAX_SEL, _WINDOW, _SLAB_TILES, ..
TORSION_MAX_T, TORSION_X_OPS, TORSION_Y_OPS = 2048, 11, 13   # CODLAD_TORSION_MAX_T, _X_OPS, _Y_OPS
REWEIGHT_STATUS = ("converged", "cap", "stalled", "failed", "none")   # CODLAD_REWEIGHT_CONVERGED .. _NONE = 0 .. 4
ODE_NORM_WORDS = 257                                   # CODLAD_ODE_NORM_WORDS

_JOB = [C.POINTER(DenoiserWeights), C.POINTER(JobDesc)]    # what every entry point that runs the denoiser starts with

_SIGS = {
    "codlad_abi_version": (C.c_int, []),
    "codlad_probe_edge_launches": (C.c_int, [C.c_int]),
    "codlad_probe_read": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "codlad_dispatch_read": (C.c_int, [P, C.c_int]),
    "codlad_metrics_scratch_bytes": (C.c_int, []),
    "codlad_eval_metrics": (C.c_int, [C.POINTER(MetricInputs), P, P, P]),
    "codlad_bond_graph_counts": (C.c_int, [P, P, P, P, P, C.c_int, C.c_int, C.c_float, P, P]),
    "codlad_ens_moments": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P]),
    "codlad_ens_pair_msd": (C.c_int, [P, P, C.c_int, P, P, C.c_int, C.c_int, P, C.c_int, P, C.c_int, C.c_int, P, P, P]),
    "codlad_ens_apply": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "codlad_ens_pairwise": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, P, P]),
    "codlad_geometry_check": (C.c_int, [P, C.c_int, C.c_int, P, P, P, P, C.c_int, C.c_float, C.c_float, C.c_float, P, P, P]),
    "codlad_stereo_check": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int, P, P, P, P]),
    "codlad_relax_scratch_bytes": (C.c_longlong, [C.c_int] * 5),
    "codlad_relax_energy": (C.c_int, [P, P, C.c_int, C.c_int, P, P, P, P, P, P, C.c_int, P, C.c_int, P, P, C.c_int] +
                            [C.c_float] * 4 + [P] * 5),
    "codlad_relax": (C.c_int, [P, C.c_int, C.c_int, P, P, P, P, P, P, C.c_int, P, C.c_int, P, P, C.c_int] +
                     [C.c_float] * 6 + [C.c_int] + [P] * 9),
    "codlad_sasa": (C.c_int, [P, C.c_int, C.c_int, P, P, P, C.c_int, P, C.c_int, P, P, P, P, P, P]),
    "codlad_contact_counts": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, C.c_float, P, P]),
    "codlad_dssp_hbonds": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int, P, P, P, P, P, P, P, P]),
    "codlad_dssp_assign": (C.c_int, [P, P, P, P, C.c_int, C.c_int, P, P, P, P]),
    "codlad_saxs_debye": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P, C.c_int, P, P, P, P, P]),
    "codlad_saxs_partials": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, C.c_int, P, P, P, P, P]),
    "codlad_saxs_hydration_fit": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int, P, C.c_int, P, P, P, P, P, P, P, P]),
    "codlad_pair_hist": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int, C.c_float, C.c_int, P, C.c_int, P, P, P, P, P]),
    "codlad_pair_hist_profile": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, C.c_int] + [P] * 11),
    "codlad_reweight_scratch_bytes": (C.c_longlong, [C.c_int] * 3),
    "codlad_reweight_solve": (C.c_int, [P, P, P, P, C.c_int, C.c_int, P, P, C.c_int, P, C.c_double, C.c_int, P, C.c_longlong] +
                              [P] * 8),
    "codlad_weighted_mean": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "codlad_rmsd_matrix_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_rmsd_matrix": (C.c_int, [P, P, C.c_int, C.c_int, P, C.c_int, C.c_double, C.c_int, P, P, P, P, P]),
    "codlad_cluster_scratch_bytes": (C.c_longlong, [C.c_int]),
    "codlad_cluster_daura": (C.c_int, [P, P, C.c_int, C.c_int, P, P, P, P, P, P]),
    "codlad_cluster_populations": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "codlad_pca_fit_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_pca_fit": (C.c_int, [P, P, C.c_int, C.c_int, P, C.c_int, P, C.c_int, C.c_double, C.c_int, C.c_int] + [P] * 8),
    "codlad_pca_align": (C.c_int, [P, P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, P]),
    "codlad_pca_deviations": (C.c_int, [P, P, P, P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, P]),
    "codlad_pca_covariance_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_pca_covariance": (C.c_int, [P, P, P, C.c_int, C.c_int, P, P, P, P, P, P]),
    "codlad_pca_eigen_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_pca_eigen": (C.c_int, [P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, P, P, P, P, P, P]),
    "codlad_pca_project": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "codlad_dist_hist_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_column_hist_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_dist_hist": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, C.c_float, C.c_int, P, P, P, P]),
    "codlad_column_hist": (C.c_int, [P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, P, P, P]),
    "codlad_hist_divergence": (C.c_int, [P, P, C.c_int, C.c_int, P, P, P, P]),
    "codlad_lddt": (C.c_int, [P, C.c_int, P, C.c_int, P, C.c_int, P, C.c_int, P, C.c_int, P, P, P, P, C.c_int, C.c_float, P, C.c_int,
                              C.c_int] + [P] * 11),
    "codlad_chain_sums_groups": (C.c_int, [C.c_int] * 2),
    "codlad_chain_sums": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, P]),
    "codlad_gyration": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P, P, P, P, P]),
    "codlad_drmsd_groups": (C.c_int, [C.c_int] * 4),
    "codlad_drmsd_matrix_scratch_bytes": (C.c_longlong, [C.c_int] * 4),
    "codlad_drmsd_matrix": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, C.c_int, C.c_double, C.c_int, P, P, P, P, P, P]),
    "codlad_drmsd_pairs": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, C.c_int, P, C.c_int, P, P, P]),
    "codlad_torsion_features": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P, P]),
    "codlad_torsion_mean_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_torsion_mean": (C.c_int, [P, P, P, C.c_int, C.c_int, P, P, P, P, P]),
    "codlad_torsion_matrix_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_torsion_matrix": (C.c_int, [P, P, C.c_int, P, P, C.c_int, C.c_int, C.c_double, C.c_int, P, P, P, P]),
    "codlad_torsion_pairs": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, P, P, P]),
    "codlad_feature_covariance_scratch_bytes": (C.c_longlong, [C.c_int] * 2),
    "codlad_feature_covariance": (C.c_int, [P, P, P, C.c_int, C.c_int, P, P, P, P, P]),
    "codlad_last_error": (C.c_char_p, []),
    "codlad_struct_sizes": (None, [C.POINTER(C.c_int)]),
    "codlad_pack_block_host": (None, [P, C.c_int, C.c_float, P]),
    "codlad_features_prepass": (C.c_int, [C.POINTER(DenoiserWeights), P, P, C.c_int, C.c_int, P, P, P]),
    "codlad_step_mods": (C.c_int, [C.POINTER(DenoiserWeights), P, C.c_int, P, P]),
    "codlad_step_mods_f": (C.c_int, [C.POINTER(DenoiserWeights), P, C.c_int, P, P]),
    "codlad_ode_combine": (C.c_int, [P, P, P, C.c_int, C.c_float, C.c_size_t, P, P]),
    "codlad_ode_error_norm": (C.c_int, [P, P, P, C.c_size_t, C.c_float, C.c_float, P, P]),
    "codlad_ode_loop": (C.c_int, _JOB + [P, P, P, C.c_int, P, C.c_int, P, P]),
    "codlad_ode_dopri5_attempt": (C.c_int, _JOB + [C.POINTER(OdeDopri5Bufs), C.c_double, C.c_float, C.c_float, P]),
    "codlad_layer0_edge_terms": (C.c_int, [C.POINTER(DenoiserWeights), P, C.c_int, P, P, P]),
    "codlad_denoiser_forward": (C.c_int, _JOB + [P, P, P, P, P]),
    "codlad_status_check": (C.c_int, [P, P]),
    "codlad_set_option": (C.c_int, [C.c_int, C.c_int]),
    "codlad_edge_plan_host": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "codlad_ddpm_update": (C.c_int, [P, P, P, P, C.c_int, P, P, P]),
    "codlad_ddpm_pred_xstart": (C.c_int, [P, P, P, C.c_int, P, P]),
    "codlad_ddpm_posterior_step": (C.c_int, [P, P, P, P, P, P, C.c_float, C.c_int, P, P, P]),
    "codlad_sample_loop": (C.c_int, _JOB + [P, P, P, P, P, C.c_int, P]),
    "codlad_sample_loop_pinned": (C.c_int, _JOB + [P, P, P, P, P, C.c_int, P, P, P]),
    "codlad_ddim_loop": (C.c_int, _JOB + [P, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "codlad_ddim_step": (C.c_int, [P, P, P, P, P, C.c_int, C.c_int, P, P, P]),
    "codlad_dpm_loop": (C.c_int, _JOB + [P, P, P, P, C.c_int, C.c_int, P, P, P]),
    "codlad_dpm_step": (C.c_int, [P, P, P, P, P, C.c_int, P, P, P]),
    "codlad_q_sample": (C.c_int, [P, P, P, C.c_int, P, C.c_int, P, C.c_int, P, P, P, P]),
    "codlad_q_posterior": (C.c_int, [P, P, P, C.c_int, P, C.c_int, P, C.c_int, P, P, P, P]),
    "codlad_vb_terms": (C.c_int, [P, P, P, P, P, C.c_int, P, C.c_int, P, C.c_int, C.POINTER(LossTerms), P]),
    "codlad_prior_bpd": (C.c_int, [P, P, C.c_int, P, C.c_int, P, P]),
    "codlad_loss_forward": (C.c_int, _JOB + [P, P, P, P, P, P, C.c_int, C.c_int, P, C.c_int, P, C.POINTER(LossTerms), P]),
    "codlad_bpd_loop": (C.c_int, _JOB + [P, P, P, P, P, C.c_int, P, C.c_int, P, P, P, P, P, P]),
    "codlad_fm_path": (C.c_int, [P, P, P, P, C.c_int, P, C.c_float, C.c_int, C.c_double, P, P, P]),
    "codlad_fm_terms": (C.c_int, [P, P, P, C.c_int, C.POINTER(FmLossOut), P]),
    "codlad_fm_loss_forward": (C.c_int, _JOB + [P, P, P, P, C.c_int, P, C.POINTER(FmLossOut), P]),
    "codlad_fm_loss_loop": (C.c_int, _JOB + [P, P, P, C.c_int, C.c_double, P, C.c_int, P, P, C.c_int, P, P,
                                             C.POINTER(FmLossOut), P]),
    "codlad_vq_lookup": (C.c_int, [P, C.c_int, P, P, P, C.c_int, P, P, P, P]),
    "codlad_ic_decode": (C.c_int, [C.POINTER(DecoderWeights), P, P, P, P, P, C.c_int, P, P, P]),
    "codlad_cg_graph": (C.c_int, [P, P, C.c_int, C.c_float, P, P, P, P]),
    "codlad_ic_to_xyz": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "codlad_ic_to_xyz_groups": (C.c_int, [P, C.c_int, C.c_int, P]),
    "codlad_xyz_to_ic": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P]),
    "codlad_tp_conv_image_bytes": (C.c_int, [C.c_int]),
    "codlad_tp_conv_pack": (C.c_int, [P, P, P]),
    "codlad_receiver_csr": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P]),
    "codlad_bench_edge_launch": (C.c_int, [C.POINTER(DenoiserWeights), P, C.c_int, P, P, P,
                                           C.POINTER(Workspace), C.c_int, C.c_int, P]),
    "codlad_tp_conv": (C.c_int, [C.POINTER(TpConvArgs), P]),
    "codlad_tp_conv_args_size": (C.c_int, []),
    "codlad_mlp_rows": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "codlad_bead_mean": (C.c_int, [P, P, P, P, C.c_int, P, P]),
    "codlad_embed_rows": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "codlad_selftest_gemm128": (C.c_int, [P, P, P, C.c_int, C.c_int, P, P]),
    "codlad_selftest_gemm128_h": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, P, P]),
}

_lib = None


def lib():
    """The loaded library; raises if it has not been built (python -m codlad_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is the only implementation of this path "
                "(build it with `python -m codlad_amd.build`)")
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:      # e.g. a build from before an entry point was added under the same ABI version
                raise RuntimeError(f"{LIB_PATH} does not export {name}: it was built from an older include/codlad_hip.h "
                                   f"(ABI version {ABI_VERSION} covers additions); rebuild it") from None
            fn.restype = res
            fn.argtypes = args
        if handle.codlad_abi_version() != ABI_VERSION:
            raise RuntimeError("libcodlad_hip.so ABI version mismatch")
        _lib = handle
    return _lib


OPT_NODEQ_MAX_TILES, OPT_EDGE_TILE_MAX_NODES, OPT_DEC_EDGE_VARIANT, OPT_TP_CONV_VARIANT, OPT_EDGE_UPD_VARIANT, OPT_EDGE_CUS, OPT_EDGE_WIDE_MAX_TILES, OPT_NODE_QUAD_MAX_TILES = 0, 1, 3, 4, 5, 6, 7, 2   # CODLAD_OPT_* of include/codlad_hip.h
OPT_EDGE_PAIR = 8
EDGE_GRID = (256, 8)    # persistent grid of the per-node edge kernels on MI355X: one 8-wave workgroup per CU


def edge_plan(K, pair=True, grid=EDGE_GRID):
    """codlad_edge_plan_host: K = the nodes' neighbour counts (node_info[:, 2], host) -> (bounds int32 [9], stats int64 [20]):
    the XCD chunk bounds of the per-node edge kernels and the tile accounting of their walk (include/codlad_hip.h)."""
    import numpy as np
    K = np.ascontiguousarray(K, dtype=np.int32)
    bounds, stats = np.zeros(9, dtype=np.int32), np.zeros(20, dtype=np.int64)
    check(lib().codlad_edge_plan_host(K.ctypes.data_as(P), K.shape[0], grid[0], grid[1], int(bool(pair)),
                                      bounds.ctypes.data_as(P), stats.ctypes.data_as(P)), "codlad_edge_plan_host")
    return bounds, stats


DISPATCH_WORDS = ("edge", "node_in", "node_upd", "chunked_in", "chunked_upd", "grid_edge_msg", "grid_edge_upd", "grid_node_in",
                  "grid_node_upd")                                   # CODLAD_DISPATCH_* of include/codlad_hip.h
EDGE_KINDS = ("f32", "wide", "tile", "node", "node_upd1")           # CODLAD_EDGE_KIND_*
NODE_KINDS = ("f32", "w", "q", "h4", "h8")                          # CODLAD_NODE_KIND_*


def dispatch_read():
    """codlad_dispatch_read: what the last forward of this process dispatched -> dict of DISPATCH_WORDS; the three kinds by
    name (EDGE_KINDS / NODE_KINDS), the placement flags as bool, the grids as int."""
    out = (C.c_int32 * len(DISPATCH_WORDS))()
    n = lib().codlad_dispatch_read(out, len(DISPATCH_WORDS))
    if n != len(DISPATCH_WORDS):
        raise RuntimeError(f"codlad_dispatch_read: the library keeps {n} words, this binding knows {len(DISPATCH_WORDS)}")
    rec = dict(zip(DISPATCH_WORDS, (int(v) for v in out)))
    rec["edge"] = EDGE_KINDS[rec["edge"]]
    rec["node_in"], rec["node_upd"] = NODE_KINDS[rec["node_in"]], NODE_KINDS[rec["node_upd"]]
    rec["chunked_in"], rec["chunked_upd"] = bool(rec["chunked_in"]), bool(rec["chunked_upd"])
    return rec


def set_option(option, value):
    """Tuning switch of the library (speed only; include/codlad_hip.h codlad_set_option)."""
    check(lib().codlad_set_option(option, value), "codlad_set_option")


def exported_symbols():
    return list(_SIGS)


def check(rc, what):
    if rc != 0:
        msg = lib().codlad_last_error().decode() or "unknown error"
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


class _TensorPtr(C.c_void_p):
    """c_void_p that keeps its tensor alive for as long as the argument object lives, i.e. until
    the foreign call has been enqueued.  (A bare integer would let a temporary such as
    `x.contiguous()` be freed - and its block reused by the next temporary - before the launch.)"""


def ptr(t):
    """Device (or host) pointer of a contiguous tensor, None -> NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), "non-contiguous tensor handed to the C ABI"
    p = _TensorPtr(t.data_ptr())
    p._keepalive = t
    return p


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
