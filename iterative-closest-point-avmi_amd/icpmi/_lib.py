"""ctypes binding of libicpmi.so (include/icpmi.h).

There is no CPU fallback: if the shared library is missing or a call fails the
caller gets an exception, never a silently different code path.
"""
import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_PKG, "csrc")
LIB_PATH = os.path.join(_PKG, "lib", "libicpmi.so")

OK = 0
ST_CONVERGED, ST_MAXITER, ST_FEW_INLIERS, ST_EMPTY, ST_SKIPPED = 1, 2, 3, 4, 5
RES_DOUBLES, RES_R, RES_T, RES_ERR, RES_DELTA, RES_ITERS, RES_STATUS = 16, 0, 9, 12, 13, 14, 15
POINT_TO_POINT, POINT_TO_LINE = 0, 1
# the record of icpmi_rotation_search (RSREC_*; the workspace offsets its callers read the filtered clouds at), what
# icpmi_rotation_search_batch adds to it (RSBREC_*, RSB_*), icpmi_rotation_refine's capacity, and the record, statuses and
# capacities of the feature alignment (FTREC_*, FT_*): include/icpmi.h's ICPMI_* names (tests/test_host_cpu.py compares)
RSREC_DOUBLES, RSREC_NS, RSREC_NT, RSREC_MUS, RSREC_MUT, RSREC_K, RSREC_CSCORE, RSREC_NF, RSREC_J, RSREC_FSCORE = 12, 0, 1, 2, 4, 6, 7, 8, 9, 10
RS_WS_COUNTS, RS_WS_CLOUDS = 16, 256
RSR_MAX_ROWS = 2048
RSBREC_DOUBLES, RSBREC_STATUS, RSBREC_EVALS, RSBREC_FEVALS = 16, 11, 12, 13
RSB_ST_OK, RSB_ST_FEW, RSB_ST_CAPACITY, RSB_ST_NO_FINE = 0, 1, 2, 3
RSB_MAX_ANGLES, RSB_MAX_ROWS = 1024, 2048
FT_MAX_ROWS, FT_MAX_KP, FT_DESC_STRIDE = 2048, 256, 32
FTREC_DOUBLES, FTREC_NS, FTREC_NT, FTREC_KPS, FTREC_KPT, FTREC_MATCHES, FTREC_INLIERS, FTREC_R, FTREC_T, FTREC_STATUS, FTREC_BEST = (
    16, 0, 1, 2, 3, 4, 5, 6, 10, 12, 13)
FT_ST_OK, FT_ST_FEW_ROWS, FT_ST_CAPACITY, FT_ST_FEW_KP, FT_ST_FEW_MATCHES, FT_ST_DESC_LEN = 0, 1, 2, 3, 4, 5
# the record of icpmi_icp_information_batch (INFO_*: H's upper triangle, g, sse, inliers, source rows, status) and the
# two sizes its kernel is built on (threads of a workgroup, target rows of an LDS tile)
INFO_DOUBLES, INFO_H, INFO_G, INFO_SSE, INFO_INLIERS, INFO_ROWS, INFO_STATUS = 16, 0, 6, 9, 10, 11, 12
INFO_THREADS, INFO_TILE_ROWS = 512, 2048
# icpmi_grid_match_batch (GM_*: capacities, the two sizes its kernels are built on, statuses) and its int32 record (GMREC_*)
GM_MAX_WINDOW, GM_MAX_ANGLES, GM_MAX_ROWS, GM_MAX_SHIFT_BITS, GM_THREADS, GM_CHUNK_ROWS = 31, 1024, 65535, 14, 256, 256
GM_ST_OK, GM_ST_EMPTY, GM_ST_CAPACITY = 0, 1, 2
GMREC_INTS, GMREC_STATUS, GMREC_ROWS, GMREC_INDEX, GMREC_A, GMREC_J, GMREC_I, GMREC_SCORE, GMREC_CENTRE = 8, 0, 1, 2, 3, 4, 5, 6, 7
# icpmi_grid_search_batch (GMW_*: its capacities, its planned survivor grid, and the four slots its record adds to GMREC_*)
GMW_MAX_WINDOW, GMW_MAX_ANGLES, GMW_SCORE_GROUPS = 255, 16384, 2048
GMW_REC_INTS, GMW_REC_BLOCKS, GMW_REC_SURVIVORS, GMW_REC_SEED, GMW_REC_MAX_BOUND = 12, 8, 9, 10, 11
# icpmi_grid_match_moments (GMOM_*: the twelve int64 slots of a pair's moments, the weight's bits, the largest half_step)
GMOM_INTS, GMOM_W, GMOM_A, GMOM_J, GMOM_I, GMOM_AA, GMOM_AJ, GMOM_AI, GMOM_JJ, GMOM_JI, GMOM_II, GMOM_SUPPORT, GMOM_EDGE = (
    12, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
GMOM_WEIGHT_BITS, GMOM_MAX_HALF_STEP = 20, 32767
# icpmi_grid_likelihood_field (LF_*: the largest radius in cells, the output tile of one workgroup)
LF_MAX_RADIUS, LF_TILE_X, LF_TILE_Y = 64, 128, 64
# icpmi_grid_cast_segments / icpmi_grid_cast_rays: the slots of a ray's int32 record and its two marks (GC_*)
GC_INTS, GC_K_HIT, GC_X_HIT, GC_Y_HIT, GC_K_UNKNOWN, GC_NONE, GC_NO_CELLS, GC_THREADS = 4, 0, 1, 2, 3, -1, -2, 256
# icpmi_grid_check_batch (GK_*: the two sizes its kernel is built on, the largest tolerance, the slots of a pair's int32 record,
# its statuses, the classes of a row with the mark of a row without cells, and the slots of a row's record)
GK_THREADS, GK_CHUNK_ROWS, GK_MAX_TOLERANCE = 256, 256, 2 ** 30
GK_INTS, GK_REC_STATUS, GK_REC_ROWS, GK_REC_CONFIRMED, GK_REC_VIOLATED, GK_REC_IN_FREE, GK_REC_UNEXPLORED, GK_REC_THROUGH_UNKNOWN = (
    8, 0, 1, 2, 3, 4, 5, 6)
GK_ST_OK, GK_ST_EMPTY, GK_ST_CAPACITY = 0, 1, 2
GK_CLASS_CONFIRMED, GK_CLASS_VIOLATED, GK_CLASS_IN_FREE, GK_CLASS_UNEXPLORED, GK_NO_CELLS = 0, 1, 2, 3, -2
GK_ROW_INTS, GK_ROW_CLASS, GK_ROW_K_HIT, GK_ROW_K, GK_ROW_K_UNKNOWN = 4, 0, 1, 2, 3
# icpmi_grid_beam_batch (GB_*: the two sizes its kernel is built on, the widest table and the clip of its entries, the slots of
# a pair's int32 record, its statuses, the index of a row without cells, and the slots of a row's record)
GB_THREADS, GB_CHUNK_ROWS, GB_MAX_HALF_WIDTH, GB_TABLE_CLIP = 256, 256, 127, 32767
GB_INTS, GB_REC_STATUS, GB_REC_ROWS, GB_REC_SCORE, GB_REC_EXPECTED, GB_REC_NOVEL, GB_REC_UNEXPLORED = 8, 0, 1, 2, 3, 4, 5
GB_ST_OK, GB_ST_EMPTY, GB_ST_CAPACITY, GB_NO_CELLS = 0, 1, 2, -2
GB_ROW_INTS, GB_ROW_INDEX, GB_ROW_K_HIT, GB_ROW_K_Z, GB_ROW_K_UNKNOWN = 4, 0, 1, 2, 3
# icpmi_pf_* (PF_*: the particle filter's capacities, the sizes its kernels are built on, the generator's purposes, the slots
# of the weights' int64 sums, the resampling's info record and statuses, the doubles of the estimate)
PF_MAX_PARTICLES, PF_THREADS, PF_PREDICT_BLOCKS, PF_PURPOSE_PREDICT, PF_PURPOSE_RESAMPLE = 2 ** 20, 256, 5, 0, 1
PF_MAX_ENTRIES, PF_MAX_SHIFT, PF_MAX_WEIGHT = 4096, 32, 2 ** 20
PF_SUMS, PF_SUM_W, PF_SUM_WW, PF_SUM_OK, PF_SUM_SMAX = 4, 0, 1, 2, 3
PF_SCAN_BLOCK, PF_SUMS_PER_LANE, PF_INFO_INTS, PF_ST_OK, PF_ST_DEGENERATE, PF_EST_CHUNK, PF_EST_DOUBLES = 1024, 4, 4, 0, 1, 1024, 8
# icpmi_pose_graph_optimize: its statuses (PG_ST_*) and the slots of its info record (PGINFO_*: three values, then PHASES clocks)
PG_ST_NOTHING, PG_ST_CONVERGED, PG_ST_MAXITER, PG_ST_SINGULAR, PG_ST_REFUSED = 0, 1, 2, 3, 4
PGINFO_DOUBLES, PGINFO_ITERATIONS, PGINFO_STATUS, PGINFO_STEP, PGINFO_PHASE_US, PGINFO_PHASES = 10, 0, 1, 2, 3, 7
# icpmi_pose_graph_marginals: the slots of its info record (its statuses are PG_ST_*) and the two paths
MARG_DOUBLES, MARG_STATUS, MARG_PATH, MARG_CLOSURES, MARG_TWINS = 4, 0, 1, 2, 3
MARG_PATH_SPLIT, MARG_PATH_DENSE = 0, 1
# icpmi_pose_graph_optimize_robust: its loss kernels and the three slots its info record adds to PGINFO_*
ROB_KERNEL_HUBER, ROB_KERNEL_CAUCHY, ROB_KERNEL_GEMAN_MCCLURE = 0, 1, 2
ROB_DOUBLES, ROB_COST_BEFORE, ROB_COST_AFTER, ROB_WEIGHTS_US = 13, 10, 11, 12
# icpmi_grid_update_plan: the counting pass of a ray-cast call
RC_PASS_NONE, RC_PASS_OWNER, RC_PASS_TILES, RC_PASS_ATOMIC = 0, 1, 2, 3
INFO_SLOTS = ("H_tt", "H_tx", "H_ty", "H_xx", "H_xy", "H_yy", "g_t", "g_x", "g_y", "sse", "inliers", "rows", "status")


class IcpParams(C.Structure):
    _fields_ = [("error_threshold", C.c_double), ("max_corr_dist", C.c_double),
                ("max_iterations", C.c_int32), ("method", C.c_int32),
                ("has_init", C.c_int32), ("dim", C.c_int32)]


class History(C.Structure):
    """icpmi_history (include/icpmi.h): the device buffers of a resident scan history."""
    _fields_ = [("pts", C.c_void_p), ("off_dev", C.c_void_p), ("ids", C.c_void_p), ("icp_vox", C.c_void_p), ("icp_cnt", C.c_void_p),
                ("icp_prepared", C.c_void_p), ("rs_vox", C.c_void_p), ("rs_cnt", C.c_void_p), ("rs_means", C.c_void_p),
                ("rs_prepared", C.c_void_p), ("voxel_ws", C.c_void_p), ("prepared_bytes", C.c_size_t), ("voxel_ws_bytes", C.c_size_t),
                ("icp_voxel", C.c_double), ("rs_voxel", C.c_double), ("scan_capacity", C.c_int32), ("row_capacity", C.c_int32),
                ("normal_k", C.c_int32), ("allow_polar", C.c_int32)]


class FeatureStore(C.Structure):
    """icpmi_feature_store (include/icpmi.h): a history's per-cloud feature tables and the configuration they were made with."""
    _fields_ = [("vox", C.c_void_p), ("curv", C.c_void_p), ("cnt", C.c_void_p), ("kp", C.c_void_p), ("kp_cnt", C.c_void_p),
                ("desc", C.c_void_p), ("desc_len", C.c_void_p), ("voxel_size", C.c_double), ("min_kp_dist", C.c_double),
                ("k_curvature", C.c_int32), ("top_n", C.c_int32), ("k_descriptor", C.c_int32), ("kp_stride", C.c_int32)]


class GridPlan(C.Structure):
    """icpmi_grid_plan (include/icpmi.h): what one icpmi_grid_update_scans_box call starts, from its host arguments."""
    _fields_ = [("pass_", C.c_int32), ("group_max", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("live_scans", C.c_int32), ("wide", C.c_int32)]


class IcpmiError(RuntimeError):
    pass


def build(verbose=False):
    """Compile the HIP sources for gfx950 into lib/libicpmi.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4", "all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise IcpmiError("building libicpmi.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout)
    return LIB_PATH


_SIGS = {
    # name: (restype, argtypes)
    "icpmi_version": (C.c_char_p, []),
    "icpmi_strerror": (C.c_char_p, [C.c_int]),
    "icpmi_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "icpmi_shutdown": (C.c_int, []),
    "icpmi_runtime_check": (C.c_int, [C.c_char_p, C.c_size_t]),
    "icpmi_voxel_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "icpmi_voxel_downsample_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_nn_batch": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_void_p]),
    "icpmi_normals_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "icpmi_normals_2d_batch": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "icpmi_p2l_solve_2d": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_icp_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "icpmi_icp_batch": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.POINTER(IcpParams), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_icp_batch_gated": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.POINTER(IcpParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_icp_information_batch": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                              C.c_void_p, C.c_void_p]),
    "icpmi_prepared_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "icpmi_prepare_targets": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "icpmi_prepare_targets_ex": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_int32, C.c_void_p]),
    "icpmi_nn_prepared_batch": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_void_p]),
    "icpmi_rotation_scores": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                        C.c_double, C.c_void_p, C.c_void_p]),
    "icpmi_rotation_search_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "icpmi_rotation_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "icpmi_rotation_refine_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "icpmi_rotation_refine": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                        C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_rotation_search_batch_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "icpmi_rotation_search_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_history_add": (C.c_int, [C.POINTER(History), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "icpmi_history_search": (C.c_int, [C.POINTER(History), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_history_world_rows": (C.c_int, [C.POINTER(History), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_history_features_add": (C.c_int, [C.POINTER(History), C.POINTER(FeatureStore), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "icpmi_history_feature_align_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "icpmi_history_feature_align": (C.c_int, [C.POINTER(History), C.POINTER(FeatureStore)] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32,
                                              C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32] +
                                    [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "icpmi_prepared_relayout": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32,
                                          C.c_int32, C.c_void_p]),
    "icpmi_feature_curvature_batch": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_feature_keypoints_batch": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "icpmi_feature_descriptors_batch": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_feature_match_batch": (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_feature_ransac_batch": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 +
                                   [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_feature_align_batch_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
    "icpmi_feature_align_batch": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_double, C.c_int32,
                                            C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "icpmi_world_to_grid": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "icpmi_bresenham_cells": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_grid_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "icpmi_grid_update_scans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                          C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_void_p]),
    "icpmi_grid_update_scans_band": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                               C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                               C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_void_p]),
    "icpmi_grid_update_scans_box": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                              C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                              C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_grid_update_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.POINTER(GridPlan)]),
    "icpmi_grid_score_field": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_grid_match_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "icpmi_grid_match_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 4 +
                               [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_bound_field": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_grid_search_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "icpmi_grid_search_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 4 +
                                [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_match_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "icpmi_grid_likelihood_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "icpmi_grid_likelihood_field": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_occupancy_planes_bytes": (C.c_size_t, [C.c_int32] * 2),
    "icpmi_grid_occupancy_planes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_cast_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_cast_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "icpmi_grid_check_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double] +
                               [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_grid_beam_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double] +
                              [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32] +
                              [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_pf_predict": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_double] * 6 + [C.c_uint64, C.c_uint32, C.c_void_p]),
    "icpmi_pf_weights": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_pf_resample": (C.c_int, [C.c_int32] + [C.c_void_p] * 9 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "icpmi_pf_estimate": (C.c_int, [C.c_int32] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "icpmi_pf_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "icpmi_pose_graph_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "icpmi_pose_graph_optimize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    "icpmi_pose_graph_weighted_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "icpmi_pose_graph_dense_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "icpmi_pose_graph_optimize_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
    "icpmi_pose_graph_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "icpmi_pose_graph_marginals_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5),
    "icpmi_pose_graph_marginals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
    "icpmi_pose_graph_robust_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "icpmi_pose_graph_optimize_robust": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_double, C.c_int32, C.c_double, C.c_int32] +
                                         [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def lib():
    """The loaded library; raises IcpmiError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IcpmiError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(or `make -C iterative-closest-point-avmi_amd/csrc`). There is no CPU fallback.")
        # torch first: it ships its own HIP runtime (libamdhip64 inside the wheel), and the process must hold ONE — the
        # streams and allocations torch hands us have to belong to the runtime our launches go through.  Loaded before
        # torch, libicpmi.so would bring in /opt/rocm's copy and torch its own beside it: every launch then fails with
        # a HIP runtime error (seen: build() followed by smoke() in one process).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)          # AttributeError here means the .so is stale
            f.restype, f.argtypes = res, args
        _lib = L
        why = runtime_problem()
        if why:
            _lib = None
            raise IcpmiError(why)
    return _lib


def runtime_problem():
    """'' or what icpmi_runtime_check found: two copies of libamdhip64 mapped into this process (every launch would fail)."""
    if _lib is None:
        return ""
    buf = C.create_string_buffer(1024)
    return buf.value.decode() if _lib.icpmi_runtime_check(buf, len(buf)) != OK else ""


ERR_HIP = -3


def check(code, what):
    if code != OK:
        hint = runtime_problem() if code == ERR_HIP else ""
        raise IcpmiError(f"{what}: {lib().icpmi_strerror(code).decode()} ({code})" + (f" [{hint}]" if hint else ""))


def set_option(name, value):
    """icpmi_set_option: change one of the library's ICPMI_* switches after it has read the environment (None unsets)."""
    check(lib().icpmi_set_option(name.encode(), None if value is None else str(value).encode()), f"set_option({name})")


def shutdown():
    """icpmi_shutdown: destroy the side streams and events the library made (made again on demand)."""
    if _lib is not None:
        check(_lib.icpmi_shutdown(), "shutdown")
