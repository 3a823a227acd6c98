"""ctypes binding of liblmgpu.so (C ABI declared in include/lmgpu.h).

The library is built in-tree by `make -C gtsam_personal_amd/csrc` (see __graft_entry__.build()).
There is no Python/CPU fallback: if the shared object is missing, importing the hot path fails loudly.
"""
from __future__ import annotations

import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblmgpu.so")

LMGPU_OK, LMGPU_INDETERMINATE, LMGPU_INVALID, LMGPU_HIP_ERROR = 0, 1, 2, 3


class lmgpu_config(ct.Structure):
    _fields_ = [("device", ct.c_int32), ("rank", ct.c_int32), ("world_size", ct.c_int32), ("flags", ct.c_int32)]


class lmgpu_lm_params(ct.Structure):
    _fields_ = [
        ("maxIterations", ct.c_int32),
        ("relativeErrorTol", ct.c_double), ("absoluteErrorTol", ct.c_double), ("errorTol", ct.c_double),
        ("lambdaInitial", ct.c_double), ("lambdaFactor", ct.c_double), ("lambdaUpperBound", ct.c_double), ("lambdaLowerBound", ct.c_double),
        ("minModelFidelity", ct.c_double),
        ("diagonalDamping", ct.c_int32), ("useFixedLambdaFactor", ct.c_int32),
        ("minDiagonal", ct.c_double), ("maxDiagonal", ct.c_double),
    ]


class lmgpu_lm_state(ct.Structure):
    _fields_ = [("error", ct.c_double), ("lambda_", ct.c_double), ("currentFactor", ct.c_double), ("iterations", ct.c_int32),
                ("totalNumberInnerIterations", ct.c_int32)]


class lmgpu_isam2_params(ct.Structure):
    _fields_ = [("relinearizeThreshold", ct.c_double), ("relinearizeSkip", ct.c_int32), ("enableRelinearization", ct.c_int32),
                ("wildfireThreshold", ct.c_double)]


class lmgpu_isam2_result(ct.Structure):
    _fields_ = [("variablesRelinearized", ct.c_int32), ("variablesReeliminated", ct.c_int32), ("factorsRecalculated", ct.c_int32),
                ("cliques", ct.c_int32), ("batch", ct.c_int32)]


class lmgpu_isam2_update_params(ct.Structure):
    _fields_ = [("n_remove", ct.c_int32), ("removeFactorIndices", ct.POINTER(ct.c_uint64)), ("has_constrained", ct.c_int32),
                ("n_constrained", ct.c_int32), ("constrainedKeys", ct.POINTER(ct.c_uint64)), ("constrainedGroups", ct.POINTER(ct.c_int32)),
                ("n_no_relin", ct.c_int32), ("noRelinKeys", ct.POINTER(ct.c_uint64)), ("n_extra_reelim", ct.c_int32),
                ("extraReelimKeys", ct.POINTER(ct.c_uint64)), ("force_relinearize", ct.c_int32), ("forceFullSolve", ct.c_int32)]


# lmgpu_ccolamd_fn: int fn(user, n_rows, n_cols, col_ptr, row_idx, cmember, perm_out)
CCOLAMD_FN = ct.CFUNCTYPE(ct.c_int, ct.c_void_p, ct.c_int32, ct.c_int32, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int32),
                          ct.POINTER(ct.c_int32))


class lmgpu_timings(ct.Structure):
    _fields_ = [("linearize_ms", ct.c_double), ("eliminate_ms", ct.c_double), ("backsub_ms", ct.c_double), ("linear_error_ms", ct.c_double),
                ("retract_error_ms", ct.c_double), ("total_ms", ct.c_double), ("inner_iterations", ct.c_int32)]


LMGPU_SOLVER_MULTIFRONTAL_CHOLESKY, LMGPU_SOLVER_PCG = 0, 1
LMGPU_PRECOND_DUMMY, LMGPU_PRECOND_BLOCK_JACOBI = 0, 1


class lmgpu_pcg_params(ct.Structure):
    _fields_ = [("preconditioner", ct.c_int32), ("minIterations", ct.c_int32), ("maxIterations", ct.c_int32), ("reset", ct.c_int32),
                ("epsilon_rel", ct.c_double), ("epsilon_abs", ct.c_double)]


class lmgpu_pcg_stats(ct.Structure):
    _fields_ = [("iterations", ct.c_int32), ("host_waits", ct.c_int32), ("gamma0", ct.c_double), ("gamma", ct.c_double),
                ("threshold", ct.c_double), ("precond_ms", ct.c_double), ("iterate_ms", ct.c_double)]


LMGPU_INIT_POSE3_ANCHOR_KEY = 99999999

LMGPU_GNC_GM, LMGPU_GNC_TLS = 0, 1
LMGPU_GNC_BASE_LM, LMGPU_GNC_BASE_GN = 0, 1
GNC_STOP_REASONS = ("maxIterations", "cost", "weights", "mu", "mu <= 0 at initialisation", "nothing unknown")


class lmgpu_gnc_params(ct.Structure):
    _fields_ = [("lossType", ct.c_int32), ("maxIterations", ct.c_int32), ("baseOptimizer", ct.c_int32), ("muStep", ct.c_double),
                ("relativeCostTol", ct.c_double), ("weightsTol", ct.c_double)]


class lmgpu_gnc_result(ct.Structure):
    _fields_ = [("iterations", ct.c_int32), ("stop", ct.c_int32), ("mu", ct.c_double), ("cost", ct.c_double), ("prev_cost", ct.c_double),
                ("base_iterations_total", ct.c_int32)]


LMGPU_NCG_FLETCHER_REEVES, LMGPU_NCG_POLAK_RIBIERE, LMGPU_NCG_HESTENES_STIEFEL, LMGPU_NCG_DAI_YUAN = 0, 1, 2, 3


class lmgpu_ncg_params(ct.Structure):
    _fields_ = [("direction_method", ct.c_int32), ("gradient_descent", ct.c_int32), ("max_iterations", ct.c_int32),
                ("relative_error_tol", ct.c_double), ("absolute_error_tol", ct.c_double), ("error_tol", ct.c_double)]


class lmgpu_debug_ncg_ctl(ct.Structure):
    """test hooks only (liblmgpu_test.so): the device's line-search record, NcgCtl of csrc/kernels_ncg.hpp"""
    _fields_ = [(f, ct.c_double) for f in ("minStep", "maxStep", "newStep", "newError", "step", "alpha", "error", "beta", "dnorm")] + [
        (f, ct.c_int32) for f in ("done", "trials", "flag", "first")]


LMGPU_TRI_VALID, LMGPU_TRI_DEGENERATE, LMGPU_TRI_BEHIND_CAMERA, LMGPU_TRI_OUTLIER, LMGPU_TRI_FAR_POINT, LMGPU_TRI_CALIBRATE_FAILED = 0, 1, 2, 3, 4, 5
LMGPU_TRI_CAM_BUNDLER, LMGPU_TRI_CAM_S2 = 0, 1  # camera_model of lmgpu_triangulate_batch


class lmgpu_triangulation_params(ct.Structure):
    _fields_ = [("rankTolerance", ct.c_double), ("enableEPI", ct.c_int32), ("useLOST", ct.c_int32), ("landmarkDistanceThreshold", ct.c_double),
                ("dynamicOutlierRejectionThreshold", ct.c_double), ("noise_inv_sigma", ct.c_double)]


class lmgpu_triangulation_stats(ct.Structure):
    _fields_ = [("n_points", ct.c_int32), ("n_status", ct.c_int32 * 6), ("max_iterations", ct.c_int32), ("sum_iterations", ct.c_int64),
                ("device_ms", ct.c_double)]


LMGPU_SMART_HESSIAN, LMGPU_SMART_IMPLICIT_SCHUR, LMGPU_SMART_JACOBIAN_Q, LMGPU_SMART_JACOBIAN_SVD = 0, 1, 2, 3
LMGPU_SMART_IGNORE_DEGENERACY, LMGPU_SMART_ZERO_ON_DEGENERACY, LMGPU_SMART_HANDLE_INFINITY = 0, 1, 2


class lmgpu_smart_params(ct.Structure):
    _fields_ = [("linearizationMode", ct.c_int32), ("degeneracyMode", ct.c_int32), ("retriangulationThreshold", ct.c_double),
                ("triangulation", lmgpu_triangulation_params)]


class lmgpu_smart_stats(ct.Structure):
    _fields_ = [("n_factors", ct.c_int32), ("retriangulations", ct.c_int32), ("n_status", ct.c_int32 * 6), ("triangulate_ms", ct.c_double),
                ("linearize_ms", ct.c_double)]


class lmgpu_marginals_stats(ct.Structure):
    _fields_ = [("launches", ct.c_int64), ("chunks", ct.c_int64), ("factorizations", ct.c_int64), ("vars_lds", ct.c_int64),
                ("vars_scratch", ct.c_int64), ("scratch_bytes", ct.c_int64), ("longest_path", ct.c_int32), ("lds_capacity", ct.c_int32),
                ("cross_launches", ct.c_int64), ("cross_chunks", ct.c_int64), ("cross_walks", ct.c_int64), ("cross_targets", ct.c_int64),
                ("cross_lds", ct.c_int64), ("cross_scratch", ct.c_int64), ("longest_union", ct.c_int32), ("cross_cap", ct.c_int32)]


class lmgpu_mfas_stats(ct.Structure):
    _fields_ = [("n_nodes", ct.c_int32), ("global_state", ct.c_int32), ("lds_node_capacity", ct.c_int32), ("pad_", ct.c_int32),
                ("kernel_ms", ct.c_double)]


# every symbol include/lmgpu.h declares: name -> (restype, argtypes)
_H = ct.c_void_p
_D = ct.POINTER(ct.c_double)
_I = ct.POINTER(ct.c_int32)
SYMBOLS = {
    "lmgpu_create": (ct.c_int, [ct.POINTER(lmgpu_config), ct.POINTER(_H)]),
    "lmgpu_destroy": (ct.c_int, [_H]),
    "lmgpu_last_error": (ct.c_char_p, [_H]),
    "lmgpu_last_failed_slot": (ct.c_int, [_H]),
    "lmgpu_set_variables": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _I]),
    "lmgpu_add_factor_bucket": (ct.c_int, [_H, ct.c_int32, ct.c_int32, _I, _I, _D, ct.c_int32, _D]),
    "lmgpu_add_factor_bucket_robust": (ct.c_int, [_H, ct.c_int32, ct.c_int32, _I, _I, _D, ct.c_int32, _D, ct.c_int32, ct.c_double]),
    "lmgpu_finalize_structure": (ct.c_int, [_H]),
    "lmgpu_set_values": (ct.c_int, [_H, _D]),
    "lmgpu_get_values": (ct.c_int, [_H, _D]),
    "lmgpu_save_values": (ct.c_int, [_H]),
    "lmgpu_restore_values": (ct.c_int, [_H]),
    "lmgpu_total_dim": (ct.c_int, [_H]),
    "lmgpu_total_store": (ct.c_int, [_H]),
    "lmgpu_error": (ct.c_int, [_H, _D]),
    "lmgpu_linearize": (ct.c_int, [_H]),
    "lmgpu_solve": (ct.c_int, [_H, ct.c_double, ct.c_int32, ct.c_double, ct.c_double, _D, _D, _D]),
    "lmgpu_retract": (ct.c_int, [_H, _D]),
    "lmgpu_hessian_diagonal": (ct.c_int, [_H, _D]),
    "lmgpu_lm_init": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_iterate": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_optimize": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_gn_iterate": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_gn_optimize": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_dl_iterate": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_dl_optimize": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_get_timings": (ct.c_int, [_H, ct.POINTER(lmgpu_timings)]),
    "lmgpu_set_linear_solver": (ct.c_int, [_H, ct.c_int32, ct.POINTER(lmgpu_pcg_params)]),
    "lmgpu_get_pcg_stats": (ct.c_int, [_H, ct.POINTER(lmgpu_pcg_stats)]),
    "lmgpu_chi2inv": (ct.c_double, [ct.c_double, ct.c_int32]),
    "lmgpu_gnc_enable": (ct.c_int, [_H, ct.c_int32, ct.c_int32]),
    "lmgpu_gnc_set_inlier_cost_thresholds": (ct.c_int, [_H, ct.c_int32, _D, ct.c_double]),
    "lmgpu_gnc_set_known": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), ct.c_int32, ct.POINTER(ct.c_uint64)]),
    "lmgpu_gnc_set_weights": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_gnc_get_weights": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_gnc_get_inlier_cost_thresholds": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_gnc_initialize_mu": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_gnc_calculate_weights": (ct.c_int, [_H, ct.c_int32, ct.c_double]),
    "lmgpu_gnc_optimize": (ct.c_int, [_H, ct.POINTER(lmgpu_gnc_params), ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state),
                                      ct.POINTER(lmgpu_gnc_result)]),
    "lmgpu_gnc_get_trace": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_gradient": (ct.c_int, [_H, _D]),
    "lmgpu_ncg_line_search": (ct.c_int, [_H, _D, _D, _I]),
    "lmgpu_ncg_iterate": (ct.c_int, [_H, ct.POINTER(lmgpu_ncg_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_ncg_optimize": (ct.c_int, [_H, ct.POINTER(lmgpu_ncg_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_ncg_get_trace": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_ncg_host_waits": (ct.c_int, [_H]),
    "lmgpu_init_pose3_create": (ct.c_int, [ct.POINTER(lmgpu_config), ct.POINTER(_H)]),
    "lmgpu_init_pose3_destroy": (ct.c_int, [_H]),
    "lmgpu_init_pose3_last_error": (ct.c_char_p, [_H]),
    "lmgpu_init_pose3_add_factors": (ct.c_int, [_H, ct.c_int32, ct.c_int32, _I, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D]),
    "lmgpu_init_pose3_finalize": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64)]),
    "lmgpu_init_pose3_num_poses": (ct.c_int, [_H]),
    "lmgpu_init_pose3_num_factors": (ct.c_int, [_H]),
    "lmgpu_init_pose3_get_slots": (ct.c_int, [_H, ct.POINTER(ct.c_uint64)]),
    "lmgpu_init_pose3_handle": (ct.c_void_p, [_H, ct.c_int32]),
    "lmgpu_init_pose3_orientations_chordal": (ct.c_int, [_H, _D]),
    "lmgpu_init_pose3_closest_rotations": (ct.c_int, [ct.c_int32, ct.c_int32, _D, _D]),
    "lmgpu_init_pose3_orientations_gradient": (ct.c_int, [_H, _D, ct.c_int32, ct.c_int32, _D, _I, _D]),
    "lmgpu_init_pose3_compute_poses": (ct.c_int, [_H, _D, ct.c_int32, _D, ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_init_pose3_initialize": (ct.c_int, [_H, _D, ct.c_int32, _D]),
    "lmgpu_translation_recovery_create": (ct.c_int, [ct.POINTER(lmgpu_config), ct.POINTER(_H)]),
    "lmgpu_translation_recovery_destroy": (ct.c_int, [_H]),
    "lmgpu_translation_recovery_last_error": (ct.c_char_p, [_H]),
    "lmgpu_translation_recovery_seed": (ct.c_int, [_H, ct.c_uint32]),
    "lmgpu_translation_recovery_set_prior_sigma": (ct.c_int, [_H, ct.c_double]),
    "lmgpu_translation_recovery_add_directions": (ct.c_int, [_H, ct.c_int32, _I, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D, ct.c_int32, ct.c_double]),
    "lmgpu_translation_recovery_add_betweens": (ct.c_int, [_H, ct.c_int32, _I, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D, ct.c_int32, ct.c_double]),
    "lmgpu_translation_recovery_finalize": (ct.c_int, [_H, ct.c_double, ct.c_int32, ct.POINTER(ct.c_uint64), _D, ct.c_int32, ct.POINTER(ct.c_uint64)]),
    "lmgpu_translation_recovery_num_keys": (ct.c_int, [_H]),
    "lmgpu_translation_recovery_num_factors": (ct.c_int, [_H]),
    "lmgpu_translation_recovery_get_keys": (ct.c_int, [_H, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint64)]),
    "lmgpu_translation_recovery_get_slots": (ct.c_int, [_H, ct.POINTER(ct.c_uint64)]),
    "lmgpu_translation_recovery_get_initial": (ct.c_int, [_H, _D]),
    "lmgpu_translation_recovery_handle": (ct.c_void_p, [_H]),
    "lmgpu_translation_recovery_run": (ct.c_int, [_H, ct.POINTER(lmgpu_lm_params), ct.POINTER(lmgpu_lm_state)]),
    "lmgpu_translation_recovery_get": (ct.c_int, [_H, _D]),
    "lmgpu_mfas_outlier_weights": (ct.c_int, [ct.c_int32, ct.c_int32, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D, _D, ct.POINTER(ct.c_uint64), _D, _D,
                                              ct.POINTER(lmgpu_mfas_stats)]),
    "lmgpu_mfas_lds_node_capacity": (ct.c_int, []),
    "lmgpu_mfas_last_error": (ct.c_char_p, []),
    "lmgpu_set_kernel_timing": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_get_kernel_times": (ct.c_int, [_H, _D, _D, ct.POINTER(ct.c_int64)]),
    "lmgpu_get_jacobian": (ct.c_int, [_H, ct.c_int32, _D, _I, _I]),
    "lmgpu_get_jacobians": (ct.c_int, [_H, _I, _I, _I, _I, ct.POINTER(ct.c_int64), _D]),
    "lmgpu_num_fronts": (ct.c_int, [_H]),
    "lmgpu_front_info": (ct.c_int, [_H, ct.c_int32, _I]),
    "lmgpu_leaf_group_launches": (ct.c_int, [_H]),
    "lmgpu_backsub_group_launches": (ct.c_int, [_H, _I]),
    "lmgpu_get_leaf_corner": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_get_front": (ct.c_int, [_H, ct.c_int32, _I, _D]),
    "lmgpu_comm_unique_id": (ct.c_int, [ct.c_char_p]),
    "lmgpu_comm_init": (ct.c_int, [_H, ct.c_char_p]),
    "lmgpu_marginal_covariance": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_joint_marginal_covariance": (ct.c_int, [_H, ct.c_int32, _I, _D]),
    "lmgpu_marginals_factor": (ct.c_int, [_H]),
    "lmgpu_marginal_covariances": (ct.c_int, [_H, ct.c_int32, _I, _D]),
    "lmgpu_marginals_path": (ct.c_int, [_H, ct.c_int32, _I, ct.c_int32]),
    "lmgpu_marginals_front_offsets": (ct.c_int, [_H, ct.c_int32, _I, _I, ct.c_int32]),
    "lmgpu_set_marginals_params": (ct.c_int, [_H, ct.c_int64, ct.c_int32]),
    "lmgpu_get_marginals_stats": (ct.c_int, [_H, ct.POINTER(lmgpu_marginals_stats)]),
    "lmgpu_marginal_cross_covariances": (ct.c_int, [_H, ct.c_int32, _I, _I, _D]),
    "lmgpu_joint_marginal_covariances": (ct.c_int, [_H, ct.c_int32, _I, _I, _D]),
    "lmgpu_marginals_junction": (ct.c_int, [_H, ct.c_int32, ct.c_int32]),
    "lmgpu_set_marginals_cross_cap": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_selftest_chain_schedule": (ct.c_int, [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int]),
    "lmgpu_selftest_dense_schedule": (ct.c_int, [ct.c_int, ct.c_int, ct.c_int, ct.c_uint, ct.c_int, _I]),
    "lmgpu_selftest_dogleg_step": (ct.c_int, [ct.c_int, _D, _D]),
    "lmgpu_selftest_factor_type": (ct.c_int, [ct.c_int32, _I]),
    "lmgpu_selftest_var_type": (ct.c_int, [ct.c_int32, _I]),
    "lmgpu_bt_products": (ct.c_int, [_H, _D, ct.c_double, _D, _D]),
    "lmgpu_triangulate_batch": (ct.c_int, [ct.c_int32, ct.c_int32, ct.c_int32, _D, ct.c_int32, _I, _I, _D, ct.POINTER(lmgpu_triangulation_params),
                                           _D, _I]),
    "lmgpu_triangulate_landmarks": (ct.c_int, [_H, ct.POINTER(lmgpu_triangulation_params), ct.c_int32, _D, _I, _I]),
    "lmgpu_num_points3": (ct.c_int, [_H]),
    "lmgpu_get_triangulation_stats": (ct.c_int, [_H, ct.POINTER(lmgpu_triangulation_stats)]),
    "lmgpu_add_smart_factors": (ct.c_int, [_H, ct.c_int32, _I, _I, _I, _D, _D, _D, ct.POINTER(lmgpu_smart_params)]),
    "lmgpu_num_smart_factors": (ct.c_int, [_H]),
    "lmgpu_smart_get_points": (ct.c_int, [_H, _D, _I]),
    "lmgpu_smart_get_hessian": (ct.c_int, [_H, ct.c_int32, _I, _D]),
    "lmgpu_smart_reset": (ct.c_int, [_H]),
    "lmgpu_get_smart_stats": (ct.c_int, [_H, ct.POINTER(lmgpu_smart_stats)]),
    "lmgpu_isam2_create": (ct.c_int, [ct.POINTER(lmgpu_config), ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.POINTER(_H)]),
    "lmgpu_isam2_destroy": (ct.c_int, [_H]),
    "lmgpu_isam2_last_error": (ct.c_char_p, [_H]),
    "lmgpu_isam2_last_failed_key": (ct.c_uint64, [_H]),
    "lmgpu_isam2_add_variables": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _I, _D]),
    "lmgpu_isam2_add_factors": (ct.c_int, [_H, ct.c_int32, ct.c_int32, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D]),
    "lmgpu_isam2_add_factors_robust": (ct.c_int, [_H, ct.c_int32, ct.c_int32, ct.POINTER(ct.c_uint64), _D, ct.c_int32, _D, ct.c_int32, ct.c_double]),
    "lmgpu_isam2_update": (ct.c_int, [_H, ct.c_int32, ct.c_void_p]),
    "lmgpu_isam2_update_with": (ct.c_int, [_H, ct.c_void_p, ct.c_void_p]),
    "lmgpu_isam2_set_relinearize_thresholds": (ct.c_int, [_H, ct.c_int32, ct.c_char_p, _I, _D]),
    "lmgpu_isam2_set_partial_relinearization_check": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_isam2_set_dogleg": (ct.c_int, [_H, ct.c_double, ct.c_double, ct.c_int32]),
    "lmgpu_isam2_get_dogleg_delta": (ct.c_double, [_H]),
    "lmgpu_isam2_set_evaluate_nonlinear_error": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_isam2_get_errors": (ct.c_int, [_H, _D, _D]),
    "lmgpu_isam2_error": (ct.c_int, [_H, ct.c_int32, _D]),
    "lmgpu_isam2_get_unused_keys": (ct.c_int, [_H, ct.POINTER(ct.c_uint64)]),
    "lmgpu_isam2_factor_exists": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_isam2_set_find_unused_factor_slots": (ct.c_int, [_H, ct.c_int32]),
    "lmgpu_isam2_marginalize_leaves": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _I, _I]),
    "lmgpu_isam2_get_marginalize_result": (ct.c_int, [_H, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint64)]),
    "lmgpu_isam2_get_fixed_variables": (ct.c_int, [_H, ct.POINTER(ct.c_uint64)]),
    "lmgpu_isam2_get_marginal_factor": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _I, _D]),
    "lmgpu_isam2_num_variables": (ct.c_int, [_H]),
    "lmgpu_isam2_num_factors": (ct.c_int, [_H]),
    "lmgpu_isam2_get_values": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _I, _D]),
    "lmgpu_isam2_get_value": (ct.c_int, [_H, ct.c_int32, ct.c_uint64, _I, _D]),
    "lmgpu_isam2_get_delta": (ct.c_int, [_H, _D]),
    "lmgpu_isam2_marginal_covariance": (ct.c_int, [_H, ct.c_uint64, _D]),
    "lmgpu_isam2_marginal_covariances": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _D]),
    "lmgpu_isam2_cross_covariances": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint64), _D]),
    "lmgpu_isam2_joint_marginal_covariances": (ct.c_int, [_H, ct.c_int32, _I, ct.POINTER(ct.c_uint64), _D]),
    "lmgpu_isam2_marginals_path": (ct.c_int, [_H, ct.c_uint64, ct.POINTER(ct.c_uint64), ct.c_int32]),
    "lmgpu_isam2_marginals_junction": (ct.c_int, [_H, ct.c_uint64, ct.c_uint64, ct.POINTER(ct.c_uint64)]),
    "lmgpu_isam2_set_marginals_params": (ct.c_int, [_H, ct.c_int64, ct.c_int32, ct.c_int32]),
    "lmgpu_isam2_get_marginals_stats": (ct.c_int, [_H, ct.POINTER(lmgpu_marginals_stats)]),
    "lmgpu_isam2_num_cliques": (ct.c_int, [_H]),
    "lmgpu_isam2_clique_info": (ct.c_int, [_H, ct.c_int32, _I]),
    "lmgpu_isam2_get_clique": (ct.c_int, [_H, ct.c_int32, ct.POINTER(ct.c_uint64), _D]),
    "lmgpu_peak_mfma_f64": (ct.c_int, [ct.c_int32, ct.c_int32, _D]),
    "lmgpu_peak_mfma_f64_clock": (ct.c_int, [ct.c_int32, ct.c_int32, ct.c_int32, _D, _D, _D]),
    "lmgpu_peak_hbm_copy": (ct.c_int, [ct.c_int32, ct.c_int64, ct.c_int32, _D]),
}

# test hooks: liblmgpu_test.so only (include/lmgpu.h, LMGPU_TEST_HOOKS)
TEST_SYMBOLS = {
    "lmgpu_local_group_create": (ct.c_int, [ct.c_int32, ct.POINTER(ct.c_void_p)]),
    "lmgpu_local_group_destroy": (ct.c_int, [ct.c_void_p]),
    "lmgpu_comm_init_local": (ct.c_int, [_H, ct.c_void_p]),
    "lmgpu_debug_table_digest": (ct.c_int, [_H, ct.c_int32, ct.c_char_p, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint64)]),
    "lmgpu_debug_ncg_direction": (ct.c_int, [ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, _D, _D, _D, _D, _I, ct.POINTER(lmgpu_debug_ncg_ctl)]),
    "lmgpu_debug_ncg_ls_control": (ct.c_int, [ct.c_int32, ct.POINTER(lmgpu_debug_ncg_ctl), ct.c_int32, _D, ct.c_int32, ct.POINTER(lmgpu_debug_ncg_ctl)]),
    "lmgpu_debug_ncg_reduce": (ct.c_int, [ct.c_int32, ct.c_int32, _D, ct.c_int32, ct.c_double, _D]),
}

KT_NAMES = ("linearize", "lds_front", "hbm_assemble", "panel", "syrk", "backsub_hbm", "backsub_lds", "linear_error", "retract_error", "allreduce", "chain")

_lib = None
_lib_test = None
TEST_LIB_PATH = os.path.join(_HERE, "liblmgpu_test.so")


_prefer_test_library = False


def use_test_library(on: bool):
    """tests only: make load() hand out liblmgpu_test.so -- the build that reads the LMGPU_* development switches from the environment
    (A/B forms of the same arithmetic, tests/test_gpu_lookahead.py) and exports the in-process communicator.  The product library reads
    none of them."""
    global _prefer_test_library
    _prefer_test_library = bool(on)


def load(test_hooks=False):
    """Load liblmgpu.so once; raises if it has not been built (no fallback).  test_hooks=True: liblmgpu_test.so, the same library
    built with the in-process communicator the sharded-loop test needs and the development switches (never used by the product path)."""
    global _lib, _lib_test
    if test_hooks or _prefer_test_library:
        if _lib_test is None:
            if not os.path.exists(TEST_LIB_PATH):
                raise ImportError(f"{TEST_LIB_PATH} not built: run `make -C gtsam_personal_amd/csrc`")
            lib = ct.CDLL(TEST_LIB_PATH)
            for name, (res, args) in list(SYMBOLS.items()) + list(TEST_SYMBOLS.items()):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib_test = lib
        return _lib_test
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or `make -C gtsam_personal_amd/csrc`). The LM hot path has no CPU fallback.")
        lib = ct.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class LmgpuError(RuntimeError):
    pass


class IndeterminantLinearSystemException(LmgpuError):
    """mirror of gtsam/linear/linearExceptions.h; `slot` is the first frontal variable of the failing front"""

    def __init__(self, slot):
        super().__init__(f"indeterminant linear system near variable slot {slot}")
        self.slot = slot
