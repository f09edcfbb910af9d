"""Python mirror of the reference's operator surface over libdliom.so (C ABI in
include/dliom.h).  Class and method names follow cartographer::mapping so the
parity tests read like the reference's own tests:

    HybridGrid                          mapping/3d/hybrid_grid.h:470-547
    RangeDataInserter3D                 mapping/3d/range_data_inserter_3d.h:35-47
    RealTimeCorrelativeScanMatcher3D    .../real_time_correlative_scan_matcher_3d.h:34-66
    CeresScanMatcher3D                  .../ceres_scan_matcher_3d.h:37-63

Everything here calls the HIP library; there is NO CPU fallback.  Importing the
package without a built libdliom.so, or creating a Context without a GPU, fails
loudly (DliomError).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libdliom.so")


class DliomError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = _lib.dliom_status_string(status).decode() if _lib is not None else "library not loaded"
        detail = _lib.dliom_last_error().decode() if _lib is not None and status == -2 else ""
        super().__init__("%s: %s (%d) %s" % (where, msg, status, detail))


OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_HIP = -2
ERR_NO_DEVICE = -3
ERR_SCORE_NOT_POSITIVE = -4
ERR_WEIGHTS = -5
ERR_GRID_EXTENT = -6
ERR_RAY_TOO_LONG = -7
ERR_EMPTY_CLOUD = -8
ERR_CAPACITY = -9
ERR_SOLVER = -10
ERR_PEER_FAILED = -12
TUNE_SCORE_KERNEL, TUNE_CSM_ONE_LAUNCH_MAX, TUNE_RESERVED_TEST_HOOK = 0, 1, 2
HOOKS_LIB_PATH = os.path.join(os.path.dirname(_HERE), "libdliom_hooks.so")  # -DDLIOM_TEST_HOOKS build (tests only)

KERNEL_RTCSM_SCORE, KERNEL_RTCSM_SELECT, KERNEL_RTCSM_RESCORE, KERNEL_CSM_EVAL, KERNEL_INSERT, KERNEL_ALLREDUCE = range(6)

_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p


class RtcsmOptions(C.Structure):
    _fields_ = [("linear_search_window", C.c_double), ("angular_search_window", C.c_double),
                ("translation_delta_cost_weight", C.c_double), ("rotation_delta_cost_weight", C.c_double)]


class RtcsmWindow(C.Structure):
    _fields_ = [("linear_window_size", C.c_int), ("angular_window_size", C.c_int),
                ("angular_step_size", C.c_float), ("max_scan_range", C.c_float),
                ("num_translations", C.c_int64), ("num_rotations", C.c_int64),
                ("num_candidates", C.c_int64)]


class RtcsmStats(C.Structure):
    _fields_ = [("window", RtcsmWindow), ("num_points", C.c_int64), ("num_rescored", C.c_int64),
                ("best_index", C.c_int64), ("score_kernel", C.c_int64), ("box_kernel_status", C.c_int64),
                ("box_kernel_variant", C.c_int64)]


BOX_RAN, BOX_NOT_REQUESTED, BOX_REFUSED_SMALL, BOX_REFUSED_NO_MIRROR = 0, 1, 2, 3
BOX_REFUSED_RANGE, BOX_REFUSED_WINDOW, BOX_REFUSED_LDS, BOX_REFUSED_FLAGGED = 4, 5, 6, 7


MAX_CLOUDS = 8


class CsmOptions(C.Structure):
    _fields_ = [("num_occupied_space_weights", C.c_int), ("occupied_space_weight", C.c_double * MAX_CLOUDS),
                ("translation_weight", C.c_double), ("rotation_weight", C.c_double),
                ("only_optimize_yaw", C.c_int), ("use_nonmonotonic_steps", C.c_int),
                ("max_num_iterations", C.c_int), ("num_threads", C.c_int)]


class CsmSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("num_iterations", C.c_int), ("num_residual_evaluations", C.c_int),
                ("num_jacobian_evaluations", C.c_int), ("termination_type", C.c_int)]


class AdaptiveVoxelFilterOptions(C.Structure):
    _fields_ = [("max_length", C.c_float), ("min_num_points", C.c_float), ("max_range", C.c_float)]


class FrontEndOptions(C.Structure):
    _fields_ = [("high_resolution_adaptive_voxel_filter", AdaptiveVoxelFilterOptions),
                ("low_resolution_adaptive_voxel_filter", AdaptiveVoxelFilterOptions),
                ("use_online_correlative_scan_matching", C.c_int),
                ("real_time_correlative_scan_matcher", RtcsmOptions),
                ("ceres_scan_matcher", CsmOptions),
                ("motion_filter_max_time_seconds", C.c_double),
                ("motion_filter_max_distance_meters", C.c_double),
                ("motion_filter_max_angle_radians", C.c_double),
                ("high_resolution", C.c_double), ("high_resolution_max_range", C.c_double),
                ("low_resolution", C.c_double), ("num_range_data", C.c_int),
                ("hit_probability", C.c_double), ("miss_probability", C.c_double),
                ("num_free_space_voxels", C.c_int)]


class FastCsmOptions(C.Structure):
    _fields_ = [("branch_and_bound_depth", C.c_int), ("full_resolution_depth", C.c_int),
                ("min_rotational_score", C.c_double), ("min_low_resolution_score", C.c_double),
                ("linear_xy_search_window", C.c_double), ("linear_z_search_window", C.c_double),
                ("angular_search_window", C.c_double)]


class FastCsmNodeData(C.Structure):
    _fields_ = [("gravity_alignment", C.c_double * 4), ("high_resolution_points", C.POINTER(C.c_float)),
                ("num_high_resolution_points", C.c_int64), ("low_resolution_points", C.POINTER(C.c_float)),
                ("num_low_resolution_points", C.c_int64),
                ("rotational_scan_matcher_histogram", C.POINTER(C.c_float))]


class FastCsmResult(C.Structure):
    _fields_ = [("found", C.c_int), ("score", C.c_float), ("pose_estimate", C.c_double * 7),
                ("rotational_score", C.c_float), ("low_resolution_score", C.c_float), ("num_discrete_scans", C.c_int),
                ("num_scored_candidates", C.c_int64), ("num_score_launches", C.c_int64)]


class BatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("batched", "per_query", "per_query_frontier", "per_query_one_launch",
                                         "without_search", "chunks", "frontier_chains", "lm_launches", "cache_misses",
                                         "synchronizations", "read_backs")]


FAST_CSM_MATCH, FAST_CSM_MATCH_FULL_SUBMAP, FAST_CSM_MATCH_WITH_3DOF_INITIAL = 0, 1, 2
_FAST_CSM_KINDS = {"Match": FAST_CSM_MATCH, "MatchFullSubmap": FAST_CSM_MATCH_FULL_SUBMAP,
                   "MatchWith3DofInitial": FAST_CSM_MATCH_WITH_3DOF_INITIAL}


class FastCsmQuery(C.Structure):
    _fields_ = [("kind", C.c_int), ("matcher", _vp), ("pose", C.c_double * 7), ("submap_pose", C.c_double * 7),
                ("node_data", FastCsmNodeData), ("histogram_size", C.c_int), ("min_score", C.c_float)]


class CsmProblem(C.Structure):
    _fields_ = [("target_translation", C.c_double * 3), ("initial_pose_estimate", C.c_double * 7),
                ("num_clouds", C.c_int), ("points_xyz", _f32p * MAX_CLOUDS), ("n", C.c_int64 * MAX_CLOUDS),
                ("clouds", _vp * MAX_CLOUDS), ("grids", _vp * MAX_CLOUDS)]


class ImuNoise(C.Structure):
    _fields_ = [("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint64), C.c_void_p)


class ImuWindowOptions(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "acc_noise", "gyr_noise", "acc_bias_noise", "gyr_bias_noise", "gravity", "integration_sigma", "prior_pose_noise",
        "prior_velocity_sigma", "prior_bias_sigma", "ceres_pose_noise_t", "ceres_pose_noise_r", "ceres_pose_noise_t_drift",
        "ceres_pose_noise_r_drift", "prior_gravity_noise")] + [
            ("window_size", C.c_int), ("iterations", C.c_int), ("enable_gravity_factor", C.c_int),
            ("frames_for_online_gravity_estimate", C.c_int), ("lidar_in_imu_translation", C.c_double * 3),
            ("graph_reset_every", C.c_int), ("tangent_preintegration", C.c_int), ("relinearize_threshold", C.c_double)]


class ImuPreintegration(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4),
                ("delta_v", C.c_double * 3), ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
                ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225)]


class MatchResult(C.Structure):
    _fields_ = [("dropped", C.c_int), ("pose_estimate", C.c_double * 7),
                ("pose_observation_in_submap", C.c_double * 7), ("initial_ceres_pose", C.c_double * 7),
                ("rtcsm_score", C.c_float), ("summary", CsmSummary), ("residual_distance", C.c_double),
                ("residual_angle", C.c_double), ("num_high_resolution_points", C.c_int64),
                ("num_low_resolution_points", C.c_int64), ("matching_submap_index", C.c_int)]


class MemoryStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("grids", "leaf_table_bytes", "leaf_pool_bytes", "mirror_bytes", "mirror_budget_bytes",
                                         "mirrors_refused", "scratch_bytes", "leaf_capacity", "leaf_slots_upper_bound")] + [
                                             ("mirror_windowed", C.c_int), ("outlier_table_bytes", C.c_int64),
                                             ("probability_grid_bytes", C.c_int64), ("points_xray_bytes", C.c_int64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class OutlierStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("voxels", "leaves", "leaf_capacity", "table_capacity", "table_bytes", "growths",
                                         "samples_walked", "probes")] + [("phase", C.c_int)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PointsXrayStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("voxels", "columns", "leaves", "table_bytes", "probes", "longest_segment", "growths",
                                         "inserts", "points")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FixedRatioSamplerStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("chunks", "repaired_chunks", "repair_passes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ProbabilityGridStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("bytes", "growths", "inserts", "cells_visited")] + [("known_box", C.c_int32 * 4),
                                                                                             ("error_word", C.c_int32)]


class InsertionResult(C.Structure):
    _fields_ = [("inserted", C.c_int), ("num_insertion_submaps", C.c_int), ("insertion_submap_index", C.c_int * 2),
                ("submap_added", C.c_int), ("submap_finished", C.c_int)]


# Every symbol include/dliom.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("dliom_status_string", C.c_char_p, [C.c_int]),
    ("dliom_last_error", C.c_char_p, []),
    ("dliom_device_count", C.c_int, []),
    ("dliom_ctx_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("dliom_ctx_create_on_stream", C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    ("dliom_ctx_destroy", C.c_int, [_vp]),
    ("dliom_ctx_synchronize", C.c_int, [_vp]),
    ("dliom_compute_lookup_table_to_apply_odds", C.c_int, [C.c_float, _u16p]),
    ("dliom_odds", C.c_float, [C.c_float]),
    ("dliom_probability_to_value", C.c_uint16, [C.c_float]),
    ("dliom_grid_set_values", C.c_int, [_vp, _i32p, _u16p, C.c_int64]),
    ("dliom_value_to_probability_table", C.c_int, [_f32p]),
    ("dliom_grid_create", C.c_int, [_vp, C.c_float, C.POINTER(_vp)]),
    ("dliom_grid_destroy", C.c_int, [_vp]),
    ("dliom_grid_resolution", C.c_int, [_vp, _f32p]),
    ("dliom_grid_bits", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_grid_mirror_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    ("dliom_ctx_memory_stats", C.c_int, [_vp, C.POINTER(MemoryStats)]),
    ("dliom_ctx_set_mirror_budget", C.c_int, [_vp, C.c_int64]),
    ("dliom_grid_memory_stats", C.c_int, [_vp, C.POINTER(MemoryStats)]),
    ("dliom_imu_window_solver_stats", C.c_int, [_vp, _i64p, _i64p]),
    ("dliom_imu_window_window_optimize", C.c_int, [_vp, _f64p, C.c_int, _f64p, _f64p, _f64p]),
    ("dliom_grid_upload_blocks", C.c_int, [_vp, _i32p, _u16p, C.c_int64]),
    ("dliom_grid_num_blocks", C.c_int, [_vp, _i64p]),
    ("dliom_grid_download_blocks", C.c_int, [_vp, _i32p, _u16p, C.c_int64, _i64p]),
    ("dliom_grid_get_values", C.c_int, [_vp, _i32p, C.c_int64, _u16p]),
    ("dliom_grid_xray_texture", C.c_int, [_vp, _f64p, C.POINTER(C.c_uint8), C.c_int64, _i32p, _i32p, _f64p, _f64p]),
    ("dliom_grid_project_to_image", C.c_int, [_vp, _f64p, C.POINTER(C.c_uint8), C.c_int64, _i32p, _i32p, _f64p, _f64p,
                                              _f64p]),
    ("dliom_probability_to_log_odds_integer", C.c_uint8, [C.c_float]),
    ("dliom_grid_to_proto", C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_int64, _i64p]),
    ("dliom_grid_from_proto", C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(_vp)]),
    ("dliom_submap3d_to_proto", C.c_int, [_f64p, C.c_int32, C.c_int, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_uint8),
                                          C.c_int64, C.c_int, C.POINTER(C.c_uint8), C.c_int64, _i64p]),
    ("dliom_submap3d_from_proto", C.c_int, [C.POINTER(C.c_uint8), C.c_int64, C.c_int, _f64p, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int), _i64p, _i64p, _i64p, _i64p]),
    ("dliom_grid_insert", C.c_int, [_vp, _f32p, _f32p, C.c_int64, _u16p, _u16p, C.c_int]),
    ("dliom_inserter_create", C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.POINTER(_vp)]),
    ("dliom_inserter_destroy", C.c_int, [_vp]),
    ("dliom_inserter_tables", C.c_int, [_vp, _u16p, _u16p]),
    ("dliom_inserter_insert", C.c_int, [_vp, _vp, _f32p, _f32p, C.c_int64]),
    ("dliom_inserter_insert_cloud", C.c_int, [_vp, _vp, _f32p, C.c_int, _f32p, _vp, C.c_float]),
    ("dliom_inserter_insert_cloud_multi", C.c_int, [_vp, C.c_int, C.POINTER(_vp), _f32p, C.POINTER(C.c_int), _f32p, _vp, _f32p]),
    ("dliom_cloud_create", C.c_int, [_vp, _f32p, C.c_int64, C.POINTER(_vp)]),
    ("dliom_cloud_destroy", C.c_int, [_vp]),
    ("dliom_cloud_size", C.c_int, [_vp, _i64p]),
    ("dliom_cloud_bounds", C.c_int, [_vp, _f32p, _f32p]),
    ("dliom_cloud_voxel_filter", C.c_int, [_vp, _vp, C.c_float, C.POINTER(_vp)]),
    ("dliom_cloud_adaptive_voxel_filter", C.c_int, [_vp, _vp, C.POINTER(AdaptiveVoxelFilterOptions), C.POINTER(_vp)]),
    ("dliom_cloud_adaptive_voxel_filter_pair", C.c_int, [_vp, _vp, C.POINTER(AdaptiveVoxelFilterOptions),
                                                         C.POINTER(AdaptiveVoxelFilterOptions), C.POINTER(_vp), C.POINTER(_vp)]),
    ("dliom_cloud_download", C.c_int, [_vp, _f32p]),
    ("dliom_cloud_download_transformed", C.c_int, [_vp, _f32p, _f32p]),
    ("dliom_outlier_remover_create", C.c_int, [_vp, C.c_double, C.POINTER(_vp)]),
    ("dliom_outlier_remover_destroy", C.c_int, [_vp]),
    ("dliom_outlier_remover_mark_hits", C.c_int, [_vp, _vp]),
    ("dliom_outlier_remover_count_rays", C.c_int, [_vp, _f32p, _vp]),
    ("dliom_outlier_remover_filter", C.c_int, [_vp, _vp, C.POINTER(_vp), _i32p, C.c_int64, _i64p]),
    ("dliom_outlier_remover_voxels", C.c_int, [_vp, _i32p, _i32p, _i32p, C.c_int64, _i64p]),
    ("dliom_outlier_remover_stats", C.c_int, [_vp, C.POINTER(OutlierStats)]),
    ("dliom_points_xray_create", C.c_int, [_vp, C.c_double, _f32p, C.POINTER(_vp)]),
    ("dliom_points_xray_destroy", C.c_int, [_vp]),
    ("dliom_points_xray_insert", C.c_int, [_vp, _vp, _f32p, C.c_int64]),
    ("dliom_points_xray_bounding_box", C.c_int, [_vp, _i32p, _i32p, C.POINTER(C.c_int)]),
    ("dliom_points_xray_columns", C.c_int, [_vp, _i32p, _f32p, _u32p, _u32p, C.c_int64, _i64p]),
    ("dliom_points_xray_voxels", C.c_int, [_vp, _i32p, C.c_int64, _i64p]),
    ("dliom_points_xray_draw", C.c_int, [_vp, _i32p, _i32p, _u32p, C.c_int64, _i32p, _i32p]),
    ("dliom_points_xray_stats", C.c_int, [_vp, C.POINTER(PointsXrayStats)]),
    ("dliom_points_xray_pixel", C.c_int, [C.c_uint32, C.c_uint32, _f32p, _u32p]),
    ("dliom_trajectory_create", C.c_int, [_vp, _i64p, _f64p, C.c_int64, C.POINTER(_vp)]),
    ("dliom_trajectory_destroy", C.c_int, [_vp]),
    ("dliom_trajectory_size", C.c_int, [_vp, _i64p]),
    ("dliom_trajectory_lookup", C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int), _f64p]),
    ("dliom_cloud_from_sensor_points", C.c_int, [_vp, _vp, C.c_int64, _f32p, C.c_int64, _f64p, C.POINTER(_vp), _f32p, _i32p,
                                                 C.c_int64, _i64p]),
    ("dliom_assemble_check_stats", C.c_int, [_vp, _i64p, _i64p, _i64p, _i64p]),
    ("dliom_cloud_min_max_range_filter", C.c_int, [_vp, _vp, _f32p, C.c_double, C.c_double, C.POINTER(_vp), _i32p, C.c_int64,
                                                   _i64p]),
    ("dliom_points_batch_create", C.c_int, [_vp, _f32p, C.c_int64, _f32p, _f32p, _f32p, C.c_int64, C.POINTER(_vp)]),
    ("dliom_points_batch_destroy", C.c_int, [_vp]),
    ("dliom_points_batch_size", C.c_int, [_vp, _i64p]),
    ("dliom_points_batch_has_intensities", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_points_batch_has_colors", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_points_batch_cloud", C.c_int, [_vp, C.POINTER(_vp)]),
    ("dliom_points_batch_origin", C.c_int, [_vp, _f32p]),
    ("dliom_points_batch_download", C.c_int, [_vp, _f32p, _f32p, _f32p]),
    ("dliom_points_batch_from_sensor_points", C.c_int, [_vp, _vp, C.c_int64, _f32p, _f32p, C.c_int64, _f64p, C.POINTER(_vp)]),
    ("dliom_points_batch_min_max_range_filter", C.c_int, [_vp, C.c_double, C.c_double]),
    ("dliom_outlier_remover_filter_batch", C.c_int, [_vp, _vp]),
    ("dliom_points_batch_color", C.c_int, [_vp, _f32p]),
    ("dliom_points_batch_intensity_to_color", C.c_int, [_vp, C.c_float, C.c_float]),
    ("dliom_points_xray_insert_batch", C.c_int, [_vp, _vp]),
    ("dliom_fixed_ratio_sampler_create", C.c_int, [C.c_double, C.POINTER(_vp)]),
    ("dliom_fixed_ratio_sampler_destroy", C.c_int, [_vp]),
    ("dliom_fixed_ratio_sampler_reset", C.c_int, [_vp]),
    ("dliom_fixed_ratio_sampler_state", C.c_int, [_vp, _i64p, _i64p]),
    ("dliom_fixed_ratio_sampler_stats", C.c_int, [_vp, C.POINTER(FixedRatioSamplerStats)]),
    ("dliom_points_batch_fixed_ratio_sample", C.c_int, [_vp, _vp]),
    ("dliom_points_batch_pack", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int64, _i64p]),
    ("dliom_ply_header", C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_char_p, C.c_int64, _i64p]),
    ("dliom_pcd_header", C.c_int, [C.c_int, C.c_int64, C.c_char_p, C.c_int64, _i64p]),
    ("dliom_rtcsm3d_match", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _f32p, C.c_int64, _vp, _f64p, _f32p]),
    ("dliom_rtcsm3d_match_cloud", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _vp, _vp, _f64p, _f32p]),
    ("dliom_rtcsm3d_shard_begin", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _vp, _vp, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint32)]),
    ("dliom_rtcsm3d_shard_finish", C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("dliom_rtcsm3d_shard_decode", C.c_int, [_vp, C.c_uint64, _f64p, _f32p]),
    ("dliom_rtcsm3d_window", C.c_int, [C.POINTER(RtcsmOptions), C.c_float, _f32p, C.c_int64, C.POINTER(RtcsmWindow)]),
    ("dliom_rtcsm3d_last_stats", C.c_int, [_vp, C.POINTER(RtcsmStats)]),
    ("dliom_rtcsm3d_box_error", C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    ("dliom_rtcsm3d_match_sharded", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _vp, _vp, C.c_int, C.c_int, EXCHANGE_FN,
                                              _vp, _f64p, C.POINTER(C.c_float)]),
    ("dliom_rtcsm3d_match_sharded_rccl", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _vp, _vp, _vp, _f64p,
                                                   C.POINTER(C.c_float)]),
    ("dliom_csm3d_match", C.c_int, [_vp, C.POINTER(CsmOptions), _f64p, _f64p, C.c_int, C.POINTER(_f32p), _i64p,
                                    C.POINTER(_vp), _f64p, C.POINTER(CsmSummary)]),
    ("dliom_csm3d_match_cloud", C.c_int, [_vp, C.POINTER(CsmOptions), _f64p, _f64p, C.c_int, C.POINTER(_vp),
                                          C.POINTER(_vp), _f64p, C.POINTER(CsmSummary)]),
    ("dliom_front_end_create", C.c_int, [_vp, C.POINTER(FrontEndOptions), C.POINTER(_vp)]),
    ("dliom_front_end_destroy", C.c_int, [_vp]),
    ("dliom_front_end_match", C.c_int, [_vp, _f64p, _f32p, _f32p, C.c_int64, C.POINTER(MatchResult)]),
    ("dliom_front_end_match_cloud", C.c_int, [_vp, _f64p, _f32p, _vp, C.POINTER(MatchResult)]),
    ("dliom_front_end_insert", C.c_int, [_vp, C.c_int64, _f64p, _f64p, C.POINTER(InsertionResult)]),
    ("dliom_front_end_num_active_submaps", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_front_end_insert_range_data", C.c_int, [_vp, _f32p, _vp, _f64p, C.POINTER(InsertionResult)]),
    ("dliom_front_end_num_finished_submaps", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_front_end_take_finished_submap", C.c_int, [_vp, _f64p, C.POINTER(C.c_int), C.POINTER(_vp), C.POINTER(_vp)]),
    ("dliom_front_end_matching_index", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_front_end_matched_clouds", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("dliom_front_end_active_submap", C.c_int, [_vp, C.c_int, _f64p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                C.POINTER(_vp), C.POINTER(_vp)]),
    ("dliom_voxel_filter", C.c_int, [C.c_float, _f32p, C.c_int64, _f32p, _i64p]),
    ("dliom_adaptive_voxel_filter", C.c_int, [C.POINTER(AdaptiveVoxelFilterOptions), _f32p, C.c_int64, _f32p, _i64p]),
    ("dliom_deskew", C.c_int, [_vp, _f64p, _f64p, C.c_double, _f32p, C.c_int64, _f32p, C.c_float, C.c_float, _f32p,
                               C.POINTER(C.c_uint8), _f32p]),
    ("dliom_add_range_data", C.c_int, [_vp, _f64p, _f64p, C.c_double, _f32p, C.c_int64, _f32p, C.c_float, C.c_float,
                                       C.c_float, C.POINTER(_vp), _f32p, _f32p]),
    ("dliom_fast_csm_create", C.c_int, [_vp, _vp, _vp, _f32p, _f32p, C.c_int, C.c_int, C.POINTER(FastCsmOptions),
                                        C.POINTER(_vp)]),
    ("dliom_fast_csm_destroy", C.c_int, [_vp]),
    ("dliom_ctx_device", C.c_int, [_vp]),
    ("dliom_fast_csm_match", C.c_int, [_vp, _vp, _f64p, _f64p, C.POINTER(FastCsmNodeData), C.c_float,
                                       C.POINTER(FastCsmResult)]),
    ("dliom_fast_csm_match_full_submap", C.c_int, [_vp, _vp, _f64p, _f64p, C.POINTER(FastCsmNodeData), C.c_float,
                                                   C.POINTER(FastCsmResult)]),
    ("dliom_fast_csm_match_with_3dof_initial", C.c_int, [_vp, _vp, _f64p, C.POINTER(FastCsmNodeData), C.c_float,
                                                         C.POINTER(FastCsmResult)]),
    ("dliom_fast_csm_level", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.POINTER(C.c_uint8), C.c_int64]),
    ("dliom_fast_csm_match_batch", C.c_int, [_vp, C.POINTER(FastCsmQuery), C.c_int, C.POINTER(FastCsmResult),
                                             C.POINTER(C.c_int), C.POINTER(BatchStats)]),
    ("dliom_csm3d_match_batch", C.c_int, [_vp, C.POINTER(CsmOptions), C.c_int, C.POINTER(CsmProblem), _f64p,
                                          C.POINTER(CsmSummary), C.POINTER(C.c_int), C.POINTER(BatchStats)]),
    ("dliom_ctx_synchronizations", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("dliom_range_accumulator_create", C.c_int, [_vp, C.POINTER(_vp)]),
    ("dliom_range_accumulator_destroy", C.c_int, [_vp]),
    ("dliom_range_accumulator_add", C.c_int, [_vp, _f64p, _f64p, C.c_double, _f32p, _f32p, C.c_int64, _f32p, C.c_int,
                                              C.c_float, C.c_float, C.c_float, _f32p, C.POINTER(C.c_int)]),
    ("dliom_range_accumulator_finish", C.c_int, [_vp, C.c_float, C.POINTER(_vp), _f32p]),
    ("dliom_imu_window_default_options", C.c_int, [C.POINTER(ImuWindowOptions)]),
    ("dliom_imu_window_create", C.c_int, [C.POINTER(ImuWindowOptions), C.POINTER(_vp)]),
    ("dliom_imu_window_destroy", C.c_int, [_vp]),
    ("dliom_imu_window_initialize", C.c_int, [_vp, _f64p, _f64p, _f64p]),
    ("dliom_imu_window_add_imu", C.c_int, [_vp, _f64p, _f64p, C.c_double]),
    ("dliom_imu_window_predict", C.c_int, [_vp, _f64p, _f64p]),
    ("dliom_imu_window_add_gravity", C.c_int, [_vp, C.c_int, _f64p]),
    ("dliom_imu_window_add_pose", C.c_int, [_vp, _f64p, C.c_int, _f64p, _f64p, _f64p]),
    ("dliom_imu_window_state", C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p]),
    ("dliom_imu_window_size", C.c_int, [_vp]),
    ("dliom_diag_imu_factor_jacobians", C.c_int, [_vp, _f64p, _f64p]),
    ("dliom_imu_window_add_imu_batch", C.c_int, [_vp, C.c_int, _f64p, _f64p, _f64p]),
    ("dliom_imu_window_gravity_estimate", C.c_int, [_vp, _f64p, C.POINTER(C.c_int), _i64p]),
    ("dliom_gravity_estimate", C.c_int, [C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, C.c_double, _f64p, C.POINTER(C.c_int)]),
    ("dliom_imu_integrator_create", C.c_int, [_f64p, _f64p, C.POINTER(ImuNoise), C.POINTER(_vp)]),
    ("dliom_imu_integrator_destroy", C.c_int, [_vp]),
    ("dliom_imu_integrator_reset", C.c_int, [_vp, _f64p, _f64p, C.POINTER(ImuNoise)]),
    ("dliom_imu_integrator_push_back", C.c_int, [_vp, C.c_double, _f64p, _f64p]),
    ("dliom_imu_integrator_repropagate", C.c_int, [_vp, _f64p, _f64p]),
    ("dliom_imu_integrator_get", C.c_int, [_vp, C.POINTER(ImuPreintegration)]),
    ("dliom_imu_integrator_evaluate", C.c_int, [_vp, _f64p, _f64p, _f64p, _f64p]),
    ("dliom_imu_integrator_predict", C.c_int, [_vp, _f64p, _f64p, _f64p]),
    ("dliom_rotational_histogram", C.c_int, [_f32p, C.c_int64, C.c_int, _f32p]),
    ("dliom_rotational_histogram_mt", C.c_int, [_f32p, C.c_int64, C.c_int, C.c_int, _f32p]),
    ("dliom_cloud_rotational_histogram", C.c_int, [_vp, _vp, _f32p, C.c_int, _f32p]),
    ("dliom_cloud_rotational_histogram_begin", C.c_int, [_vp, _vp, _f32p, C.c_int]),
    ("dliom_cloud_rotational_histogram_finish", C.c_int, [_vp, _f32p]),
    ("dliom_diag_std_sort_order", C.c_int, [_vp, _f32p, C.c_int, C.POINTER(C.c_int32)]),
    ("dliom_diag_sequential_sums", C.c_int, [_vp, _f32p, C.c_int, C.c_int, _f32p, _f32p]),
    ("dliom_diag_histogram_contributions", C.c_int, [_vp, _vp, _f32p, C.c_int, C.POINTER(C.c_int32), _f32p, C.c_int64,
                                                      C.POINTER(C.c_int64)]),
    ("dliom_rotational_scan_match", C.c_int, [_f32p, _f32p, C.c_int, C.c_int, _f32p, C.c_float, _f32p, C.c_int, _f32p]),
    ("dliom_rtcsm2d_match", C.c_int, [C.POINTER(RtcsmOptions), _f64p, _f32p, C.c_int64, _u16p, C.c_int, C.c_int,
                                      C.c_double, C.c_double, C.c_double, _f64p, _f64p]),
    ("dliom_probe_transform_cell_indices", C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_float, _i32p]),
    ("dliom_rtcsm3d_score_volume", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _f32p, C.c_int64, _vp, _u64p,
                                             C.c_int64, _i64p]),
    ("dliom_rtcsm3d_sequential_sums", C.c_int, [_vp, C.POINTER(RtcsmOptions), _f64p, _f32p, C.c_int64, _vp, _i64p,
                                                C.c_int64, C.c_int, _f32p]),
    ("dliom_csm3d_evaluate", C.c_int, [_vp, C.POINTER(CsmOptions), _f64p, _f64p, _f64p, C.c_int, C.POINTER(_f32p),
                                       _i64p, C.POINTER(_vp), _f64p, _f64p, _f64p]),
    ("dliom_probability_grid_create", C.c_int, [_vp, C.c_double, C.c_int64, C.POINTER(_vp)]),
    ("dliom_probability_grid_create_with_limits", C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                            C.c_int64, C.POINTER(_vp)]),
    ("dliom_probability_grid_destroy", C.c_int, [_vp]),
    ("dliom_probability_grid_limits", C.c_int, [_vp, _f64p, _f64p, _i32p]),
    ("dliom_probability_grid_memory_stats", C.c_int, [_vp, C.POINTER(MemoryStats)]),
    ("dliom_probability_grid_get_stats", C.c_int, [_vp, C.POINTER(ProbabilityGridStats)]),
    ("dliom_probability_grid_grow_limits", C.c_int, [C.c_double, _f64p, _i32p, C.c_float, C.c_float, C.c_int64, _i32p,
                                                     C.POINTER(C.c_int32)]),
    ("dliom_compute_lookup_table_to_apply_correspondence_cost_odds", C.c_int, [C.c_float, _u16p]),
    ("dliom_inserter2d_create", C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.POINTER(_vp)]),
    ("dliom_inserter2d_destroy", C.c_int, [_vp]),
    ("dliom_inserter2d_tables", C.c_int, [_vp, _u16p, _u16p]),
    ("dliom_inserter2d_insert_cloud", C.c_int, [_vp, _vp, _f32p, _vp]),
    ("dliom_inserter2d_insert", C.c_int, [_vp, _vp, _f32p, _f32p, C.c_int64]),
    ("dliom_probability_grid_cells", C.c_int, [_vp, _u16p, C.c_int64, _i32p, _i32p, C.c_int]),
    ("dliom_probability_grid_get_probabilities", C.c_int, [_vp, _i32p, C.c_int64, _f32p, C.POINTER(C.c_uint8)]),
    ("dliom_probability_grid_draw", C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_int64, _i32p, _i32p, C.c_int]),
    ("dliom_probability_grid_color_table", C.c_int, [C.POINTER(C.c_uint8)]),
    ("dliom_ros_map_yaml_origin", C.c_int, [C.c_double, _f64p, _i32p, C.c_int32, C.c_int32, _f64p]),
    ("dliom_ros_map_pgm_header", C.c_int, [C.c_double, C.c_int32, C.c_int32, C.c_char_p, C.c_int64, _i64p]),
    ("dliom_ros_map_yaml", C.c_int, [C.c_double, _f64p, C.c_char_p, C.c_char_p, C.c_int64, _i64p]),
    ("dliom_ctx_set_tuning", C.c_int, [_vp, C.c_int, C.c_int]),
    ("dliom_ctx_poll_fallbacks", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("dliom_ctx_read_backs", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("dliom_ctx_voxel_filter_reruns", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("dliom_host_register", C.c_int, [_vp, _vp, C.c_size_t]),
    ("dliom_host_unregister", C.c_int, [_vp, _vp]),
    ("dliom_ctx_get_tuning", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("dliom_deskew_check_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("dliom_ctx_set_profiling", C.c_int, [_vp, C.c_int]),
    ("dliom_ctx_reset_profiling", C.c_int, [_vp]),
    ("dliom_ctx_kernel_time", C.c_int, [_vp, C.c_int, _f64p, _i64p]),
]

_lib = None


def load_library(path=None):
    """Loads libdliom.so and binds every symbol of include/dliom.h (AttributeError if one is
    missing).  Loading needs the HIP runtime but no GPU."""
    global _lib
    if _lib is None:
        p = path or os.environ.get("DLIOM_LIB") or LIB_PATH  # DLIOM_LIB: A/B builds of the library (tools/)
        if not os.path.exists(p):
            raise DliomError(ERR_NO_DEVICE, "libdliom.so not built at %s (run __graft_entry__.build())" % p)
        lib = C.CDLL(p)
        for name, res, args in SYMBOLS:
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib


def _check(status, where):
    if status != OK:
        raise DliomError(status, where)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return a.ctypes.data_as(t)


def device_count():
    return load_library().dliom_device_count()


def compute_lookup_table_to_apply_odds(odds):
    """mapping/probability_values.cc:73-83"""
    out = np.zeros(32768, dtype=np.uint16)
    _check(load_library().dliom_compute_lookup_table_to_apply_odds(C.c_float(odds), _p(out, _u16p)), "lookup table")
    return out


def odds(p):
    return load_library().dliom_odds(C.c_float(p))


def value_to_probability_table():
    out = np.zeros(65536, dtype=np.float32)
    _check(load_library().dliom_value_to_probability_table(_p(out, _f32p)), "value table")
    return out


class Context:
    """One HIP stream + scratch memory (dliom_ctx)."""

    def __init__(self, device_id=0, stream=None):
        L = load_library()
        self._L = L
        h = _vp()
        if stream is None:
            _check(L.dliom_ctx_create(device_id, C.byref(h)), "dliom_ctx_create")
        else:
            _check(L.dliom_ctx_create_on_stream(device_id, _vp(stream), C.byref(h)), "dliom_ctx_create_on_stream")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self._L.dliom_ctx_synchronize(self.h), "synchronize")

    def voxel_filter_reruns(self):
        """dliom_ctx_voxel_filter_reruns: voxel filter launches repeated with 21-bit keys (a point beyond 4095 edges)."""
        n = C.c_int64(0)
        _check(self._L.dliom_ctx_voxel_filter_reruns(self.h, C.byref(n)), "voxel_filter_reruns")
        return int(n.value)

    def memory_stats(self):
        """dliom_ctx_memory_stats: HBM held by this context's grids and scratch buffers; no sync."""
        m = MemoryStats()
        _check(self._L.dliom_ctx_memory_stats(self.h, C.byref(m)), "ctx_memory_stats")
        return m.as_dict()

    def set_mirror_budget(self, num_bytes):
        """dliom_ctx_set_mirror_budget: cap on the sum of this context's dense mirrors (0 = none)."""
        _check(self._L.dliom_ctx_set_mirror_budget(self.h, int(num_bytes)), "ctx_set_mirror_budget")

    def host_register(self, array):
        """dliom_host_register: page-locks a numpy array the caller keeps (uploads from it become one asynchronous DMA)."""
        _check(self._L.dliom_host_register(self.h, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes)), "host_register")

    def host_unregister(self, array):
        _check(self._L.dliom_host_unregister(self.h, C.c_void_p(array.ctypes.data)), "host_unregister")

    def synchronizations(self):
        """dliom_ctx_synchronizations: stream synchronisations of the loop-closure paths on this context so far."""
        n = C.c_int64()
        _check(self._L.dliom_ctx_synchronizations(self.h, C.byref(n)), "synchronizations")
        return n.value

    def read_backs(self):
        """dliom_ctx_read_backs: polled host round trips on this context so far."""
        n = C.c_int64(0)
        _check(self._L.dliom_ctx_read_backs(self.h, C.byref(n)), "read_backs")
        return int(n.value)

    def poll_fallbacks(self):
        """dliom_ctx_poll_fallbacks: read-backs that ran out of polling time and synchronised the stream instead."""
        n = C.c_int64(0)
        _check(self._L.dliom_ctx_poll_fallbacks(self.h, C.byref(n)), "poll_fallbacks")
        return int(n.value)

    def set_tuning(self, knob, value):
        """dliom_ctx_set_tuning: TUNE_SCORE_KERNEL, TUNE_CSM_ONE_LAUNCH_MAX (knob 2 is reserved: refused by
        the shipped library, the fault injection of libdliom_hooks.so)."""
        _check(self._L.dliom_ctx_set_tuning(self.h, int(knob), int(value)), "set_tuning")

    def deskew_check_stats(self):
        """(records checked against glibc on the host, ring overflows, hits whose device cast differed and were redone)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._L.dliom_deskew_check_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "deskew_check_stats")
        return int(a.value), int(b.value), int(c.value)

    def assemble_check_stats(self):
        """dliom_assemble_check_stats: (points recorded by the batch assembler, records recomputed with glibc on the host,
        points whose device cast differed and were redone, calls whose records outgrew the ring)."""
        v = [C.c_int64() for _ in range(4)]
        _check(self._L.dliom_assemble_check_stats(self.h, *[C.byref(x) for x in v]), "assemble_check_stats")
        return tuple(int(x.value) for x in v)

    def get_tuning(self, knob):
        v = C.c_int(0)
        _check(self._L.dliom_ctx_get_tuning(self.h, int(knob), C.byref(v)), "get_tuning")
        return v.value

    def set_profiling(self, on):
        _check(self._L.dliom_ctx_set_profiling(self.h, int(on)), "set_profiling")

    def reset_profiling(self):
        _check(self._L.dliom_ctx_reset_profiling(self.h), "reset_profiling")

    def kernel_time(self, kernel_id):
        ms, n = C.c_double(), C.c_int64()
        _check(self._L.dliom_ctx_kernel_time(self.h, kernel_id, C.byref(ms), C.byref(n)), "kernel_time")
        return ms.value, n.value

    def probe_transform_cell_indices(self, pose7_f32, points, resolution):
        pose = _f32(pose7_f32)
        pts = _f32(points).reshape(-1, 3)
        out = np.zeros((len(pts), 3), dtype=np.int32)
        _check(self._L.dliom_probe_transform_cell_indices(self.h, _p(pose, _f32p), _p(pts, _f32p), len(pts),
                                                          C.c_float(resolution), _p(out, _i32p)), "probe cells")
        return out


def _cloud_bounds(lib, handle):
    max_norm, abs_max = C.c_float(), np.zeros(3, dtype=np.float32)
    _check(lib.dliom_cloud_bounds(handle, C.byref(max_norm), _p(abs_max, _f32p)), "dliom_cloud_bounds")
    return np.float32(max_norm.value), abs_max


class PointCloud:
    """sensor::PointCloud staged in HBM (dliom_cloud)."""

    def __init__(self, ctx, points=None, _handle=None):
        self._L = ctx._L
        self.ctx = ctx
        if _handle is not None:  # a cloud built on the device (filters)
            self.h = _handle
            n = C.c_int64()
            _check(self._L.dliom_cloud_size(self.h, C.byref(n)), "dliom_cloud_size")
            self.n = n.value
            return
        pts = _f32(points).reshape(-1, 3)
        self.n = len(pts)
        h = _vp()
        _check(self._L.dliom_cloud_create(ctx.h, _p(pts, _f32p), len(pts), C.byref(h)), "dliom_cloud_create")
        self.h = h

    def __len__(self):
        return self.n

    def voxel_filter(self, size):
        """sensor::VoxelFilter(size).Filter(cloud) on the device -> new PointCloud."""
        h = _vp()
        _check(self._L.dliom_cloud_voxel_filter(self.ctx.h, self.h, C.c_float(size), C.byref(h)), "dliom_cloud_voxel_filter")
        return PointCloud(self.ctx, _handle=h)

    def adaptive_voxel_filter(self, max_length, min_num_points, max_range):
        """sensor::AdaptiveVoxelFilter(options).Filter(cloud) on the device -> new PointCloud."""
        o = AdaptiveVoxelFilterOptions(max_length, min_num_points, max_range)
        h = _vp()
        _check(self._L.dliom_cloud_adaptive_voxel_filter(self.ctx.h, self.h, C.byref(o), C.byref(h)),
               "dliom_cloud_adaptive_voxel_filter")
        return PointCloud(self.ctx, _handle=h)

    def adaptive_voxel_filter_pair(self, first, second):
        """Two AdaptiveVoxelFilter option triples (max_length, min_num_points, max_range) searched together
        -> (PointCloud, PointCloud), each equal to adaptive_voxel_filter(*triple)."""
        a, b = AdaptiveVoxelFilterOptions(*first), AdaptiveVoxelFilterOptions(*second)
        ha, hb = _vp(), _vp()
        _check(self._L.dliom_cloud_adaptive_voxel_filter_pair(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(ha),
                                                              C.byref(hb)), "dliom_cloud_adaptive_voxel_filter_pair")
        return PointCloud(self.ctx, _handle=ha), PointCloud(self.ctx, _handle=hb)

    def min_max_range_filter(self, origin, min_range, max_range):
        """io::MinMaxRangeFiteringPointsProcessor on the device -> (PointCloud, int32 input indices of the survivors)."""
        h, kept = _vp(), C.c_int64()
        index = np.zeros(max(self.n, 1), dtype=np.int32)
        _check(self._L.dliom_cloud_min_max_range_filter(self.ctx.h, self.h, _p(_f32(origin), _f32p), float(min_range),
                                                        float(max_range), C.byref(h), _p(index, _i32p), self.n,
                                                        C.byref(kept)), "dliom_cloud_min_max_range_filter")
        return PointCloud(self.ctx, _handle=h), index[:kept.value].copy()

    def bounds(self):
        """dliom_cloud_bounds -> (max_norm np.float32, abs_max float32[3]; a negative component: unknown)."""
        return _cloud_bounds(self._L, self.h)

    def pack_xyz(self, capacity=None, fill=0):
        """PointsBatch.pack_xyz of the cloud's points (dliom_cloud_pack_xyz)."""
        return _pack_xyz(self._L.dliom_cloud_pack_xyz, self.h, capacity, fill)

    def download(self, pose7=None):
        """The points, packed xyz; pose7 (float [t, q]): sensor::TransformPointCloud(cloud, pose) applied on the device."""
        out = np.zeros((self.n, 3), dtype=np.float32)
        if pose7 is None:
            _check(self._L.dliom_cloud_download(self.h, _p(out, _f32p)), "dliom_cloud_download")
        else:
            _check(self._L.dliom_cloud_download_transformed(self.h, _p(_f32(pose7), _f32p), _p(out, _f32p)),
                   "dliom_cloud_download_transformed")
        return out

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_cloud_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trajectory:
    """transform::TransformInterpolationBuffer as an immutable array of nodes (dliom_trajectory): times in common::Time
    ticks (100 ns), poses [tx,ty,tz,qw,qx,qy,qz].  ctx None: a host-only buffer (has / lookup)."""

    def __init__(self, ctx, times, poses7):
        self._L = ctx._L if ctx is not None else load_library()
        self.ctx = ctx
        t = np.ascontiguousarray(times, dtype=np.int64).reshape(-1)
        p = _f64(poses7).reshape(-1, 7)
        if len(t) != len(p):
            raise ValueError("one pose per time")
        h = _vp()
        _check(self._L.dliom_trajectory_create(ctx.h if ctx is not None else None, _p(t, _i64p), _p(p, _f64p), len(t), C.byref(h)),
               "dliom_trajectory_create")
        self.h = h
        self.n = len(t)

    def __len__(self):
        return self.n

    def has(self, time):
        has = C.c_int()
        _check(self._L.dliom_trajectory_lookup(self.h, int(time), C.byref(has), None), "dliom_trajectory_lookup")
        return bool(has.value)

    def lookup(self, time):
        """Lookup(time) as float64[7], or None where not Has(time)."""
        has, pose = C.c_int(), np.zeros(7, dtype=np.float64)
        _check(self._L.dliom_trajectory_lookup(self.h, int(time), C.byref(has), _p(pose, _f64p)), "dliom_trajectory_lookup")
        return pose if has.value else None

    def assemble(self, cloud_time, points_xyzt, sensor_to_tracking, capacity=None):
        """HandleMessage's loop on the device (dliom_cloud_from_sensor_points) -> (PointCloud or None, float32 origin[3],
        int32 input indices of the kept points)."""
        pts = _f32(points_xyzt).reshape(-1, 4)
        h, kept, origin = _vp(), C.c_int64(), np.zeros(3, dtype=np.float32)
        cap = len(pts) if capacity is None else int(capacity)
        index = np.zeros(max(cap, 1), dtype=np.int32)
        _check(self._L.dliom_cloud_from_sensor_points(self.ctx.h, self.h, int(cloud_time), _p(pts, _f32p), len(pts),
                                                      _p(_f64(sensor_to_tracking), _f64p), C.byref(h), _p(origin, _f32p),
                                                      _p(index, _i32p), cap, C.byref(kept)), "dliom_cloud_from_sensor_points")
        if not h:
            return None, origin, index[:0].copy()
        return PointCloud(self.ctx, _handle=h), origin, index[:kept.value].copy()

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_trajectory_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OutlierRemover:
    """io::OutlierRemovingPointsProcessor's voxel table on the device (dliom_outlier_remover): mark_hits over every
    batch, then count_rays over every batch, then filter every batch."""

    def __init__(self, ctx, voxel_size):
        self._L = ctx._L
        self.ctx = ctx
        h = _vp()
        _check(self._L.dliom_outlier_remover_create(ctx.h, float(voxel_size), C.byref(h)), "dliom_outlier_remover_create")
        self.h = h

    def mark_hits(self, cloud):
        _check(self._L.dliom_outlier_remover_mark_hits(self.h, cloud.h), "dliom_outlier_remover_mark_hits")

    def count_rays(self, origin, cloud):
        _check(self._L.dliom_outlier_remover_count_rays(self.h, _p(_f32(origin), _f32p), cloud.h),
               "dliom_outlier_remover_count_rays")

    def filter(self, cloud):
        """-> (PointCloud of the points kept, int32 input indices of them)."""
        h, kept = _vp(), C.c_int64()
        index = np.zeros(max(cloud.n, 1), dtype=np.int32)
        _check(self._L.dliom_outlier_remover_filter(self.h, cloud.h, C.byref(h), _p(index, _i32p), cloud.n, C.byref(kept)),
               "dliom_outlier_remover_filter")
        return PointCloud(self.ctx, _handle=h), index[:kept.value].copy()

    def voxels(self):
        """Every voxel with hits > 0, sorted by (z, y, x) -> (xyz int32 (n, 3), hits int32, rays int32)."""
        n = C.c_int64()
        _check(self._L.dliom_outlier_remover_voxels(self.h, None, None, None, 0, C.byref(n)), "dliom_outlier_remover_voxels")
        xyz = np.zeros((n.value, 3), dtype=np.int32)
        hits, rays = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        if n.value > 0:
            _check(self._L.dliom_outlier_remover_voxels(self.h, _p(xyz, _i32p), _p(hits, _i32p), _p(rays, _i32p), n.value,
                                                        C.byref(n)), "dliom_outlier_remover_voxels")
        return xyz, hits, rays

    def stats(self):
        s = OutlierStats()
        _check(self._L.dliom_outlier_remover_stats(self.h, C.byref(s)), "dliom_outlier_remover_stats")
        return s.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_outlier_remover_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def points_xray_pixel(occupied, max_occupied, mean_rgb):
    """dliom_points_xray_pixel: one pixel of IntoImage on the host's libm (io::Image's 0xFFrrggbb)."""
    out = C.c_uint32()
    _check(load_library().dliom_points_xray_pixel(int(occupied), int(max_occupied), _p(_f32(mean_rgb), _f32p), C.byref(out)),
           "dliom_points_xray_pixel")
    return int(out.value)


class PointsXray:
    """One Aggregation of io::XRayPointsProcessor on the device (dliom_points_xray): occupied voxels and per-column colour
    sums, equal to the reference's bit for bit.  transform7 = [tx, ty, tz, qw, qx, qy, qz] (a Rigid3f)."""

    def __init__(self, ctx, voxel_size, transform7=(0, 0, 0, 1, 0, 0, 0)):
        self._L = ctx._L
        self.ctx = ctx
        h = _vp()
        _check(self._L.dliom_points_xray_create(ctx.h, float(voxel_size), _p(_f32(transform7), _f32p), C.byref(h)),
               "dliom_points_xray_create")
        self.h = h

    def insert(self, cloud, colors=None):
        """colors: None (the reference's default black), one (r, g, b) for the batch, or float32 (n, 3) per point."""
        if colors is None:
            _check(self._L.dliom_points_xray_insert(self.h, cloud.h, None, 0), "dliom_points_xray_insert")
            return
        c = _f32(colors).reshape(-1, 3)
        _check(self._L.dliom_points_xray_insert(self.h, cloud.h, _p(c, _f32p), len(c)), "dliom_points_xray_insert")

    def bounding_box(self):
        """-> (min int32[3], max int32[3]) of the cell indices inserted, or None while empty."""
        lo, hi, empty = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32), C.c_int()
        _check(self._L.dliom_points_xray_bounding_box(self.h, _p(lo, _i32p), _p(hi, _i32p), C.byref(empty)),
               "dliom_points_xray_bounding_box")
        return None if empty.value else (lo, hi)

    def columns(self):
        """column_data sorted by (y, z) -> (yz int32 (n, 2), sums float32 (n, 3), counts uint32, occupied voxels uint32)."""
        n = C.c_int64()
        _check(self._L.dliom_points_xray_columns(self.h, None, None, None, None, 0, C.byref(n)), "dliom_points_xray_columns")
        yz, sums = np.zeros((n.value, 2), dtype=np.int32), np.zeros((n.value, 3), dtype=np.float32)
        counts, occupied = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        if n.value > 0:
            _check(self._L.dliom_points_xray_columns(self.h, _p(yz, _i32p), _p(sums, _f32p), _p(counts, _u32p), _p(occupied, _u32p),
                                                     n.value, C.byref(n)), "dliom_points_xray_columns")
        return yz, sums, counts, occupied

    def voxels(self):
        """The occupied voxels sorted by (z, y, x) -> int32 (n, 3)."""
        n = C.c_int64()
        _check(self._L.dliom_points_xray_voxels(self.h, None, 0, C.byref(n)), "dliom_points_xray_voxels")
        xyz = np.zeros((n.value, 3), dtype=np.int32)
        if n.value > 0:
            _check(self._L.dliom_points_xray_voxels(self.h, _p(xyz, _i32p), n.value, C.byref(n)), "dliom_points_xray_voxels")
        return xyz

    def draw(self, box=None):
        """IntoImage in `box` ((min, max) of cell indices; None: the aggregator's own) -> uint32 (height, width) 0xFFrrggbb;
        (0, 0) for an empty box."""
        lo = hi = None
        if box is not None:
            lo, hi = np.ascontiguousarray(box[0], dtype=np.int32), np.ascontiguousarray(box[1], dtype=np.int32)
        args = (None, None) if box is None else (_p(lo, _i32p), _p(hi, _i32p))
        w, h = C.c_int32(), C.c_int32()
        _check(self._L.dliom_points_xray_draw(self.h, args[0], args[1], None, 0, C.byref(w), C.byref(h)), "dliom_points_xray_draw")
        image = np.zeros((h.value, w.value), dtype=np.uint32)
        if image.size > 0:
            _check(self._L.dliom_points_xray_draw(self.h, args[0], args[1], _p(image, _u32p), image.size, C.byref(w), C.byref(h)),
                   "dliom_points_xray_draw")
        return image

    def stats(self):
        s = PointsXrayStats()
        _check(self._L.dliom_points_xray_stats(self.h, C.byref(s)), "dliom_points_xray_stats")
        return s.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_points_xray_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PACK_PLY, PACK_PCD = 0, 1


class _BorrowedCloud:
    """The points of a PointsBatch as the stages that take a dliom_cloud see them (not owned: no close)."""

    def __init__(self, L, handle, n):
        self._L, self.h, self.n = L, handle, n

    def __len__(self):
        return self.n

    def bounds(self):
        return _cloud_bounds(self._L, self.h)


class PointsBatch:
    """io::PointsBatch in HBM (dliom_points_batch): map-frame points, the origin, and optionally one intensity and one
    colour a point.  The stages below rewrite it in place; nothing but counts comes back until download() or pack()."""

    def __init__(self, ctx, points=None, origin=(0, 0, 0), intensities=None, colors=None, _handle=None):
        self._L = ctx._L
        self.ctx = ctx
        if _handle is not None:
            self.h = _handle
            return
        pts = _f32(points).reshape(-1, 3)
        it = None if intensities is None else _f32(intensities).reshape(-1)
        col = None if colors is None else _f32(colors).reshape(-1, 3)
        if it is not None and len(it) != len(pts):
            raise DliomError(ERR_INVALID_ARGUMENT, "one intensity a point")
        h = _vp()
        _check(self._L.dliom_points_batch_create(ctx.h, _p(pts, _f32p), len(pts), _p(_f32(origin), _f32p),
                                                 None if it is None else _p(it, _f32p), None if col is None else _p(col, _f32p),
                                                 0 if col is None else len(col), C.byref(h)), "dliom_points_batch_create")
        self.h = h

    @classmethod
    def from_sensor_points(cls, trajectory, cloud_time, points_xyzt, sensor_to_tracking, intensities=None):
        """dliom_points_batch_from_sensor_points -> PointsBatch, or None when no point is kept."""
        pts = _f32(points_xyzt).reshape(-1, 4)
        it = None if intensities is None else _f32(intensities).reshape(-1)
        if it is not None and len(it) != len(pts):
            raise DliomError(ERR_INVALID_ARGUMENT, "one intensity a point")
        h = _vp()
        _check(trajectory._L.dliom_points_batch_from_sensor_points(
            trajectory.ctx.h, trajectory.h, int(cloud_time), _p(pts, _f32p), None if it is None else _p(it, _f32p), len(pts),
            _p(_f64(sensor_to_tracking), _f64p), C.byref(h)), "dliom_points_batch_from_sensor_points")
        return cls(trajectory.ctx, _handle=h) if h else None

    def __len__(self):
        n = C.c_int64()
        _check(self._L.dliom_points_batch_size(self.h, C.byref(n)), "dliom_points_batch_size")
        return int(n.value)

    @property
    def has_intensities(self):
        v = C.c_int()
        _check(self._L.dliom_points_batch_has_intensities(self.h, C.byref(v)), "dliom_points_batch_has_intensities")
        return bool(v.value)

    @property
    def has_colors(self):
        v = C.c_int()
        _check(self._L.dliom_points_batch_has_colors(self.h, C.byref(v)), "dliom_points_batch_has_colors")
        return bool(v.value)

    @property
    def origin(self):
        o = np.zeros(3, dtype=np.float32)
        _check(self._L.dliom_points_batch_origin(self.h, _p(o, _f32p)), "dliom_points_batch_origin")
        return o

    def cloud(self):
        """The points, borrowed, for OutlierRemover.mark_hits / count_rays and the inserters: valid until the next
        compacting call on this batch."""
        h = _vp()
        _check(self._L.dliom_points_batch_cloud(self.h, C.byref(h)), "dliom_points_batch_cloud")
        return _BorrowedCloud(self._L, h, len(self))

    def download(self):
        """-> (points float32 (n, 3), intensities float32 (n,) or None, colors float32 (n, 3) or None)"""
        n = len(self)
        pts = np.zeros((n, 3), dtype=np.float32)
        it = np.zeros(n, dtype=np.float32) if self.has_intensities else None
        col = np.zeros((n, 3), dtype=np.float32) if self.has_colors else None
        _check(self._L.dliom_points_batch_download(self.h, _p(pts, _f32p), None if it is None else _p(it, _f32p),
                                                   None if col is None else _p(col, _f32p)), "dliom_points_batch_download")
        return pts, it, col

    def min_max_range_filter(self, min_range, max_range):
        _check(self._L.dliom_points_batch_min_max_range_filter(self.h, float(min_range), float(max_range)),
               "dliom_points_batch_min_max_range_filter")

    def remove_outliers(self, remover):
        """Phase three of an OutlierRemover, in place."""
        _check(self._L.dliom_outlier_remover_filter_batch(remover.h, self.h), "dliom_outlier_remover_filter_batch")

    def fixed_ratio_sample(self, sampler):
        _check(self._L.dliom_points_batch_fixed_ratio_sample(sampler.h, self.h), "dliom_points_batch_fixed_ratio_sample")

    def color(self, rgb):
        _check(self._L.dliom_points_batch_color(self.h, _p(_f32(rgb), _f32p)), "dliom_points_batch_color")

    def intensity_to_color(self, min_intensity, max_intensity):
        _check(self._L.dliom_points_batch_intensity_to_color(self.h, C.c_float(min_intensity), C.c_float(max_intensity)),
               "dliom_points_batch_intensity_to_color")

    def xray_insert(self, xray):
        _check(self._L.dliom_points_xray_insert_batch(xray.h, self.h), "dliom_points_xray_insert_batch")

    def pack_size(self, fmt, with_colors, with_intensities=False):
        n = C.c_int64()
        _check(self._L.dliom_points_batch_pack(self.h, int(fmt), int(with_colors), int(with_intensities), None, 0, C.byref(n)),
               "dliom_points_batch_pack")
        return int(n.value)

    def pack(self, fmt, with_colors, with_intensities=False, capacity=None, fill=0):
        """The writers' records -> uint8 array of `capacity` bytes (default: exactly the size) pre-filled with `fill`, and
        the number of bytes written."""
        size = self.pack_size(fmt, with_colors, with_intensities)
        out = np.full(size if capacity is None else int(capacity), fill, dtype=np.uint8)
        n = C.c_int64()
        _check(self._L.dliom_points_batch_pack(self.h, int(fmt), int(with_colors), int(with_intensities),
                                               _p(out, C.POINTER(C.c_uint8)), len(out), C.byref(n)), "dliom_points_batch_pack")
        return out, int(n.value)

    def pack_xyz_size(self):
        """The size of the batch's XYZ text in bytes (one read-back)."""
        return _pack_xyz_size(self._L.dliom_points_batch_pack_xyz, self.h)

    def pack_xyz(self, capacity=None, fill=0):
        """The XYZ writer's text ("x y z\\n" a point, every float as '%.6g') -> uint8 array of `capacity` bytes (default:
        exactly the size) pre-filled with `fill`, and the number of bytes written."""
        return _pack_xyz(self._L.dliom_points_batch_pack_xyz, self.h, capacity, fill)

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_points_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FixedRatioSampler:
    """common::FixedRatioSampler whose Pulse() loop over a batch runs on the device (dliom_fixed_ratio_sampler)."""

    def __init__(self, ratio):
        self._L = load_library()
        h = _vp()
        _check(self._L.dliom_fixed_ratio_sampler_create(float(ratio), C.byref(h)), "dliom_fixed_ratio_sampler_create")
        self.h = h

    def reset(self):
        _check(self._L.dliom_fixed_ratio_sampler_reset(self.h), "dliom_fixed_ratio_sampler_reset")

    def state(self):
        """-> (num_pulses, num_samples)"""
        a, b = C.c_int64(), C.c_int64()
        _check(self._L.dliom_fixed_ratio_sampler_state(self.h, C.byref(a), C.byref(b)), "dliom_fixed_ratio_sampler_state")
        return int(a.value), int(b.value)

    def stats(self):
        s = FixedRatioSamplerStats()
        _check(self._L.dliom_fixed_ratio_sampler_stats(self.h, C.byref(s)), "dliom_fixed_ratio_sampler_stats")
        return s.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_fixed_ratio_sampler_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ply_header(with_colors, with_intensities, num_points):
    """WriteBinaryPlyHeader (io/ply_writing_points_processor.cc:35-56) -> bytes."""
    return _text(lambda b, c, n: load_library().dliom_ply_header(int(with_colors), int(with_intensities), int(num_points), b, c, n))


def pcd_header(with_colors, num_points):
    """WriteBinaryPcdHeader (io/pcd_writing_points_processor.cc:35-57) -> bytes."""
    return _text(lambda b, c, n: load_library().dliom_pcd_header(int(with_colors), int(num_points), b, c, n))


SYMBOLS += [
    ("dliom_float_text", C.c_int, [C.c_float, C.c_char_p, _i32p]),
    ("dliom_points_batch_pack_xyz", C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_int64, _i64p]),
    ("dliom_cloud_pack_xyz", C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_int64, _i64p]),
]
XYZ_MAX_RECORD = 39  # DLIOM_XYZ_MAX_RECORD: "-1.17549e-38" three times, two spaces, one newline


def float_text(value):
    """What `std::ostream << std::setprecision(6) << float` writes for np.float32(value) -> bytes (dliom_float_text; host)."""
    buffer = C.create_string_buffer(16)
    n = C.c_int32()
    _check(load_library().dliom_float_text(C.c_float(np.float32(value)), buffer, C.byref(n)), "dliom_float_text")
    return buffer.raw[:n.value]


def _pack_xyz_size(entry, handle):
    n = C.c_int64()
    _check(entry(handle, None, 0, C.byref(n)), "pack_xyz")
    return int(n.value)


def _pack_xyz(entry, handle, capacity, fill):
    size = _pack_xyz_size(entry, handle) if capacity is None else int(capacity)
    out = np.full(size, fill, dtype=np.uint8)
    n = C.c_int64()
    _check(entry(handle, _p(out, C.POINTER(C.c_uint8)), len(out), C.byref(n)), "pack_xyz")
    return out, int(n.value)


KERNEL_PG_HITS, KERNEL_PG_RAYS, KERNEL_PG_CLEAR = 6, 7, 8
ERR_INTERNAL = -13
_u8p = C.POINTER(C.c_uint8)


def lookup_table_to_apply_correspondence_cost_odds(odds):
    """mapping/probability_values.cc:85-101"""
    out = np.zeros(32768, dtype=np.uint16)
    _check(load_library().dliom_compute_lookup_table_to_apply_correspondence_cost_odds(C.c_float(odds), _p(out, _u16p)),
           "correspondence cost lookup table")
    return out


def probability_grid_color_table():
    """The gray value of every cell value: 128 unknown, else ProbabilityToColor (probability_grid_points_processor.cc:49-54)."""
    out = np.zeros(32768, dtype=np.uint8)
    _check(load_library().dliom_probability_grid_color_table(_p(out, _u8p)), "color table")
    return out


def probability_grid_grow_limits(resolution, max_xy, num_cells, point_xy, budget_bytes=0):
    """Grid2D::GrowLimits on the limits alone -> (max_xy, num_cells, offset of the old cell (0, 0), doublings)."""
    mx, nc, off, turns = _f64(max_xy).copy(), np.array(num_cells, dtype=np.int32), np.zeros(2, dtype=np.int32), C.c_int32()
    _check(load_library().dliom_probability_grid_grow_limits(float(resolution), _p(mx, _f64p), _p(nc, _i32p), C.c_float(point_xy[0]),
                                                            C.c_float(point_xy[1]), int(budget_bytes), _p(off, _i32p),
                                                            C.byref(turns)), "dliom_probability_grid_grow_limits")
    return mx, nc, off, turns.value


def ros_map_yaml_origin(resolution, max_xy, offset, width, height):
    """ros_map_writing_points_processor.cc:73-76; width / height of the rotated image."""
    out = np.zeros(2)
    _check(load_library().dliom_ros_map_yaml_origin(float(resolution), _p(_f64(max_xy), _f64p),
                                                   _p(np.ascontiguousarray(offset, dtype=np.int32), _i32p), int(width), int(height),
                                                   _p(out, _f64p)), "dliom_ros_map_yaml_origin")
    return out


def _text(call):
    buf, n = C.create_string_buffer(1024), C.c_int64()
    _check(call(buf, 1024, C.byref(n)), "ros map text")
    return buf.raw[:n.value]


def ros_map_pgm_header(resolution, width, height):
    """WritePgm's header (ros_map.cc:23-26) -> bytes."""
    return _text(lambda b, c, n: load_library().dliom_ros_map_pgm_header(float(resolution), int(width), int(height), b, c, n))


def ros_map_yaml(resolution, origin, pgm_filename):
    """WriteYaml's text (ros_map.cc:41-45) -> bytes."""
    o = _f64(origin)
    return _text(lambda b, c, n: load_library().dliom_ros_map_yaml(float(resolution), _p(o, _f64p), pgm_filename.encode(), b, c, n))


class ProbabilityGrid2D:
    """mapping::ProbabilityGrid of the export pipeline in HBM (dliom_probability_grid).  limits=None:
    io::CreateProbabilityGrid(resolution); else (max_x, max_y, num_x_cells, num_y_cells)."""

    def __init__(self, ctx, resolution, limits=None, budget_bytes=0):
        self._L = ctx._L
        self.ctx = ctx
        h = _vp()
        if limits is None:
            _check(self._L.dliom_probability_grid_create(ctx.h, float(resolution), int(budget_bytes), C.byref(h)),
                   "dliom_probability_grid_create")
        else:
            _check(self._L.dliom_probability_grid_create_with_limits(ctx.h, float(resolution), float(limits[0]), float(limits[1]),
                                                                     int(limits[2]), int(limits[3]), int(budget_bytes),
                                                                     C.byref(h)), "dliom_probability_grid_create_with_limits")
        self.h = h

    def limits(self):
        """-> (resolution, (max_x, max_y), (num_x_cells, num_y_cells))"""
        r, mx, nc = C.c_double(), np.zeros(2), np.zeros(2, dtype=np.int32)
        _check(self._L.dliom_probability_grid_limits(self.h, C.byref(r), _p(mx, _f64p), _p(nc, _i32p)), "dliom_probability_grid_limits")
        return r.value, (float(mx[0]), float(mx[1])), (int(nc[0]), int(nc[1]))

    def cells(self, cropped=False):
        """-> (uint16 [num_y, num_x], offset (x, y)): the whole grid, or ComputeCroppedLimits' box."""
        off, num = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        _check(self._L.dliom_probability_grid_cells(self.h, None, 0, _p(off, _i32p), _p(num, _i32p), int(cropped)),
               "dliom_probability_grid_cells")
        out = np.zeros((int(num[1]), int(num[0])), dtype=np.uint16)
        _check(self._L.dliom_probability_grid_cells(self.h, _p(out, _u16p), out.size, _p(off, _i32p), _p(num, _i32p), int(cropped)),
               "dliom_probability_grid_cells")
        return out, (int(off[0]), int(off[1]))

    def get_probabilities(self, cell_xy):
        """GetProbability / IsKnown of cells (x, y) -> (float32, bool)."""
        xy = np.ascontiguousarray(cell_xy, dtype=np.int32).reshape(-1, 2)
        p, k = np.zeros(len(xy), dtype=np.float32), np.zeros(len(xy), dtype=np.uint8)
        _check(self._L.dliom_probability_grid_get_probabilities(self.h, _p(xy, _i32p), len(xy), _p(p, _f32p), _p(k, _u8p)),
               "dliom_probability_grid_get_probabilities")
        return p, k.astype(bool)

    def draw(self, rotate_cw=False):
        """DrawProbabilityGrid -> (uint8 [height, width], offset (x, y)); a fresh grid draws one unknown pixel."""
        off, size = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        _check(self._L.dliom_probability_grid_draw(self.h, None, 0, _p(off, _i32p), _p(size, _i32p), int(rotate_cw)),
               "dliom_probability_grid_draw")
        out = np.zeros((int(size[1]), int(size[0])), dtype=np.uint8)
        _check(self._L.dliom_probability_grid_draw(self.h, _p(out, _u8p), out.size, _p(off, _i32p), _p(size, _i32p), int(rotate_cw)),
               "dliom_probability_grid_draw")
        return out, (int(off[0]), int(off[1]))

    def stats(self):
        s = ProbabilityGridStats()
        _check(self._L.dliom_probability_grid_get_stats(self.h, C.byref(s)), "dliom_probability_grid_get_stats")
        d = {n: int(getattr(s, n)) for n in ("bytes", "growths", "inserts", "cells_visited", "error_word")}
        d["known_box"] = tuple(int(v) for v in s.known_box)
        return d

    def memory_stats(self):
        m = MemoryStats()
        _check(self._L.dliom_probability_grid_memory_stats(self.h, C.byref(m)), "dliom_probability_grid_memory_stats")
        return m.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_probability_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Inserter2D:
    """mapping::ProbabilityGridRangeDataInserter2D (dliom_inserter2d): insert(grid, origin, points) is one Insert with the
    points as returns and no misses, as the export pipeline calls it."""

    def __init__(self, ctx, hit_probability, miss_probability, insert_free_space=True):
        self._L = ctx._L
        self.ctx = ctx
        h = _vp()
        _check(self._L.dliom_inserter2d_create(ctx.h, float(hit_probability), float(miss_probability), int(insert_free_space),
                                               C.byref(h)), "dliom_inserter2d_create")
        self.h = h

    def tables(self):
        hit, miss = np.zeros(32768, dtype=np.uint16), np.zeros(32768, dtype=np.uint16)
        _check(self._L.dliom_inserter2d_tables(self.h, _p(hit, _u16p), _p(miss, _u16p)), "dliom_inserter2d_tables")
        return hit, miss

    def insert(self, grid, origin, points):
        """points: a PointCloud on the device, or an array (n, 3)."""
        o = _f32(origin)
        if isinstance(points, PointCloud):
            _check(self._L.dliom_inserter2d_insert_cloud(self.h, grid.h, _p(o, _f32p), points.h), "dliom_inserter2d_insert_cloud")
        else:
            pts = _f32(points).reshape(-1, 3)
            _check(self._L.dliom_inserter2d_insert(self.h, grid.h, _p(o, _f32p), _p(pts, _f32p), len(pts)), "dliom_inserter2d_insert")

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_inserter2d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HybridGrid:
    """Device-resident mapping::HybridGrid."""

    def __init__(self, ctx, resolution):
        self._L = ctx._L
        self.ctx = ctx
        self.resolution = float(np.float32(resolution))
        h = _vp()
        _check(self._L.dliom_grid_create(ctx.h, C.c_float(resolution), C.byref(h)), "dliom_grid_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bits(self):
        b = C.c_int()
        _check(self._L.dliom_grid_bits(self.h, C.byref(b)), "grid_bits")
        return b.value

    def memory_stats(self):
        """dliom_grid_memory_stats: this grid's HBM (leaf table, pool, mirror), capacity and slot upper bound; no sync."""
        m = MemoryStats()
        _check(self._L.dliom_grid_memory_stats(self.h, C.byref(m)), "grid_memory_stats")
        return m.as_dict()

    def mirror_stats(self):
        """(rebuilds, bytes, windowed) of the correlative matcher's dense mirror of this grid."""
        r, b, w = C.c_int64(), C.c_int64(), C.c_int()
        _check(self._L.dliom_grid_mirror_stats(self.h, C.byref(r), C.byref(b), C.byref(w)), "grid_mirror_stats")
        return int(r.value), int(b.value), bool(w.value)

    def upload_blocks(self, origins, values512):
        origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
        values512 = np.ascontiguousarray(values512, dtype=np.uint16).reshape(-1, 512)
        assert len(origins) == len(values512)
        _check(self._L.dliom_grid_upload_blocks(self.h, _p(origins, _i32p), _p(values512, _u16p), len(origins)),
               "grid_upload_blocks")

    def num_blocks(self):
        n = C.c_int64()
        _check(self._L.dliom_grid_num_blocks(self.h, C.byref(n)), "grid_num_blocks")
        return n.value

    def download_blocks(self):
        n = self.num_blocks()
        origins = np.zeros((n, 3), dtype=np.int32)
        values = np.zeros((n, 512), dtype=np.uint16)
        got = C.c_int64()
        _check(self._L.dliom_grid_download_blocks(self.h, _p(origins, _i32p), _p(values, _u16p), n, C.byref(got)),
               "grid_download_blocks")
        return origins[:got.value], values[:got.value]

    def cells(self):
        """Non-zero cells as a dict {(x,y,z): value} (what HybridGrid's iterator yields)."""
        origins, values = self.download_blocks()
        out = {}
        for o, v in zip(origins, values):
            nz = np.nonzero(v)[0]
            for c in nz:
                out[(int(o[0]) + (c & 7), int(o[1]) + ((c >> 3) & 7), int(o[2]) + (c >> 6))] = int(v[c])
        return out

    def to_proto(self):
        """Serialized mapping::proto::HybridGrid (bytes)."""
        n = C.c_int64()
        _check(self._L.dliom_grid_to_proto(self.h, None, 0, C.byref(n)), "dliom_grid_to_proto")
        buf = (C.c_uint8 * max(n.value, 1))()
        _check(self._L.dliom_grid_to_proto(self.h, buf, n.value, C.byref(n)), "dliom_grid_to_proto")
        return bytes(buf[:n.value])

    @classmethod
    def from_proto(cls, ctx, data):
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        h = _vp()
        _check(ctx._L.dliom_grid_from_proto(ctx.h, buf, len(data), C.byref(h)), "dliom_grid_from_proto")
        g = cls.__new__(cls)
        g._L = ctx._L
        g.ctx = ctx
        g.h = h
        res = C.c_float()
        _check(ctx._L.dliom_grid_resolution(h, C.byref(res)), "dliom_grid_resolution")
        g.resolution = res.value
        return g

    def set_values(self, cells_xyz, values):
        cells = np.ascontiguousarray(cells_xyz, dtype=np.int32).reshape(-1, 3)
        vals = np.ascontiguousarray(values, dtype=np.uint16)
        _check(self._L.dliom_grid_set_values(self.h, _p(cells, _i32p), _p(vals, _u16p), len(vals)), "grid_set_values")

    def SetProbability(self, index, probability):
        """hybrid_grid.h:489-491"""
        self.set_values([index], [self._L.dliom_probability_to_value(C.c_float(probability))])

    def values(self, cells_xyz):
        cells = np.ascontiguousarray(cells_xyz, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(len(cells), dtype=np.uint16)
        _check(self._L.dliom_grid_get_values(self.h, _p(cells, _i32p), len(cells), _p(out, _u16p)), "grid_get_values")
        return out


class RangeDataInserter3D:
    """mapping::RangeDataInserter3D: options -> two odds tables; Insert(range_data, grid).

    With a Context the tables live in HBM (dliom_inserter); without one the host tables are
    passed on every Insert (dliom_grid_insert)."""

    def __init__(self, hit_probability, miss_probability, num_free_space_voxels, ctx=None):
        if not hit_probability > 0.5 or not miss_probability < 0.5:
            raise ValueError("CHECK_GT(hit, 0.5) / CHECK_LT(miss, 0.5) (range_data_inserter_3d.cc:64-65)")
        self.num_free_space_voxels = int(num_free_space_voxels)
        self.h = None
        if ctx is not None:
            self._L = ctx._L
            h = _vp()
            _check(self._L.dliom_inserter_create(ctx.h, hit_probability, miss_probability,
                                                 self.num_free_space_voxels, C.byref(h)), "dliom_inserter_create")
            self.h = h
            self.hit_table = np.zeros(32768, dtype=np.uint16)
            self.miss_table = np.zeros(32768, dtype=np.uint16)
            _check(self._L.dliom_inserter_tables(h, _p(self.hit_table, _u16p), _p(self.miss_table, _u16p)),
                   "dliom_inserter_tables")
        else:
            # Odds(float(options.hit_probability()))
            self.hit_table = compute_lookup_table_to_apply_odds(odds(np.float32(hit_probability)))
            self.miss_table = compute_lookup_table_to_apply_odds(odds(np.float32(miss_probability)))

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_inserter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Insert(self, origin, returns, grid):
        origin = _f32(origin)
        returns = _f32(returns).reshape(-1, 3)
        if self.h is not None:
            _check(grid._L.dliom_inserter_insert(self.h, grid.h, _p(origin, _f32p), _p(returns, _f32p), len(returns)),
                   "dliom_inserter_insert")
        else:
            _check(grid._L.dliom_grid_insert(grid.h, _p(origin, _f32p), _p(returns, _f32p), len(returns),
                                             _p(self.hit_table, _u16p), _p(self.miss_table, _u16p),
                                             self.num_free_space_voxels), "dliom_grid_insert")

    def InsertCloud(self, grid, cloud, poses=(), origin=(0.0, 0.0, 0.0), max_range=0.0):
        """Submap3D::InsertRangeData's data path on the device: transform the HBM-resident cloud
        through `poses` (0..2 float poses, applied in order), range-filter, insert."""
        assert self.h is not None, "InsertCloud needs an inserter created with a Context"
        poses = _f32(np.asarray(poses, dtype=np.float32).reshape(-1, 7)) if len(poses) else np.zeros((0, 7), np.float32)
        origin = _f32(origin)
        _check(grid._L.dliom_inserter_insert_cloud(self.h, grid.h, _p(poses, _f32p), len(poses), _p(origin, _f32p),
                                                   cloud.h, C.c_float(max_range)), "dliom_inserter_insert_cloud")


def insert_cloud_multi(inserter, cloud, targets, origin=(0.0, 0.0, 0.0)):
    """targets: list of (grid, poses (0..2 float poses), max_range).  One set of launches, one sync."""
    k = len(targets)
    grids = (_vp * k)(*[g.h for g, _, _ in targets])
    poses = np.zeros((k, 14), dtype=np.float32)
    nposes = (C.c_int * k)()
    ranges = np.zeros(k, dtype=np.float32)
    for i, (_, ps, mr) in enumerate(targets):
        ps = np.asarray(ps, dtype=np.float32).reshape(-1, 7) if len(ps) else np.zeros((0, 7), np.float32)
        nposes[i] = len(ps)
        poses[i, :7 * len(ps)] = ps.reshape(-1)
        ranges[i] = mr
    _check(inserter._L.dliom_inserter_insert_cloud_multi(inserter.h, k, grids, _p(poses, _f32p), nposes,
                                                         _p(_f32(origin), _f32p), cloud.h, _p(ranges, _f32p)),
           "dliom_inserter_insert_cloud_multi")


def _rtcsm_opts(o):
    return RtcsmOptions(o["linear_search_window"], o["angular_search_window"],
                        o["translation_delta_cost_weight"], o["rotation_delta_cost_weight"])


class RealTimeCorrelativeScanMatcher3D:
    def __init__(self, ctx, options):
        self.ctx = ctx
        self._L = ctx._L
        self.options = _rtcsm_opts(options)

    def Match(self, initial_pose_estimate, point_cloud, hybrid_grid):
        """Returns (score, pose_estimate[7]).  point_cloud: ndarray or PointCloud."""
        init = _f64(initial_pose_estimate)
        out = np.zeros(7)
        score = C.c_float()
        if isinstance(point_cloud, PointCloud):
            s = self._L.dliom_rtcsm3d_match_cloud(self.ctx.h, C.byref(self.options), _p(init, _f64p), point_cloud.h,
                                                  hybrid_grid.h, _p(out, _f64p), C.byref(score))
        else:
            pts = _f32(point_cloud).reshape(-1, 3)
            s = self._L.dliom_rtcsm3d_match(self.ctx.h, C.byref(self.options), _p(init, _f64p), _p(pts, _f32p),
                                            len(pts), hybrid_grid.h, _p(out, _f64p), C.byref(score))
        _check(s, "dliom_rtcsm3d_match")
        return score.value, out

    def window(self, resolution, point_cloud):
        pts = _f32(point_cloud).reshape(-1, 3)
        w = RtcsmWindow()
        _check(self._L.dliom_rtcsm3d_window(C.byref(self.options), C.c_float(resolution), _p(pts, _f32p), len(pts),
                                            C.byref(w)), "dliom_rtcsm3d_window")
        return w

    def box_error(self):
        f = C.c_uint32(0)
        _check(self._L.dliom_rtcsm3d_box_error(self.ctx.h, C.byref(f)), "box_error")
        return f.value

    def last_stats(self):
        st = RtcsmStats()
        _check(self._L.dliom_rtcsm3d_last_stats(self.ctx.h, C.byref(st)), "last_stats")
        return st

    def sequential_sums(self, initial_pose_estimate, point_cloud, hybrid_grid, candidate_indices, method):
        pts = _f32(point_cloud).reshape(-1, 3)
        idx = np.ascontiguousarray(candidate_indices, dtype=np.int64)
        out = np.zeros(len(idx), dtype=np.float32)
        _check(self._L.dliom_rtcsm3d_sequential_sums(self.ctx.h, C.byref(self.options),
                                                     _p(_f64(initial_pose_estimate), _f64p), _p(pts, _f32p), len(pts),
                                                     hybrid_grid.h, _p(idx, _i64p), len(idx), int(method),
                                                     _p(out, _f32p)), "dliom_rtcsm3d_sequential_sums")
        return out

    def score_volume(self, initial_pose_estimate, point_cloud, hybrid_grid):
        init = _f64(initial_pose_estimate)
        pts = _f32(point_cloud).reshape(-1, 3)
        n = C.c_int64()
        _check(self._L.dliom_rtcsm3d_score_volume(self.ctx.h, C.byref(self.options), _p(init, _f64p), _p(pts, _f32p),
                                                  len(pts), hybrid_grid.h, None, 0, C.byref(n)), "score_volume(size)")
        sums = np.zeros(n.value, dtype=np.uint64)
        _check(self._L.dliom_rtcsm3d_score_volume(self.ctx.h, C.byref(self.options), _p(init, _f64p), _p(pts, _f32p),
                                                  len(pts), hybrid_grid.h, _p(sums, _u64p), n.value, C.byref(n)),
               "score_volume")
        return sums


class RtcsmShard:
    """One rank's share of a sharded RealTimeCorrelativeScanMatcher3D::Match (BASELINE config 4): match() is the
    one-collective protocol of dliom_rtcsm3d_match_sharded (the collective is the caller's function), begin / finish /
    decode the three local phases of the two-collective variant."""

    def match(self, initial_pose_estimate, cloud, hybrid_grid, all_reduce_max):
        """all_reduce_max(int) -> int: MAX over the ranks of one unsigned 64-bit value."""
        def cb(value_ptr, _user):
            try:
                value_ptr[0] = int(all_reduce_max(int(value_ptr[0])))
                return 0
            except Exception:
                return 1
        fn = EXCHANGE_FN(cb)
        out, score = np.zeros(7), C.c_float()
        _check(self._L.dliom_rtcsm3d_match_sharded(self.ctx.h, C.byref(self.options), _p(_f64(initial_pose_estimate), _f64p),
                                                   cloud.h, hybrid_grid.h, self.shard, self.num_shards, fn, None,
                                                   _p(out, _f64p), C.byref(score)), "dliom_rtcsm3d_match_sharded")
        return score.value, out

    def match_rccl(self, initial_pose_estimate, cloud, hybrid_grid, nccl_comm):
        """nccl_comm: an ncclComm_t as an integer / c_void_p; rank and size are the communicator's."""
        out, score = np.zeros(7), C.c_float()
        _check(self._L.dliom_rtcsm3d_match_sharded_rccl(self.ctx.h, C.byref(self.options),
                                                        _p(_f64(initial_pose_estimate), _f64p), cloud.h, hybrid_grid.h,
                                                        C.c_void_p(nccl_comm), _p(out, _f64p), C.byref(score)),
               "dliom_rtcsm3d_match_sharded_rccl")
        return score.value, out

    def __init__(self, ctx, options, shard, num_shards):
        self.ctx = ctx
        self._L = ctx._L
        self.options = _rtcsm_opts(options)
        self.shard, self.num_shards = int(shard), int(num_shards)

    def begin(self, initial_pose_estimate, cloud, hybrid_grid):
        bits = C.c_uint32()
        _check(self._L.dliom_rtcsm3d_shard_begin(self.ctx.h, C.byref(self.options), _p(_f64(initial_pose_estimate), _f64p),
                                                 cloud.h, hybrid_grid.h, self.shard, self.num_shards, C.byref(bits)),
               "dliom_rtcsm3d_shard_begin")
        return bits.value

    def finish(self, global_best_lower_bound_bits):
        packed = C.c_uint64()
        _check(self._L.dliom_rtcsm3d_shard_finish(self.ctx.h, int(global_best_lower_bound_bits), C.byref(packed)),
               "dliom_rtcsm3d_shard_finish")
        return packed.value

    def decode(self, global_best_packed):
        out = np.zeros(7)
        score = C.c_float()
        _check(self._L.dliom_rtcsm3d_shard_decode(self.ctx.h, int(global_best_packed), _p(out, _f64p), C.byref(score)),
               "dliom_rtcsm3d_shard_decode")
        return score.value, out


def _csm_opts(o):
    c = CsmOptions()
    w = list(o["occupied_space_weight"])
    c.num_occupied_space_weights = len(w)
    for i, v in enumerate(w[:MAX_CLOUDS]):
        c.occupied_space_weight[i] = v
    c.translation_weight = o["translation_weight"]
    c.rotation_weight = o["rotation_weight"]
    c.only_optimize_yaw = int(o.get("only_optimize_yaw", False))
    c.use_nonmonotonic_steps = int(o.get("use_nonmonotonic_steps", False))
    c.max_num_iterations = int(o["max_num_iterations"])
    c.num_threads = int(o.get("num_threads", 1))
    return c


class CeresScanMatcher3D:
    def __init__(self, ctx, options):
        self.ctx = ctx
        self._L = ctx._L
        self.options = _csm_opts(options)

    def Match(self, target_translation, initial_pose_estimate, point_clouds_and_hybrid_grids):
        """Returns (pose_estimate[7], summary dict)."""
        k = len(point_clouds_and_hybrid_grids)
        tgt = _f64(target_translation)
        init = _f64(initial_pose_estimate)
        out = np.zeros(7)
        summ = CsmSummary()
        grids = (_vp * k)(*[g.h for _, g in point_clouds_and_hybrid_grids])
        if all(isinstance(c, PointCloud) for c, _ in point_clouds_and_hybrid_grids):
            clouds = (_vp * k)(*[c.h for c, _ in point_clouds_and_hybrid_grids])
            s = self._L.dliom_csm3d_match_cloud(self.ctx.h, C.byref(self.options), _p(tgt, _f64p), _p(init, _f64p), k,
                                                clouds, grids, _p(out, _f64p), C.byref(summ))
        else:
            arrs = [_f32(c).reshape(-1, 3) for c, _ in point_clouds_and_hybrid_grids]
            ptrs = (_f32p * k)(*[_p(a, _f32p) for a in arrs])
            ns = np.array([len(a) for a in arrs], dtype=np.int64)
            s = self._L.dliom_csm3d_match(self.ctx.h, C.byref(self.options), _p(tgt, _f64p), _p(init, _f64p), k, ptrs,
                                          _p(ns, _i64p), grids, _p(out, _f64p), C.byref(summ))
        _check(s, "dliom_csm3d_match")
        return out, {f: getattr(summ, f) for f, _ in CsmSummary._fields_}

    def match_batch(self, problems):
        """dliom_csm3d_match_batch.  problems: (target_translation, initial_pose_estimate, [(cloud, grid), ...]) with
        clouds as PointCloud or (n, 3) arrays.  Returns (poses[n, 7], summaries, statuses, stats); every pose and summary
        equals Match() of the same problem."""
        n = len(problems)
        arr = (CsmProblem * max(n, 1))()
        keep = []
        for i, (tgt, init, pairs) in enumerate(problems):
            q = arr[i]
            q.target_translation[:] = [float(v) for v in tgt]
            q.initial_pose_estimate[:] = [float(v) for v in init]
            q.num_clouds = len(pairs)
            for j, (c, g) in enumerate(pairs[:MAX_CLOUDS]):
                q.grids[j] = g.h
                if isinstance(c, PointCloud):
                    q.clouds[j] = c.h
                else:
                    a = _f32(c).reshape(-1, 3)
                    keep.append(a)
                    q.points_xyz[j] = _p(a, _f32p)
                    q.n[j] = len(a)
        poses = np.zeros((max(n, 1), 7))
        summ = (CsmSummary * max(n, 1))()
        st = (C.c_int * max(n, 1))()
        stats = BatchStats()
        _check(self._L.dliom_csm3d_match_batch(self.ctx.h, C.byref(self.options), n, arr, _p(poses, _f64p), summ, st,
                                               C.byref(stats)), "dliom_csm3d_match_batch")
        return (poses[:n], [{f: getattr(summ[i], f) for f, _ in CsmSummary._fields_} for i in range(n)],
                [st[i] for i in range(n)], {f: getattr(stats, f) for f, _ in BatchStats._fields_})

    def evaluate(self, target_translation, initial_pose_estimate, pose, point_clouds_and_hybrid_grids):
        k = len(point_clouds_and_hybrid_grids)
        arrs = [_f32(c).reshape(-1, 3) for c, _ in point_clouds_and_hybrid_grids]
        ptrs = (_f32p * k)(*[_p(a, _f32p) for a in arrs])
        ns = np.array([len(a) for a in arrs], dtype=np.int64)
        grids = (_vp * k)(*[g.h for _, g in point_clouds_and_hybrid_grids])
        cost = C.c_double()
        grad = np.zeros(6)
        jtj = np.zeros((6, 6))
        _check(self._L.dliom_csm3d_evaluate(self.ctx.h, C.byref(self.options), _p(_f64(target_translation), _f64p),
                                            _p(_f64(initial_pose_estimate), _f64p), _p(_f64(pose), _f64p), k, ptrs,
                                            _p(ns, _i64p), grids, C.byref(cost), _p(grad, _f64p), _p(jtj, _f64p)),
               "dliom_csm3d_evaluate")
        return cost.value, grad, jtj


def submap3d_to_proto(local_pose7, num_range_data, finished, high_grid_proto=None, low_grid_proto=None, wrap=False):
    """Serialized mapping::proto::Submap3D (or proto::Submap around it) -- Submap3D::ToProto, host only."""
    L = load_library()

    def buf(b):
        return (None, 0) if b is None else ((C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if len(b) else b"\0"), len(b))
    (hp, hn), (lp, ln) = buf(high_grid_proto), buf(low_grid_proto)
    if high_grid_proto is not None and hn == 0:
        hp = (C.c_uint8 * 1)()
    if low_grid_proto is not None and ln == 0:
        lp = (C.c_uint8 * 1)()
    pose = _f64(local_pose7)
    n = C.c_int64()
    args = (_p(pose, _f64p), int(num_range_data), int(bool(finished)), hp, hn, lp, ln, int(bool(wrap)))
    _check(L.dliom_submap3d_to_proto(*args, None, 0, C.byref(n)), "dliom_submap3d_to_proto")
    out = (C.c_uint8 * max(n.value, 1))()
    _check(L.dliom_submap3d_to_proto(*args, out, n.value, C.byref(n)), "dliom_submap3d_to_proto")
    return bytes(out[:n.value])


def submap3d_from_proto(data, wrapped=False):
    """(local_pose7, num_range_data, finished, high grid bytes or None, low grid bytes or None)."""
    L = load_library()
    b = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
    pose = np.zeros(7)
    n, fin = C.c_int32(), C.c_int()
    ho, hs, lo, ls = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _check(L.dliom_submap3d_from_proto(b, len(data), int(bool(wrapped)), _p(pose, _f64p), C.byref(n), C.byref(fin),
                                       C.byref(ho), C.byref(hs), C.byref(lo), C.byref(ls)), "dliom_submap3d_from_proto")
    hi = None if hs.value < 0 else bytes(data[ho.value:ho.value + hs.value])
    low = None if ls.value < 0 else bytes(data[lo.value:lo.value + ls.value])
    return pose, n.value, bool(fin.value), hi, low


# ---- compressed point clouds and trajectory node data (dliom.h "compressed point clouds") ----
_u8p = C.POINTER(C.c_uint8)


class TrajectoryNodeData(C.Structure):
    _fields_ = [("timestamp", C.c_int64), ("gravity_alignment_wxyz", C.c_double * 4), ("filtered_gravity_aligned", _vp),
                ("high_resolution", _vp), ("low_resolution", _vp), ("histogram", _f32p), ("histogram_size", C.c_int),
                ("local_pose7", C.c_double * 7)]


SYMBOLS += [
    ("dliom_trajectory_nodes_data_to_proto", C.c_int, [_vp, C.POINTER(TrajectoryNodeData), C.c_int, _u8p, C.c_int64, _i64p,
                                                       C.POINTER(C.c_int)]),
    ("dliom_clouds_compress", C.c_int, [_vp, C.POINTER(_vp), C.c_int, _i32p, C.c_int64, _i64p, C.POINTER(C.c_int)]),
    ("dliom_cloud_compress", C.c_int, [_vp, _vp, _i32p, C.c_int64, _i64p]),
    ("dliom_clouds_compress_to_proto", C.c_int, [_vp, C.POINTER(_vp), C.c_int, _u8p, C.c_int64, _i64p, C.POINTER(C.c_int)]),
    ("dliom_cloud_decompress", C.c_int, [_vp, C.c_int32, _i32p, C.c_int64, C.POINTER(_vp)]),
    ("dliom_cloud_from_compressed_proto", C.c_int, [_vp, _u8p, C.c_int64, C.POINTER(_vp)]),
    ("dliom_compressed_point_cloud_to_proto", C.c_int, [C.c_int32, _i32p, C.c_int64, _u8p, C.c_int64, _i64p]),
    ("dliom_compressed_point_cloud_from_proto", C.c_int, [_u8p, C.c_int64, C.POINTER(C.c_int32), _i32p, C.c_int64, _i64p]),
    ("dliom_compressed_point_cloud_check", C.c_int, [C.c_int32, _i32p, C.c_int64]),
    ("dliom_trajectory_node_data_to_proto", C.c_int, [_vp, C.c_int64, _f64p, _vp, _vp, _vp, _f32p, C.c_int, _f64p, _u8p,
                                                      C.c_int64, _i64p]),
    ("dliom_trajectory_node_data_from_proto", C.c_int, [_vp, _u8p, C.c_int64, _i64p, _f64p, C.POINTER(_vp), C.POINTER(_vp),
                                                        C.POINTER(_vp), _f32p, C.c_int, C.POINTER(C.c_int), _f64p]),
]


class CloudRefused(DliomError):
    """A batch refused by Compress's bound check: first_refused is the lowest offending cloud's index."""

    def __init__(self, status, where, first_refused):
        super().__init__(status, where)
        self.first_refused = first_refused


def _bytes_in(data):
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) if len(data) else b"\0")


def _cloud_handles(clouds):
    return (_vp * max(len(clouds), 1))(*[None if c is None else c.h for c in clouds])


def _compress_call(fn, name, ctx, clouds, dtype):
    """Query-then-fill of a batched compression -> (flat output, offsets[k + 1])."""
    k, handles = len(clouds), _cloud_handles(clouds)
    offsets, refused = np.zeros(k + 1, dtype=np.int64), C.c_int(-1)

    def call(out, capacity):
        s = fn(ctx.h, handles, k, out, capacity, _p(offsets, _i64p), C.byref(refused))
        if s == ERR_GRID_EXTENT and refused.value >= 0:
            raise CloudRefused(s, name, refused.value)
        _check(s, name)
    call(None, 0)
    out = np.zeros(max(int(offsets[k]), 1), dtype=dtype)
    call(_p(out, C.POINTER(C.c_int32 if dtype == np.int32 else C.c_uint8)), int(offsets[k]))
    return out[:int(offsets[k])], offsets


def compress_point_clouds(ctx, clouds):
    """sensor::CompressedPointCloud(cloud) for every PointCloud of the list (None: the empty cloud), one batch on the
    device -> [(num_points, int32 point_data)]."""
    out, off = _compress_call(ctx._L.dliom_clouds_compress, "dliom_clouds_compress", ctx, clouds, np.int32)
    return [(0 if c is None else len(c), out[off[i]:off[i + 1]].copy()) for i, c in enumerate(clouds)]


def compress_point_clouds_to_proto(ctx, clouds):
    """The serialized sensor::proto::CompressedPointCloud of every cloud of the list, one batch -> [bytes]."""
    out, off = _compress_call(ctx._L.dliom_clouds_compress_to_proto, "dliom_clouds_compress_to_proto", ctx, clouds, np.uint8)
    return [out[off[i]:off[i + 1]].tobytes() for i in range(len(clouds))]


def compress_point_cloud(ctx, cloud):
    """(num_points, int32 point_data) of one PointCloud: the batch of one (dliom_cloud_compress)."""
    n = C.c_int64()
    try:
        _check(ctx._L.dliom_cloud_compress(ctx.h, cloud.h, None, 0, C.byref(n)), "dliom_cloud_compress")
    except DliomError as e:
        if e.status == ERR_GRID_EXTENT:
            raise CloudRefused(e.status, "dliom_cloud_compress", 0)
        raise
    out = np.zeros(max(n.value, 1), dtype=np.int32)
    _check(ctx._L.dliom_cloud_compress(ctx.h, cloud.h, _p(out, _i32p), n.value, C.byref(n)), "dliom_cloud_compress")
    return len(cloud), out[:n.value]


def _words(point_data):
    return np.ascontiguousarray(point_data, dtype=np.int32).reshape(-1)


def decompress_point_cloud(ctx, num_points, point_data):
    """CompressedPointCloud::Decompress on the device -> PointCloud; a malformed stream is refused."""
    w, h = _words(point_data), _vp()
    _check(ctx._L.dliom_cloud_decompress(ctx.h, int(num_points), _p(w, _i32p), len(w), C.byref(h)), "dliom_cloud_decompress")
    return PointCloud(ctx, _handle=h)


def point_cloud_from_compressed_proto(ctx, data):
    """A serialized sensor::proto::CompressedPointCloud -> PointCloud on the device."""
    h = _vp()
    _check(ctx._L.dliom_cloud_from_compressed_proto(ctx.h, _bytes_in(data), len(data), C.byref(h)),
           "dliom_cloud_from_compressed_proto")
    return PointCloud(ctx, _handle=h)


def compressed_point_cloud_to_proto(num_points, point_data):
    """Serialized sensor::proto::CompressedPointCloud around words the caller holds (host only)."""
    L, w, n = load_library(), _words(point_data), C.c_int64()
    args = (int(num_points), _p(w, _i32p), len(w))
    _check(L.dliom_compressed_point_cloud_to_proto(*args, None, 0, C.byref(n)), "dliom_compressed_point_cloud_to_proto")
    out = (C.c_uint8 * max(n.value, 1))()
    _check(L.dliom_compressed_point_cloud_to_proto(*args, out, n.value, C.byref(n)), "dliom_compressed_point_cloud_to_proto")
    return bytes(out[:n.value])


def compressed_point_cloud_from_proto(data):
    """(num_points, int32 point_data) of a serialized sensor::proto::CompressedPointCloud (host only, not validated)."""
    L, b, n, num = load_library(), _bytes_in(data), C.c_int64(), C.c_int32()
    _check(L.dliom_compressed_point_cloud_from_proto(b, len(data), C.byref(num), None, 0, C.byref(n)),
           "dliom_compressed_point_cloud_from_proto")
    out = np.zeros(max(n.value, 1), dtype=np.int32)
    _check(L.dliom_compressed_point_cloud_from_proto(b, len(data), C.byref(num), _p(out, _i32p), n.value, C.byref(n)),
           "dliom_compressed_point_cloud_from_proto")
    return num.value, out[:n.value]


def compressed_point_cloud_check(num_points, point_data):
    """True for a stream Decompress accepts (host only): counts > 0 that sum to num_points, no truncation, no trailing
    words, every point word in [0, 2^30)."""
    w = _words(point_data)
    s = load_library().dliom_compressed_point_cloud_check(int(num_points), _p(w, _i32p), len(w))
    if s not in (OK, ERR_INVALID_ARGUMENT):
        _check(s, "dliom_compressed_point_cloud_check")
    return s == OK


def trajectory_nodes_data_to_proto(ctx, nodes):
    """The serialized mapping::proto::TrajectoryNodeData of every node of the list -- dicts with timestamp,
    gravity_alignment (w, x, y, z), filtered_gravity_aligned, high_resolution, low_resolution (PointClouds on `ctx` or
    None: empty), histogram, local_pose -- all clouds compressed as one batch -> [bytes]."""
    count = len(nodes)
    structs, keep = (TrajectoryNodeData * max(count, 1))(), []
    for s, node in zip(structs, nodes):
        hist = _f32(node["histogram"]).reshape(-1)
        keep.append(hist)
        s.timestamp = int(node["timestamp"])
        s.gravity_alignment_wxyz[:] = [float(v) for v in node["gravity_alignment"]]
        for name in ("filtered_gravity_aligned", "high_resolution", "low_resolution"):
            setattr(s, name, None if node.get(name) is None else node[name].h)
        s.histogram, s.histogram_size = _p(hist, _f32p), len(hist)
        s.local_pose7[:] = list(_pose7(node["local_pose"]))
    offsets, refused = np.zeros(count + 1, dtype=np.int64), C.c_int(-1)
    where = "dliom_trajectory_nodes_data_to_proto"

    def call(out, capacity):
        st = ctx._L.dliom_trajectory_nodes_data_to_proto(ctx.h, structs, count, out, capacity, _p(offsets, _i64p), C.byref(refused))
        if st == ERR_GRID_EXTENT and refused.value >= 0:
            raise CloudRefused(st, where, refused.value)
        _check(st, where)
    call(None, 0)
    out = (C.c_uint8 * max(int(offsets[count]), 1))()
    call(out, int(offsets[count]))
    blob = bytes(out)
    return [blob[offsets[i]:offsets[i + 1]] for i in range(count)]


def trajectory_node_data_to_proto(ctx, timestamp, gravity_alignment_wxyz, filtered_gravity_aligned, high_resolution,
                                  low_resolution, histogram, local_pose7):
    """Serialized mapping::proto::TrajectoryNodeData (mapping::ToProto(TrajectoryNode::Data)); the clouds are PointClouds
    on `ctx` or None (empty), compressed as one batch."""
    g, pose, hist = _f64(gravity_alignment_wxyz), _pose7(local_pose7), _f32(histogram).reshape(-1)
    h = [None if c is None else c.h for c in (filtered_gravity_aligned, high_resolution, low_resolution)]
    n = C.c_int64()
    args = (ctx.h, int(timestamp), _p(g, _f64p), h[0], h[1], h[2], _p(hist, _f32p), len(hist), _p(pose, _f64p))
    where = "dliom_trajectory_node_data_to_proto"
    _check(ctx._L.dliom_trajectory_node_data_to_proto(*args, None, 0, C.byref(n)), where)
    out = (C.c_uint8 * max(n.value, 1))()
    _check(ctx._L.dliom_trajectory_node_data_to_proto(*args, out, n.value, C.byref(n)), where)
    return bytes(out[:n.value])


def trajectory_node_data_from_proto(ctx, data, histogram_capacity=1024):
    """mapping::FromProto(TrajectoryNodeData) -> dict(timestamp, gravity_alignment (w, x, y, z), filtered_gravity_aligned,
    high_resolution, low_resolution (PointClouds on the device), histogram, local_pose (x, y, z, qw, qx, qy, qz))."""
    g, pose, hist = np.zeros(4), np.zeros(7), np.zeros(max(histogram_capacity, 1), dtype=np.float32)
    t, hn, h = C.c_int64(), C.c_int(), [_vp(), _vp(), _vp()]
    s = ctx._L.dliom_trajectory_node_data_from_proto(ctx.h, _bytes_in(data), len(data), C.byref(t), _p(g, _f64p), C.byref(h[0]),
                                                     C.byref(h[1]), C.byref(h[2]), _p(hist, _f32p), histogram_capacity,
                                                     C.byref(hn), _p(pose, _f64p))
    if s == ERR_CAPACITY and hn.value > histogram_capacity:
        return trajectory_node_data_from_proto(ctx, data, hn.value)
    _check(s, "dliom_trajectory_node_data_from_proto")
    clouds = [PointCloud(ctx, _handle=x) for x in h]
    return dict(timestamp=t.value, gravity_alignment=g, filtered_gravity_aligned=clouds[0], high_resolution=clouds[1],
                low_resolution=clouds[2], histogram=hist[:hn.value].copy(), local_pose=pose)


XRAY_MAX_PIXELS = 1 << 26  # DLIOM_XRAY_MAX_PIXELS


def _pose7(pose):
    p = _f64(pose).reshape(-1)
    if p.shape != (7,):
        raise ValueError("pose must be (tx, ty, tz, qw, qx, qy, qz)")
    return p


def grid_xray_texture(grid, pose):
    """Submap3D::ToResponseProto's texture of one grid (submap_3d.cc:53-177) at `global_submap_pose`, on the device:
    (width, height, resolution, slice_pose7, cells) with cells the uncompressed (height, width, 2) uint8 array of
    (value, alpha).  An empty projection is 0 x 0."""
    p = _pose7(pose)
    w, h, res = C.c_int32(), C.c_int32(), C.c_double()
    slice_pose = np.zeros(7, dtype=np.float64)
    L = grid._L
    _check(L.dliom_grid_xray_texture(grid.h, _p(p, _f64p), None, 0, C.byref(w), C.byref(h), C.byref(res),
                                     _p(slice_pose, _f64p)), "dliom_grid_xray_texture")
    cells = np.zeros((h.value, w.value, 2), dtype=np.uint8)
    if cells.size:
        _check(L.dliom_grid_xray_texture(grid.h, _p(p, _f64p), _p(cells, C.POINTER(C.c_uint8)), cells.size, C.byref(w),
                                         C.byref(h), C.byref(res), _p(slice_pose, _f64p)), "dliom_grid_xray_texture")
    return w.value, h.value, res.value, slice_pose, cells


def grid_project_to_image(grid, pose):
    """D-LIOM's ProjectToCvMat (submap_3d.cc:381-443) on the device: (image, ox, oy, resolution) with image the
    (height, width) uint8 array the reference wraps in a CV_8UC1 cv::Mat (values reduced modulo 256, empty pixels
    224).  An empty projection is 0 x 0."""
    p = _pose7(pose)
    w, h, ox, oy, res = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_double()
    L = grid._L
    _check(L.dliom_grid_project_to_image(grid.h, _p(p, _f64p), None, 0, C.byref(w), C.byref(h), C.byref(ox), C.byref(oy),
                                         C.byref(res)), "dliom_grid_project_to_image")
    image = np.zeros((h.value, w.value), dtype=np.uint8)
    if image.size:
        _check(L.dliom_grid_project_to_image(grid.h, _p(p, _f64p), _p(image, C.POINTER(C.c_uint8)), image.size, C.byref(w),
                                             C.byref(h), C.byref(ox), C.byref(oy), C.byref(res)),
               "dliom_grid_project_to_image")
    return image, ox.value, oy.value, res.value


def probability_to_log_odds_integer(probability):
    """ProbabilityToLogOddsInteger (mapping/submaps.h:37-52) from the library's step table (host)."""
    return int(load_library().dliom_probability_to_log_odds_integer(C.c_float(probability)))


def voxel_filter(size, points):
    """sensor::VoxelFilter(size).Filter(points) (host)."""
    pts = _f32(points).reshape(-1, 3)
    out = np.zeros_like(pts)
    n = C.c_int64()
    _check(load_library().dliom_voxel_filter(C.c_float(size), _p(pts, _f32p), len(pts), _p(out, _f32p), C.byref(n)),
           "dliom_voxel_filter")
    return out[:n.value].copy()


def adaptive_voxel_filter(max_length, min_num_points, max_range, points):
    """sensor::AdaptiveVoxelFilter(options).Filter(points) (host)."""
    pts = _f32(points).reshape(-1, 3)
    out = np.zeros_like(pts)
    n = C.c_int64()
    o = AdaptiveVoxelFilterOptions(max_length, min_num_points, max_range)
    _check(load_library().dliom_adaptive_voxel_filter(C.byref(o), _p(pts, _f32p), len(pts), _p(out, _f32p), C.byref(n)),
           "dliom_adaptive_voxel_filter")
    return out[:n.value].copy()


class _BorrowedGrid(HybridGrid):
    """A grid owned by a front end (never destroyed from Python)."""

    def __init__(self, ctx, handle, resolution):
        self._L = ctx._L
        self.ctx = ctx
        self.resolution = float(np.float32(resolution))
        self.h = handle

    def close(self):
        self.h = None


def front_end_options_struct(options):
    """dliom_front_end_options from the nested dict the tests and tools use."""
    o = FrontEndOptions()
    hi, lo = options["high_resolution_adaptive_voxel_filter"], options["low_resolution_adaptive_voxel_filter"]
    o.high_resolution_adaptive_voxel_filter = AdaptiveVoxelFilterOptions(hi["max_length"], hi["min_num_points"], hi["max_range"])
    o.low_resolution_adaptive_voxel_filter = AdaptiveVoxelFilterOptions(lo["max_length"], lo["min_num_points"], lo["max_range"])
    o.use_online_correlative_scan_matching = int(options["use_online_correlative_scan_matching"])
    o.real_time_correlative_scan_matcher = _rtcsm_opts(options["real_time_correlative_scan_matcher"])
    o.ceres_scan_matcher = _csm_opts(options["ceres_scan_matcher"])
    m, s = options["motion_filter"], options["submaps"]
    o.motion_filter_max_time_seconds = m["max_time_seconds"]
    o.motion_filter_max_distance_meters = m["max_distance_meters"]
    o.motion_filter_max_angle_radians = m["max_angle_radians"]
    o.high_resolution = s["high_resolution"]
    o.high_resolution_max_range = s["high_resolution_max_range"]
    o.low_resolution = s["low_resolution"]
    o.num_range_data = s["num_range_data"]
    o.hit_probability = s["hit_probability"]
    o.miss_probability = s["miss_probability"]
    o.num_free_space_voxels = s["num_free_space_voxels"]
    return o


class LocalTrajectoryBuilder3D:
    """AddAccumulatedRangeData + InsertIntoSubmap of the reference's LocalTrajectoryBuilder3D
    (local_trajectory_builder_3d.cc:493-622), over ActiveSubmaps3D; WindowOptimize sits between match and insert
    (dliom.ImuWindow)."""

    def __init__(self, ctx, options):
        self.ctx = ctx
        self._L = ctx._L
        o = FrontEndOptions()
        hi, lo = options["high_resolution_adaptive_voxel_filter"], options["low_resolution_adaptive_voxel_filter"]
        o.high_resolution_adaptive_voxel_filter = AdaptiveVoxelFilterOptions(hi["max_length"], hi["min_num_points"], hi["max_range"])
        o.low_resolution_adaptive_voxel_filter = AdaptiveVoxelFilterOptions(lo["max_length"], lo["min_num_points"], lo["max_range"])
        o.use_online_correlative_scan_matching = int(options["use_online_correlative_scan_matching"])
        o.real_time_correlative_scan_matcher = _rtcsm_opts(options["real_time_correlative_scan_matcher"])
        o.ceres_scan_matcher = _csm_opts(options["ceres_scan_matcher"])
        m, s = options["motion_filter"], options["submaps"]
        o.motion_filter_max_time_seconds = m["max_time_seconds"]
        o.motion_filter_max_distance_meters = m["max_distance_meters"]
        o.motion_filter_max_angle_radians = m["max_angle_radians"]
        o.high_resolution = s["high_resolution"]
        o.high_resolution_max_range = s["high_resolution_max_range"]
        o.low_resolution = s["low_resolution"]
        o.num_range_data = s["num_range_data"]
        o.hit_probability = s["hit_probability"]
        o.miss_probability = s["miss_probability"]
        o.num_free_space_voxels = s["num_free_space_voxels"]
        self.resolutions = (s["high_resolution"], s["low_resolution"])
        h = _vp()
        _check(self._L.dliom_front_end_create(ctx.h, C.byref(o), C.byref(h)), "dliom_front_end_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_front_end_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def match(self, pose_prediction, origin, returns):
        returns = _f32(returns).reshape(-1, 3)
        r = MatchResult()
        _check(self._L.dliom_front_end_match(self.h, _p(_f64(pose_prediction), _f64p), _p(_f32(origin), _f32p),
                                             _p(returns, _f32p), len(returns), C.byref(r)), "dliom_front_end_match")
        return self._result(r)

    @staticmethod
    def _result(r):
        return dict(dropped=bool(r.dropped), pose_estimate=np.array(r.pose_estimate),
                    pose_observation_in_submap=np.array(r.pose_observation_in_submap),
                    initial_ceres_pose=np.array(r.initial_ceres_pose), rtcsm_score=r.rtcsm_score,
                    final_cost=r.summary.final_cost, num_iterations=r.summary.num_iterations,
                    num_high=r.num_high_resolution_points, num_low=r.num_low_resolution_points,
                    residual_distance=r.residual_distance, residual_angle=r.residual_angle,
                    matching_submap_index=r.matching_submap_index)

    def match_cloud(self, pose_prediction, origin, cloud):
        """match() on range data that already lives on the device (keep `cloud` alive until insert())."""
        r = MatchResult()
        _check(self._L.dliom_front_end_match_cloud(self.h, _p(_f64(pose_prediction), _f64p), _p(_f32(origin), _f32p),
                                                   cloud.h, C.byref(r)), "dliom_front_end_match_cloud")
        return self._result(r)

    def insert(self, time_ticks, pose_estimate, gravity_alignment):
        r = InsertionResult()
        _check(self._L.dliom_front_end_insert(self.h, int(time_ticks), _p(_f64(pose_estimate), _f64p),
                                              _p(_f64(gravity_alignment), _f64p), C.byref(r)), "dliom_front_end_insert")
        return dict(inserted=bool(r.inserted), num_insertion_submaps=r.num_insertion_submaps,
                    insertion_submap_index=list(r.insertion_submap_index)[:r.num_insertion_submaps],
                    submap_added=bool(r.submap_added), submap_finished=bool(r.submap_finished))

    def num_active_submaps(self):
        n = C.c_int()
        _check(self._L.dliom_front_end_num_active_submaps(self.h, C.byref(n)), "num_active_submaps")
        return n.value

    def matching_index(self):
        n = C.c_int()
        _check(self._L.dliom_front_end_matching_index(self.h, C.byref(n)), "matching_index")
        return n.value

    def num_finished_submaps(self):
        n = C.c_int()
        _check(self._L.dliom_front_end_num_finished_submaps(self.h, C.byref(n)), "num_finished_submaps")
        return n.value

    def take_finished_submap(self):
        """Oldest finished submap; its grids are OWNED by the returned HybridGrid objects (close() frees them)."""
        pose = np.zeros(7)
        n = C.c_int()
        hi, lo = _vp(), _vp()
        _check(self._L.dliom_front_end_take_finished_submap(self.h, _p(pose, _f64p), C.byref(n), C.byref(hi), C.byref(lo)),
               "take_finished_submap")
        grids = []
        for h, res in ((hi, self.resolutions[0]), (lo, self.resolutions[1])):
            g = HybridGrid.__new__(HybridGrid)
            g._L, g.ctx, g.resolution, g.h = self._L, self.ctx, float(np.float32(res)), h
            grids.append(g)
        return dict(local_pose=pose, num_range_data=n.value, hi=grids[0], lo=grids[1])

    def active_submap(self, i):
        pose = np.zeros(7)
        n, fin = C.c_int(), C.c_int()
        hi, lo = _vp(), _vp()
        _check(self._L.dliom_front_end_active_submap(self.h, i, _p(pose, _f64p), C.byref(n), C.byref(fin),
                                                     C.byref(hi), C.byref(lo)), "active_submap")
        return dict(local_pose=pose, num_range_data=n.value, finished=bool(fin.value),
                    hi=_BorrowedGrid(self.ctx, hi, self.resolutions[0]), lo=_BorrowedGrid(self.ctx, lo, self.resolutions[1]))


class RealTimeCorrelativeScanMatcher2D:
    """BASELINE config 1: the 2D matcher over a dense ProbabilityGrid, host only by contract."""

    def __init__(self, options):
        self._L = load_library()
        self.options = _rtcsm_opts(options)

    def Match(self, initial_pose_estimate, point_cloud, cells, resolution, max_xy):
        """cells: uint16 [num_y_cells, num_x_cells] correspondence-cost values.  Returns (score, pose[3])."""
        pts = _f32(point_cloud).reshape(-1, 3)
        cells = np.ascontiguousarray(cells, dtype=np.uint16)
        out = np.zeros(3)
        score = C.c_double()
        _check(self._L.dliom_rtcsm2d_match(C.byref(self.options), _p(_f64(initial_pose_estimate), _f64p),
                                           _p(pts, _f32p), len(pts), _p(cells, _u16p), cells.shape[1], cells.shape[0],
                                           resolution, max_xy[0], max_xy[1], _p(out, _f64p), C.byref(score)),
               "dliom_rtcsm2d_match")
        return score.value, out


def deskew(ctx, prev_pose, predicted_pose, scan_period, hits_xyzt, origin, min_range, max_range):
    """local_trajectory_builder_3d.cc:421-472 on the device.  Returns (xyz[n,3], kind[n], current_pose[7] float32)."""
    h = _f32(hits_xyzt).reshape(-1, 4)
    n = len(h)
    out = np.zeros((n, 3), dtype=np.float32)
    kind = np.zeros(n, dtype=np.uint8)
    cur = np.zeros(7, dtype=np.float32)
    _check(ctx._L.dliom_deskew(ctx.h, _p(_f64(prev_pose), _f64p), _p(_f64(predicted_pose), _f64p), scan_period,
                               _p(h, _f32p), n, _p(_f32(origin), _f32p), C.c_float(min_range), C.c_float(max_range),
                               _p(out, _f32p), kind.ctypes.data_as(C.POINTER(C.c_uint8)), _p(cur, _f32p)), "dliom_deskew")
    return out, kind, cur


def add_range_data_preprocess(ctx, prev_pose, predicted_pose, scan_period, ranges_xyzt, origin, min_range, max_range,
                              voxel_filter_size):
    """AddRangeData's pre-processing chain (:393-487): VoxelFilter(0.5 vfs) [host] -> de-skew + range gate
    [device] -> VoxelFilter(vfs) [host] -> back to the tracking frame by current_pose.inverse() [host,
    float].  Returns (returns_in_tracking, origin_in_tracking, current_pose)."""
    r = _f32(ranges_xyzt).reshape(-1, 4)
    keep = voxel_filter_indices(0.5 * np.float32(voxel_filter_size), r[:, :3])
    hits = r[keep]
    xyz, kind, cur = deskew(ctx, prev_pose, predicted_pose, scan_period, hits, origin, min_range, max_range)
    returns = voxel_filter(voxel_filter_size, xyz[kind == 1])
    inv = _pose_inverse_f32(cur)
    return _transform_f32(inv, returns), _transform_f32(inv, cur[:3].reshape(1, 3))[0], cur


def add_range_data(ctx, prev_pose, predicted_pose, scan_period, ranges_xyzt, origin, min_range, max_range,
                   voxel_filter_size):
    """The same chain entirely on the device (dliom_add_range_data).
    Returns (PointCloud returns_in_tracking, origin_in_tracking, current_pose)."""
    r = _f32(ranges_xyzt).reshape(-1, 4)
    h = _vp()
    o = np.zeros(3, dtype=np.float32)
    cur = np.zeros(7, dtype=np.float32)
    _check(ctx._L.dliom_add_range_data(ctx.h, _p(_f64(prev_pose), _f64p), _p(_f64(predicted_pose), _f64p), scan_period,
                                       _p(r, _f32p), len(r), _p(_f32(origin), _f32p), C.c_float(min_range),
                                       C.c_float(max_range), C.c_float(voxel_filter_size), C.byref(h), _p(o, _f32p),
                                       _p(cur, _f32p)), "dliom_add_range_data")
    return PointCloud(ctx, _handle=h), o, cur


def voxel_filter_indices(size, points):
    """Indices kept by sensor::VoxelFilter (first point per voxel), via the host filter."""
    pts = _f32(points).reshape(-1, 3)
    kept = voxel_filter(size, pts)
    # the filter preserves order and keeps exact copies: recover the indices by a single sweep
    idx = np.zeros(len(kept), dtype=np.int64)
    j = 0
    for i in range(len(pts)):
        if j < len(kept) and pts[i, 0] == kept[j, 0] and pts[i, 1] == kept[j, 1] and pts[i, 2] == kept[j, 2]:
            idx[j] = i
            j += 1
    assert j == len(kept)
    return idx


def _pose_inverse_f32(p):
    """Rigid3f::inverse() in float32 with Eigen's operation order (transform/rigid_transform.h:167-171)."""
    f = np.float32
    w, x, y, z = f(p[3]), f(-p[4]), f(-p[5]), f(-p[6])
    t = _transform_f32(np.array([0, 0, 0, w, x, y, z], dtype=np.float32), np.asarray(p[:3], dtype=np.float32).reshape(1, 3))[0]
    return np.array([-t[0], -t[1], -t[2], w, x, y, z], dtype=np.float32)


def _transform_f32(pose, pts):
    """rigid * point in float32: uv = 2 (u x v); (v + w uv) + u x uv, then + t."""
    f = np.float32
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    w, ux, uy, uz = f(pose[3]), f(pose[4]), f(pose[5]), f(pose[6])
    vx, vy, vz = pts[:, 0], pts[:, 1], pts[:, 2]
    uvx = uy * vz - uz * vy
    uvy = uz * vx - ux * vz
    uvz = ux * vy - uy * vx
    uvx = uvx + uvx
    uvy = uvy + uvy
    uvz = uvz + uvz
    cx = uy * uvz - uz * uvy
    cy = uz * uvx - ux * uvz
    cz = ux * uvy - uy * uvx
    out = np.stack([((vx + w * uvx) + cx) + f(pose[0]), ((vy + w * uvy) + cy) + f(pose[1]),
                    ((vz + w * uvz) + cz) + f(pose[2])], axis=1)
    return out.astype(np.float32)


class FastCorrelativeScanMatcher3D:
    """mapping::scan_matching::FastCorrelativeScanMatcher3D on the device (dliom_fast_csm_*); `nodes` are given
    as the (histogram, yaw) pairs HistogramsAtAnglesFromNodes extracts."""

    def __init__(self, ctx, hybrid_grid, low_resolution_hybrid_grid, node_histograms, node_angles, options):
        self.ctx = ctx
        self._L = ctx._L
        h = _f32(node_histograms).reshape(len(node_angles), -1)
        self.hist_size = h.shape[1]
        self.grids = (hybrid_grid, low_resolution_hybrid_grid)
        o = FastCsmOptions(options["branch_and_bound_depth"], options["full_resolution_depth"],
                           options["min_rotational_score"], options["min_low_resolution_score"],
                           options["linear_xy_search_window"], options["linear_z_search_window"],
                           options["angular_search_window"])
        hnd = _vp()
        _check(self._L.dliom_fast_csm_create(ctx.h, hybrid_grid.h, low_resolution_hybrid_grid.h, _p(h, _f32p),
                                             _p(_f32(node_angles), _f32p), h.shape[0], h.shape[1], C.byref(o),
                                             C.byref(hnd)), "dliom_fast_csm_create")
        self.h = hnd
        self.depth = options["branch_and_bound_depth"]

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_fast_csm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level(self, depth):
        """(lo[3], values[nz, ny, nx] uint8) of one pyramid level."""
        lo = np.zeros(3, dtype=np.int32)
        dims = np.zeros(3, dtype=np.int32)
        _check(self._L.dliom_fast_csm_level(self.h, depth, _p(lo, _i32p), _p(dims, _i32p), None, 0), "level")
        v = np.zeros((int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.uint8)
        if v.size:
            _check(self._L.dliom_fast_csm_level(self.h, depth, _p(lo, _i32p), _p(dims, _i32p),
                                                v.ctypes.data_as(C.POINTER(C.c_uint8)), v.size), "level")
        return lo, v

    def _data(self, data):
        self._hi = _f32(data["high_resolution_point_cloud"]).reshape(-1, 3)
        self._lo = _f32(data["low_resolution_point_cloud"]).reshape(-1, 3)
        self._hist = _f32(data["rotational_scan_matcher_histogram"])
        assert len(self._hist) == self.hist_size
        d = FastCsmNodeData()
        for i in range(4):
            d.gravity_alignment[i] = float(data["gravity_alignment"][i])
        d.high_resolution_points = _p(self._hi, _f32p)
        d.num_high_resolution_points = len(self._hi)
        d.low_resolution_points = _p(self._lo, _f32p)
        d.num_low_resolution_points = len(self._lo)
        d.rotational_scan_matcher_histogram = _p(self._hist, _f32p)
        return d

    @staticmethod
    def _result(r):
        return dict(found=bool(r.found), score=np.float32(r.score), rotational_score=np.float32(r.rotational_score),
                    low_resolution_score=np.float32(r.low_resolution_score), num_discrete_scans=r.num_discrete_scans,
                    num_scored_candidates=r.num_scored_candidates, num_score_launches=r.num_score_launches,
                    pose=np.array(r.pose_estimate) if r.found else None)

    def Match(self, global_node_pose, global_submap_pose, data, min_score, ctx=None):
        """ctx: the calling thread's Context (default: the one the matcher was created on)."""
        d, r = self._data(data), FastCsmResult()
        _check(self._L.dliom_fast_csm_match((ctx or self.ctx).h, self.h, _p(_f64(global_node_pose), _f64p), _p(_f64(global_submap_pose), _f64p),
                                            C.byref(d), C.c_float(min_score), C.byref(r)), "dliom_fast_csm_match")
        return self._result(r)

    def MatchFullSubmap(self, global_node_rotation, global_submap_rotation, data, min_score, ctx=None):
        d, r = self._data(data), FastCsmResult()
        _check(self._L.dliom_fast_csm_match_full_submap((ctx or self.ctx).h, self.h, _p(_f64(global_node_rotation), _f64p),
                                                        _p(_f64(global_submap_rotation), _f64p), C.byref(d),
                                                        C.c_float(min_score), C.byref(r)), "dliom_fast_csm_match_full_submap")
        return self._result(r)

    def MatchWith3DofInitial(self, pose_in_submap_guess, data, min_score, ctx=None):
        d, r = self._data(data), FastCsmResult()
        _check(self._L.dliom_fast_csm_match_with_3dof_initial((ctx or self.ctx).h, self.h, _p(_f64(pose_in_submap_guess), _f64p), C.byref(d),
                                                              C.c_float(min_score), C.byref(r)),
               "dliom_fast_csm_match_with_3dof_initial")
        return self._result(r)


def fast_csm_match_batch(ctx, queries):
    """dliom_fast_csm_match_batch.  queries: dicts with kind ("Match", "MatchFullSubmap", "MatchWith3DofInitial"),
    matcher (FastCorrelativeScanMatcher3D), the kind's pose arguments (global_node_pose + global_submap_pose,
    global_node_rotation + global_submap_rotation, or pose_in_submap_guess), data (as for Match) and min_score.
    Returns (results, statuses, stats); results[i] is what the single call returns (its dict)."""
    L = ctx._L
    n = len(queries)
    arr = (FastCsmQuery * max(n, 1))()
    keep = []
    for i, q in enumerate(queries):
        m = q["matcher"]
        kind = _FAST_CSM_KINDS[q["kind"]]
        d = m._data(q["data"])
        keep.append((m._hi, m._lo, m._hist))
        a = arr[i]
        a.kind = kind
        a.matcher = m.h
        if kind == FAST_CSM_MATCH:
            a.pose[:] = [float(v) for v in q["global_node_pose"]]
            a.submap_pose[:] = [float(v) for v in q["global_submap_pose"]]
        elif kind == FAST_CSM_MATCH_FULL_SUBMAP:
            a.pose[:4] = [float(v) for v in q["global_node_rotation"]]
            a.submap_pose[:4] = [float(v) for v in q["global_submap_rotation"]]
        else:
            a.pose[:] = [float(v) for v in q["pose_in_submap_guess"]]
        a.node_data = d
        a.histogram_size = m.hist_size
        a.min_score = float(q["min_score"])
    res = (FastCsmResult * max(n, 1))()
    st = (C.c_int * max(n, 1))()
    stats = BatchStats()
    _check(L.dliom_fast_csm_match_batch(ctx.h, arr, n, res, st, C.byref(stats)), "dliom_fast_csm_match_batch")
    return ([FastCorrelativeScanMatcher3D._result(res[i]) for i in range(n)], [st[i] for i in range(n)],
            {f: getattr(stats, f) for f, _ in BatchStats._fields_})


def compute_constraints(ctx, queries, ceres_scan_matcher):
    """ConstraintBuilder3D::ComputeConstraint's three stages (constraint_builder_3d.cc:202-334) for a list of queries
    (fast_csm_match_batch's dicts): the fast estimate, the prune when it finds nothing, and CeresScanMatcher3D::Match
    with target = the match's translation, initial = the match's pose and the clouds {high resolution, B's high
    resolution grid}, {low resolution, B's low resolution grid}.  Returns per query None (no constraint) or a dict with
    the fast search's result under "match" and the refined pose under "pose"; and the two calls' stats."""
    results, statuses, fast_stats = fast_csm_match_batch(ctx, queries)
    for s in statuses:
        _check(s, "dliom_fast_csm_match_batch")
    found = [i for i, r in enumerate(results) if r["found"]]
    problems = []
    for i in found:
        q, r = queries[i], results[i]
        hi_grid, lo_grid = q["matcher"].grids
        problems.append((r["pose"][:3], r["pose"], [(q["data"]["high_resolution_point_cloud"], hi_grid),
                                                   (q["data"]["low_resolution_point_cloud"], lo_grid)]))
    poses, _, csm_statuses, csm_stats = ceres_scan_matcher.match_batch(problems)
    for s in csm_statuses:
        _check(s, "dliom_csm3d_match_batch")
    out = [None] * len(queries)
    for k, i in enumerate(found):
        out[i] = dict(match=results[i], pose=poses[k])
    return out, fast_stats, csm_stats


def cloud_rotational_histogram(ctx, cloud, histogram_size, rotation_wxyz=None):
    """RotationalScanMatcher::ComputeHistogram on the device (dliom_cloud_rotational_histogram) of a device cloud,
    optionally rotated by a float quaternion first (the gravity alignment)."""
    out = np.zeros(histogram_size, dtype=np.float32)
    rot = None if rotation_wxyz is None else _p(_f32(rotation_wxyz), _f32p)
    _check(load_library().dliom_cloud_rotational_histogram(ctx.h, cloud.h, rot, int(histogram_size), _p(out, _f32p)),
           "dliom_cloud_rotational_histogram")
    return out


def cloud_rotational_histogram_begin(ctx, cloud, histogram_size, rotation_wxyz=None):
    """First half of cloud_rotational_histogram: the kernels go onto the context's auxiliary stream and the call returns."""
    rot = None if rotation_wxyz is None else _p(_f32(rotation_wxyz), _f32p)
    _check(load_library().dliom_cloud_rotational_histogram_begin(ctx.h, cloud.h, rot, int(histogram_size)),
           "dliom_cloud_rotational_histogram_begin")


def cloud_rotational_histogram_finish(ctx, histogram_size):
    """Second half: waits for the pending histogram of the context and returns it."""
    out = np.zeros(histogram_size, dtype=np.float32)
    _check(load_library().dliom_cloud_rotational_histogram_finish(ctx.h, _p(out, _f32p)), "dliom_cloud_rotational_histogram_finish")
    return out


def diag_sequential_sums(ctx, values, acc0=None):
    """dliom_diag_sequential_sums: the device's exact parallel replay of sequential float sums; values (k, n)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    k, n = v.shape
    a = np.zeros(k, dtype=np.float32) if acc0 is None else np.ascontiguousarray(acc0, dtype=np.float32).reshape(k)
    out = np.zeros(k, dtype=np.float32)
    _check(load_library().dliom_diag_sequential_sums(ctx.h, _p(v, _f32p), k, n, _p(a, _f32p), _p(out, _f32p)),
           "dliom_diag_sequential_sums")
    return out


def diag_histogram_contributions(ctx, cloud, histogram_size, rotation_wxyz=None):
    """dliom_diag_histogram_contributions: (buckets, values) of every addition the device histogram is made of, in order."""
    cap = int(cloud.n) + 1
    buckets = np.zeros(cap, dtype=np.int32)
    values = np.zeros(cap, dtype=np.float32)
    count = C.c_int64(0)
    rot = None if rotation_wxyz is None else _p(_f32(rotation_wxyz), _f32p)
    _check(load_library().dliom_diag_histogram_contributions(ctx.h, cloud.h, rot, int(histogram_size),
                                                             buckets.ctypes.data_as(C.POINTER(C.c_int32)), _p(values, _f32p), cap,
                                                             C.byref(count)), "dliom_diag_histogram_contributions")
    return buckets[:count.value].copy(), values[:count.value].copy()


def diag_std_sort_order(ctx, keys):
    """dliom_diag_std_sort_order: the device's restatement of std::sort's order (ties included); <= 4096 keys through the
    LDS path of the small slices, more through the HBM path."""
    keys = _f32(keys).reshape(-1)
    out = np.zeros(len(keys), dtype=np.int32)
    _check(load_library().dliom_diag_std_sort_order(ctx.h, _p(keys, _f32p), len(keys), out.ctypes.data_as(C.POINTER(C.c_int32))),
           "dliom_diag_std_sort_order")
    return out


def rotational_histogram(points, histogram_size, threads=None):
    """RotationalScanMatcher::ComputeHistogram (host); threads: explicit host thread count (same bits at any)."""
    pts = _f32(points).reshape(-1, 3)
    out = np.zeros(histogram_size, dtype=np.float32)
    if threads is None:
        _check(load_library().dliom_rotational_histogram(_p(pts, _f32p), len(pts), histogram_size, _p(out, _f32p)),
               "dliom_rotational_histogram")
    else:
        _check(load_library().dliom_rotational_histogram_mt(_p(pts, _f32p), len(pts), histogram_size, int(threads), _p(out, _f32p)),
               "dliom_rotational_histogram_mt")
    return out


ERR_DIVERGED = -11


class RangeDataAccumulator:
    """dliom_range_accumulator_*: AddRangeData calls feeding one AddAccumulatedRangeData
    (num_accumulated_range_data > 1), with the RangeDataSynchronizer's origin table."""

    def __init__(self, ctx):
        self.ctx, self._L = ctx, ctx._L
        h = _vp()
        _check(self._L.dliom_range_accumulator_create(ctx.h, C.byref(h)), "dliom_range_accumulator_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_range_accumulator_destroy(self.h)
            self.h = None

    __del__ = close

    def add(self, prev_pose, predicted_pose, scan_period, ranges_xyzt, min_range, max_range, voxel_filter_size,
            origins=((0.0, 0.0, 0.0),), origin_index=None):
        r = _f32(ranges_xyzt).reshape(-1, 4)
        og = _f32(origins).reshape(-1, 3)
        oi = None if origin_index is None else _f32(origin_index)
        cur = np.zeros(7, dtype=np.float32)
        k = C.c_int()
        _check(self._L.dliom_range_accumulator_add(self.h, _p(_f64(prev_pose), _f64p), _p(_f64(predicted_pose), _f64p),
                                                   float(scan_period), _p(r, _f32p), None if oi is None else _p(oi, _f32p),
                                                   len(r), _p(og, _f32p), len(og), C.c_float(min_range), C.c_float(max_range),
                                                   C.c_float(voxel_filter_size), _p(cur, _f32p), C.byref(k)),
               "dliom_range_accumulator_add")
        return cur, k.value

    def add_timed_cloud(self, prev_pose, predicted_pose, scan_period, ranges, min_range, max_range, voxel_filter_size,
                        origins=((0.0, 0.0, 0.0),)):
        """dliom_range_accumulator_add_timed_cloud: add() with the ranges and the origin index taken from a TimedCloud."""
        og = _f32(origins).reshape(-1, 3)
        cur = np.zeros(7, dtype=np.float32)
        k = C.c_int()
        _check(self._L.dliom_range_accumulator_add_timed_cloud(self.h, _p(_f64(prev_pose), _f64p), _p(_f64(predicted_pose), _f64p),
                                                               float(scan_period), ranges.h, _p(og, _f32p), len(og),
                                                               C.c_float(min_range), C.c_float(max_range),
                                                               C.c_float(voxel_filter_size), _p(cur, _f32p), C.byref(k)),
               "dliom_range_accumulator_add_timed_cloud")
        return cur, k.value

    def finish(self, voxel_filter_size):
        h = _vp()
        org = np.zeros(3, dtype=np.float32)
        _check(self._L.dliom_range_accumulator_finish(self.h, C.c_float(voxel_filter_size), C.byref(h), _p(org, _f32p)),
               "dliom_range_accumulator_finish")
        return PointCloud(self.ctx, _handle=h), org


class ImuWindow:
    """LocalTrajectoryBuilder3D::WindowOptimize without GTSAM (dliom_imu_window_*; host): IMU-preintegration factor,
    bias random walk, matched-pose prior and gravity factor in a fixed-lag Gauss-Newton smoother."""

    def __init__(self, **overrides):
        self._L = load_library()
        self.options = ImuWindowOptions()
        _check(self._L.dliom_imu_window_default_options(C.byref(self.options)), "dliom_imu_window_default_options")
        for k, v in overrides.items():
            setattr(self.options, k, v)
        h = _vp()
        _check(self._L.dliom_imu_window_create(C.byref(self.options), C.byref(h)), "dliom_imu_window_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_imu_window_destroy(self.h)
            self.h = None

    __del__ = close

    def initialize(self, pose7, velocity, bias6):
        _check(self._L.dliom_imu_window_initialize(self.h, _p(_f64(pose7), _f64p), _p(_f64(velocity), _f64p),
                                                   _p(_f64(bias6), _f64p)), "dliom_imu_window_initialize")

    def add_imu(self, acc, gyr, dt):
        _check(self._L.dliom_imu_window_add_imu(self.h, _p(_f64(acc), _f64p), _p(_f64(gyr), _f64p), float(dt)),
               "dliom_imu_window_add_imu")

    def add_imu_batch(self, acc, gyr, dt):
        """n samples in one call (acc, gyr: n x 3; dt: scalar or n)."""
        acc, gyr = _f64(acc).reshape(-1, 3), _f64(gyr).reshape(-1, 3)
        dts = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (len(acc),)))
        _check(self._L.dliom_imu_window_add_imu_batch(self.h, len(acc), _p(acc, _f64p), _p(gyr, _f64p), _p(dts, _f64p)),
               "dliom_imu_window_add_imu_batch")

    def predict(self):
        pose, vel = np.zeros(7), np.zeros(3)
        _check(self._L.dliom_imu_window_predict(self.h, _p(pose, _f64p), _p(vel, _f64p)), "dliom_imu_window_predict")
        return pose, vel

    def add_gravity(self, states_back, direction):
        _check(self._L.dliom_imu_window_add_gravity(self.h, int(states_back), _p(_f64(direction), _f64p)),
               "dliom_imu_window_add_gravity")

    def add_pose(self, matched_pose7, is_drift=False):
        """Returns (pose7, velocity, bias6, status); status is 0 or ERR_DIVERGED (FailureDetection)."""
        pose, vel, bias = np.zeros(7), np.zeros(3), np.zeros(6)
        s = self._L.dliom_imu_window_add_pose(self.h, _p(_f64(matched_pose7), _f64p), int(bool(is_drift)), _p(pose, _f64p),
                                              _p(vel, _f64p), _p(bias, _f64p))
        if s not in (ERR_DIVERGED, ERR_SOLVER):
            _check(s, "dliom_imu_window_add_pose")
        return pose, vel, bias, s

    def window_optimize(self, matched_pose7, is_drift=False):
        """LocalTrajectoryBuilder3D::WindowOptimize as the reference calls it: the first call after initialize() only starts
        the graph and returns the initial state; every later one is add_pose.  Returns (pose7, velocity, bias6, status)."""
        pose, vel, bias = np.zeros(7), np.zeros(3), np.zeros(6)
        s = self._L.dliom_imu_window_window_optimize(self.h, _p(_f64(matched_pose7), _f64p), int(bool(is_drift)), _p(pose, _f64p),
                                                     _p(vel, _f64p), _p(bias, _f64p))
        if s not in (ERR_DIVERGED, ERR_SOLVER):
            _check(s, "dliom_imu_window_window_optimize")
        return pose, vel, bias, s

    def state(self, states_back=0):
        pose, vel, bias = np.zeros(7), np.zeros(3), np.zeros(6)
        _check(self._L.dliom_imu_window_state(self.h, int(states_back), _p(pose, _f64p), _p(vel, _f64p), _p(bias, _f64p)),
               "dliom_imu_window_state")
        return pose, vel, bias

    def __len__(self):
        return int(self._L.dliom_imu_window_size(self.h))

    def solver_stats(self):
        """(linearisation points moved, chain blocks eliminated) so far."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(self._L.dliom_imu_window_solver_stats(self.h, C.byref(a), C.byref(b)), "dliom_imu_window_solver_stats")
        return int(a.value), int(b.value)

    def gravity_estimate(self):
        """(g_vec_est_G_, passed the reference's gates?, gravity factors added so far) -- EstimateGravity, .cc:1106-1154."""
        g, ok, n = np.zeros(3), C.c_int(0), C.c_int64(0)
        _check(self._L.dliom_imu_window_gravity_estimate(self.h, _p(g, _f64p), C.byref(ok), C.byref(n)),
               "dliom_imu_window_gravity_estimate")
        return g, bool(ok.value), int(n.value)

    def diag_imu_factor_jacobians(self):
        """(analytic, numeric) 15 x 30 Jacobians of the IMU factor between the two newest states."""
        a, b = np.zeros((15, 30)), np.zeros((15, 30))
        _check(self._L.dliom_diag_imu_factor_jacobians(self.h, _p(a, _f64p), _p(b, _f64p)), "dliom_diag_imu_factor_jacobians")
        return a, b


def gravity_estimate(poses7, delta_t, delta_p, delta_v, velocities, gravity_norm, lidar_in_imu_translation=(0.0, 0.0, 0.0)):
    """GravityEstimator::Estimate (gravity_estimator.cc:172-188) -> (gravity in the first frame, accepted)."""
    poses7 = _f64(poses7).reshape(-1, 7)
    g, ok = np.zeros(3), C.c_int(0)
    _check(load_library().dliom_gravity_estimate(len(poses7), _p(poses7, _f64p), _p(_f64(delta_t), _f64p),
                                                 _p(_f64(delta_p).reshape(-1, 3), _f64p), _p(_f64(delta_v).reshape(-1, 3), _f64p),
                                                 _p(_f64(velocities).reshape(-1, 3), _f64p),
                                                 _p(_f64(lidar_in_imu_translation), _f64p), float(gravity_norm), _p(g, _f64p),
                                                 C.byref(ok)), "dliom_gravity_estimate")
    return g, bool(ok.value)


class ImuIntegrator:
    """IMU preintegration between two scans (dliom_imu_integrator_*; host)."""

    def __init__(self, ba, bg, noise):
        self._L = load_library()
        self._noise = ImuNoise(*[float(x) for x in noise])
        h = _vp()
        _check(self._L.dliom_imu_integrator_create(_p(_f64(ba), _f64p), _p(_f64(bg), _f64p), C.byref(self._noise),
                                                   C.byref(h)), "dliom_imu_integrator_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_imu_integrator_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, ba, bg):
        _check(self._L.dliom_imu_integrator_reset(self.h, _p(_f64(ba), _f64p), _p(_f64(bg), _f64p), C.byref(self._noise)),
               "dliom_imu_integrator_reset")

    def push_back(self, dt, acc, gyr):
        _check(self._L.dliom_imu_integrator_push_back(self.h, float(dt), _p(_f64(acc), _f64p), _p(_f64(gyr), _f64p)),
               "dliom_imu_integrator_push_back")

    def repropagate(self, ba, bg):
        _check(self._L.dliom_imu_integrator_repropagate(self.h, _p(_f64(ba), _f64p), _p(_f64(bg), _f64p)),
               "dliom_imu_integrator_repropagate")

    def get(self):
        o = ImuPreintegration()
        _check(self._L.dliom_imu_integrator_get(self.h, C.byref(o)), "dliom_imu_integrator_get")
        return dict(sum_dt=o.sum_dt, delta_p=np.array(o.delta_p), delta_q=np.array(o.delta_q),
                    delta_v=np.array(o.delta_v), jacobian=np.array(o.jacobian).reshape(15, 15),
                    covariance=np.array(o.covariance).reshape(15, 15))

    def evaluate(self, state_i, state_j, gravity):
        r = np.zeros(15)
        _check(self._L.dliom_imu_integrator_evaluate(self.h, _p(_f64(state_i), _f64p), _p(_f64(state_j), _f64p),
                                                     _p(_f64(gravity), _f64p), _p(r, _f64p)), "dliom_imu_integrator_evaluate")
        return r

    def predict(self, state_i, gravity):
        sj = np.zeros(16)
        _check(self._L.dliom_imu_integrator_predict(self.h, _p(_f64(state_i), _f64p), _p(_f64(gravity), _f64p),
                                                    _p(sj, _f64p)), "dliom_imu_integrator_predict")
        return sj


def rotational_scan_match(node_histograms, node_angles, scan_histogram, initial_angle, angles):
    """RotationalScanMatcher(nodes).Match(histogram, initial_angle, angles) (host)."""
    h = _f32(node_histograms).reshape(len(node_angles), -1)
    a = _f32(angles)
    out = np.zeros(len(a), dtype=np.float32)
    _check(load_library().dliom_rotational_scan_match(_p(h, _f32p), _p(_f32(node_angles), _f32p), h.shape[0], h.shape[1],
                                                      _p(_f32(scan_histogram), _f32p), C.c_float(initial_angle),
                                                      _p(a, _f32p), len(a), _p(out, _f32p)), "dliom_rotational_scan_match")
    return out


# ---- pose graph optimisation (include/dliom.h "pose graph optimisation") ------------------------------------------------
ERR_TOO_LARGE = -14
POSE_GRAPH_MAX_REDUCED_DIMENSION = 8192


class PoseGraphOptions(C.Structure):
    _fields_ = [("fix_z_in_3d", C.c_int), ("use_nonmonotonic_steps", C.c_int), ("max_num_iterations", C.c_int),
                ("num_threads", C.c_int)]


class PoseGraphConstraint(C.Structure):
    _fields_ = [("submap", C.c_int32), ("node", C.c_int32), ("zbar", C.c_double * 7), ("translation_weight", C.c_double),
                ("rotation_weight", C.c_double)]


class PoseGraphSummary(C.Structure):
    _fields_ = CsmSummary._fields_ + [("reduced_dimension", C.c_int), ("linear_solver_failures", C.c_int),
                                      ("linearise_ms", C.c_double), ("eliminate_ms", C.c_double), ("factor_ms", C.c_double),
                                      ("back_substitute_ms", C.c_double), ("host_ms", C.c_double),
                                      ("num_recorded_steps", C.c_int), ("steps", C.c_uint8 * 256)]


POSE_GRAPH_CONSTRAINT_DTYPE = np.dtype([("submap", "<i4"), ("node", "<i4"), ("zbar", "<f8", 7), ("translation_weight", "<f8"),
                                        ("rotation_weight", "<f8")])
assert POSE_GRAPH_CONSTRAINT_DTYPE.itemsize == C.sizeof(PoseGraphConstraint)
_pgc = C.POINTER(PoseGraphConstraint)
_PG_GRAPH = [C.c_int, _f64p, _u8p, C.c_int, C.c_int, _f64p, _u8p, C.c_int64, _pgc]


class PoseGraphTerms(C.Structure):
    _fields_ = [("num_fixed_frames", C.c_int), ("fixed_frame_poses7", _f64p), ("num_fixed_frame_constraints", C.c_int64),
                ("fixed_frame_constraints", _pgc), ("huber_scale", C.c_double), ("inter_submap", _u8p)]


_pgt = C.POINTER(PoseGraphTerms)


class PoseGraphLandmarkObservation(C.Structure):
    _fields_ = [("landmark", C.c_int32), ("prev_node", C.c_int32), ("next_node", C.c_int32),
                ("interpolation_parameter", C.c_double), ("landmark_to_tracking7", C.c_double * 7),
                ("translation_weight", C.c_double), ("rotation_weight", C.c_double)]


POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE = np.dtype(
    {"names": ["landmark", "prev_node", "next_node", "interpolation_parameter", "landmark_to_tracking", "translation_weight",
               "rotation_weight"],
     "formats": ["<i4", "<i4", "<i4", "<f8", ("<f8", 7), "<f8", "<f8"], "offsets": [0, 4, 8, 16, 24, 80, 88], "itemsize": 96})
assert POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE.itemsize == C.sizeof(PoseGraphLandmarkObservation)
assert all(POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE.fields[n][1] == getattr(PoseGraphLandmarkObservation, f).offset
           for n, (f, _) in zip(POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE.names, PoseGraphLandmarkObservation._fields_))
_pglo = C.POINTER(PoseGraphLandmarkObservation)


class PoseGraphLandmarks(C.Structure):
    _fields_ = [("num_landmarks", C.c_int), ("landmark_poses7", _f64p), ("landmark_constant", _u8p),
                ("num_observations", C.c_int64), ("observations", _pglo)]


_pgl = C.POINTER(PoseGraphLandmarks)
SYMBOLS += [
    ("dliom_pose_graph_solve_landmarks", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, _pgl, C.POINTER(PoseGraphSummary)]),
    ("dliom_pose_graph_evaluate_landmarks", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, _pgl, _f64p, _f64p, _f64p]),
    ("dliom_pose_graph_step_landmarks", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, _pgl, C.c_double, _f64p, _f64p,
                                                                                                 C.POINTER(C.c_int)]),
    ("dliom_pose_graph_initial_landmark_pose", C.c_int, [_f64p, _f64p, C.c_double, _f64p, _f64p]),
]
SYMBOLS += [
    ("dliom_pose_graph_solve", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [C.POINTER(PoseGraphSummary)]),
    ("dliom_pose_graph_evaluate", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_f64p, _f64p, _f64p]),
    ("dliom_pose_graph_step", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [C.c_double, _f64p, _f64p,
                                                                                       C.POINTER(C.c_int)]),
    ("dliom_pose_graph_solve_terms", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, C.POINTER(PoseGraphSummary)]),
    ("dliom_pose_graph_evaluate_terms", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, _f64p, _f64p, _f64p]),
    ("dliom_pose_graph_step_terms", C.c_int, [_vp, C.POINTER(PoseGraphOptions)] + _PG_GRAPH + [_pgt, C.c_double, _f64p, _f64p,
                                                                                             C.POINTER(C.c_int)]),
]


def initial_landmark_pose(prev_pose, next_pose, t, landmark_to_tracking):
    """GetInitialLandmarkPose (dliom_pose_graph_initial_landmark_pose): a landmark's start value from an observation."""
    prev_pose, next_pose, z, out = _f64(prev_pose).copy(), _f64(next_pose).copy(), _f64(landmark_to_tracking).copy(), np.zeros(7)
    _check(load_library().dliom_pose_graph_initial_landmark_pose(_p(prev_pose, _f64p), _p(next_pose, _f64p), float(t),
                                                                _p(z, _f64p), _p(out, _f64p)),
           "dliom_pose_graph_initial_landmark_pose")
    return out


class PoseGraph:
    """OptimizationProblem3D::Solve on compacted indices.  submap_poses / node_poses: (n, 7) [t, q wxyz]; constraints:
    a POSE_GRAPH_CONSTRAINT_DTYPE array; *_constant: uint8 flags or None; gravity_aligned_submap: index or -1.

    The further terms (dliom_pose_graph_terms): fixed_frame_poses (F, 7), fixed_frame_constraints (their `submap` is the
    fixed frame's index), huber_scale and inter_submap (uint8 flags a constraint, or None).  entry: "plain" calls
    dliom_pose_graph_*, "null" the *_terms entry points with a NULL struct, "terms" those with the struct; None picks
    "plain" when there is no further term and "terms" otherwise.

    Landmarks (dliom_pose_graph_landmarks): landmarks (L, 7) start values, landmark_constant (uint8 flags or None) and
    landmark_observations (a POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE array).  With any of them the entry is "landmarks" (the
    *_landmarks entry points with both structs); "landmarks_null" and "landmarks_empty" call those with a NULL / an empty
    landmark struct and NULL terms, and carry no further term."""

    def __init__(self, ctx, submap_poses, node_poses, constraints, submap_constant=None, node_constant=None,
                 gravity_aligned_submap=0, fix_z_in_3d=False, use_nonmonotonic_steps=False, max_num_iterations=10,
                 fixed_frame_poses=None, fixed_frame_constraints=None, huber_scale=0.0, inter_submap=None, entry=None,
                 landmarks=None, landmark_constant=None, landmark_observations=None):
        self.ctx, self._L = ctx, ctx._L
        self.landmarks = _f64(np.zeros((0, 7)) if landmarks is None else landmarks).reshape(-1, 7).copy()
        self.landmark_constant = None if landmark_constant is None else np.ascontiguousarray(landmark_constant, dtype=np.uint8)
        self.landmark_observations = np.ascontiguousarray(
            np.zeros(0, POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE) if landmark_observations is None else landmark_observations,
            dtype=POSE_GRAPH_LANDMARK_OBSERVATION_DTYPE)
        if self.landmark_constant is not None and len(self.landmark_constant) != len(self.landmarks):
            raise ValueError("landmark_constant: one flag a landmark")
        self.submaps = _f64(submap_poses).reshape(-1, 7).copy()
        self.nodes = _f64(node_poses).reshape(-1, 7).copy()
        self.constraints = np.ascontiguousarray(constraints, dtype=POSE_GRAPH_CONSTRAINT_DTYPE)
        self.submap_constant = None if submap_constant is None else np.ascontiguousarray(submap_constant, dtype=np.uint8)
        self.node_constant = None if node_constant is None else np.ascontiguousarray(node_constant, dtype=np.uint8)
        self.gravity = int(gravity_aligned_submap)
        self.options = PoseGraphOptions(int(fix_z_in_3d), int(use_nonmonotonic_steps), int(max_num_iterations), 1)
        self.fixed_frames = _f64(np.zeros((0, 7)) if fixed_frame_poses is None else fixed_frame_poses).reshape(-1, 7).copy()
        self.fixed_frame_constraints = np.ascontiguousarray(
            np.zeros(0, POSE_GRAPH_CONSTRAINT_DTYPE) if fixed_frame_constraints is None else fixed_frame_constraints,
            dtype=POSE_GRAPH_CONSTRAINT_DTYPE)
        self.huber_scale = float(huber_scale)
        self.inter_submap = None if inter_submap is None else np.ascontiguousarray(inter_submap, dtype=np.uint8)
        if self.inter_submap is not None and len(self.inter_submap) != len(self.constraints):
            raise ValueError("inter_submap: one flag a constraint")
        plain = len(self.fixed_frames) == 0 and len(self.fixed_frame_constraints) == 0 and self.huber_scale == 0.0
        with_landmarks = len(self.landmarks) > 0 or len(self.landmark_observations) > 0
        self.entry = ("landmarks" if with_landmarks else "plain" if plain else "terms") if entry is None else entry
        if self.entry not in ("plain", "null", "terms", "landmarks", "landmarks_null", "landmarks_empty") or \
                (self.entry not in ("terms", "landmarks") and not plain) or (self.entry != "landmarks" and with_landmarks):
            raise ValueError("entry %r cannot carry the further terms" % (self.entry,))

    def _graph(self):
        u8 = lambda a: None if a is None else _p(a, _u8p)  # noqa: E731
        return (len(self.submaps), _p(self.submaps, _f64p), u8(self.submap_constant), self.gravity, len(self.nodes),
                _p(self.nodes, _f64p), u8(self.node_constant), len(self.constraints), _p(self.constraints, _pgc))

    def _call(self, name, *rest):
        """dliom_pose_graph_<name> or its _terms form, by self.entry; rest: the arguments behind the graph."""
        if self.entry == "plain":
            status = getattr(self._L, "dliom_pose_graph_" + name)(self.ctx.h, C.byref(self.options), *self._graph(), *rest)
        else:
            terms = None
            if self.entry in ("terms", "landmarks"):
                terms = C.byref(PoseGraphTerms(
                    len(self.fixed_frames), _p(self.fixed_frames, _f64p) if len(self.fixed_frames) else None,
                    len(self.fixed_frame_constraints),
                    _p(self.fixed_frame_constraints, _pgc) if len(self.fixed_frame_constraints) else None, self.huber_scale,
                    None if self.inter_submap is None else _p(self.inter_submap, _u8p)))
            if self.entry.startswith("landmarks"):
                landmarks = None
                if self.entry != "landmarks_null":
                    landmarks = C.byref(PoseGraphLandmarks(
                        len(self.landmarks), _p(self.landmarks, _f64p) if len(self.landmarks) else None,
                        None if self.landmark_constant is None else _p(self.landmark_constant, _u8p),
                        len(self.landmark_observations),
                        _p(self.landmark_observations, _pglo) if len(self.landmark_observations) else None))
                status = getattr(self._L, "dliom_pose_graph_%s_landmarks" % name)(self.ctx.h, C.byref(self.options), *self._graph(),
                                                                                  terms, landmarks, *rest)
            else:
                status = getattr(self._L, "dliom_pose_graph_%s_terms" % name)(self.ctx.h, C.byref(self.options), *self._graph(),
                                                                              terms, *rest)
        _check(status, "dliom_pose_graph_" + name)

    def evaluate(self):
        """-> (cost, residuals (C + CF + O, 6), gradient (S + N + F + L, 6)): the constraints, the fixed frames' and then the
        observations; the submaps, the nodes, the fixed frames and then the landmarks"""
        cost = C.c_double()
        r = np.zeros((len(self.constraints) + len(self.fixed_frame_constraints) + len(self.landmark_observations), 6))
        g = np.zeros((len(self.submaps) + len(self.nodes) + len(self.fixed_frames) + len(self.landmarks), 6))
        self._call("evaluate", C.byref(cost), _p(r, _f64p), _p(g, _f64p))
        return cost.value, r, g

    def step(self, radius=1e4):
        """-> (delta (S + N + F + L, 6), model_cost_change, reduced_dimension)"""
        d = np.zeros((len(self.submaps) + len(self.nodes) + len(self.fixed_frames) + len(self.landmarks), 6))
        m, n = C.c_double(), C.c_int()
        self._call("step", float(radius), _p(d, _f64p), C.byref(m), C.byref(n))
        return d, m.value, n.value

    def solve(self):
        """Overwrites self.submaps / self.nodes / self.fixed_frames / self.landmarks with the best iterate -> the summary as a dict (steps:
        list of 1 / 0 / 2)."""
        s = PoseGraphSummary()
        self._call("solve", C.byref(s))
        out = {k: getattr(s, k) for k, _ in PoseGraphSummary._fields_ if k not in ("steps", "num_recorded_steps")}
        out["steps"] = list(s.steps[:s.num_recorded_steps])
        return out


# ---- submap feature matching (include/dliom.h "submap feature matching") ---------------------------------------------------
FEATURE_RANSAC_HYPOTHESES, FEATURE_MAX_GOOD, FEATURE_TRAIN_CHUNK, FEATURE_MAX_TRAIN_SETS = 2000, 4096, 64, 8192
FEATURE_MATCHED, FEATURE_TOO_FEW_KEYPOINTS, FEATURE_TOO_FEW_GOOD_MATCHES, FEATURE_NO_MODEL, FEATURE_SCALE_REJECTED = range(5)


class FeatureMatchOptions(C.Structure):
    _fields_ = [("good_match_ratio_of_distance", C.c_double), ("minimum_good_match_num", C.c_int), ("reserved", C.c_int),
                ("ransac_threshold", C.c_double), ("scale_estimated_tolerance", C.c_double), ("seed", C.c_uint64)]


class SubmapMatch(C.Structure):
    _fields_ = [("key", C.c_int64), ("status", C.c_int), ("good_matches", C.c_int), ("inliers", C.c_int),
                ("hypothesis", C.c_int)] + [(f, C.c_double) for f in ("a", "b", "tx", "ty", "scale", "theta")]


class FeatureMatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("pairs", "matched", "too_few_keypoints", "too_few_good_matches", "no_model",
                                         "scale_rejected", "over_capacity", "ransac_pairs", "read_backs")] + \
               [(f, C.c_double) for f in ("knn_ms", "good_ms", "ransac_ms")]


class FeatureRansacResult(C.Structure):
    _fields_ = [("status", C.c_int), ("inliers", C.c_int), ("hypothesis", C.c_int), ("num_hypotheses", C.c_int)] + \
               [(f, C.c_double) for f in ("a", "b", "tx", "ty", "scale", "theta")]


class FeatureIndexMemory(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("sets", "keypoints", "descriptor_bytes", "keypoint_bytes", "scratch_bytes")]


SUBMAP_MATCH_DTYPE = np.dtype([("key", "<i8"), ("status", "<i4"), ("good_matches", "<i4"), ("inliers", "<i4"),
                               ("hypothesis", "<i4"), ("a", "<f8"), ("b", "<f8"), ("tx", "<f8"), ("ty", "<f8"),
                               ("scale", "<f8"), ("theta", "<f8")])
assert SUBMAP_MATCH_DTYPE.itemsize == C.sizeof(SubmapMatch)
SYMBOLS += [
    ("dliom_feature_index_create", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("dliom_feature_index_destroy", None, [_vp]),
    ("dliom_feature_index_size", C.c_int, [_vp, _i64p]),
    ("dliom_feature_index_memory_stats", C.c_int, [_vp, C.POINTER(FeatureIndexMemory)]),
    ("dliom_feature_index_add", C.c_int, [_vp, C.c_int64, _f32p, _f32p, C.c_int32, C.c_double, C.c_double, C.c_double]),
    ("dliom_feature_index_remove", C.c_int, [_vp, C.c_int64]),
    ("dliom_feature_index_match", C.c_int, [_vp, C.c_int64, _i64p, C.c_int, C.POINTER(FeatureMatchOptions),
                                            C.POINTER(SubmapMatch), C.POINTER(FeatureMatchStats)]),
    ("dliom_feature_index_knn", C.c_int, [_vp, C.c_int64, C.c_int64, _i32p, _i32p, _f32p, _f32p]),
    ("dliom_feature_ransac", C.c_int, [_vp, _f32p, _f32p, C.c_int, C.c_double, C.c_uint64, C.POINTER(FeatureRansacResult),
                                       _u8p]),
]


def feature_match_options(good_match_ratio_of_distance, minimum_good_match_num, ransac_threshold, scale_estimated_tolerance,
                          seed=0):
    return FeatureMatchOptions(float(good_match_ratio_of_distance), int(minimum_good_match_num), 0, float(ransac_threshold),
                               float(scale_estimated_tolerance), int(seed))


class FeatureIndex:
    """The key points and descriptors of the finished submaps in HBM (dliom_feature_index) and the second half of
    ConstraintBuilder3D::ExtractFeaturesForSubmap on them.  Parity unpinned against OpenCV (dliom.h)."""

    def __init__(self, ctx, descriptor_size):
        self.ctx, self._L = ctx, ctx._L
        h = _vp()
        _check(self._L.dliom_feature_index_create(ctx.h, int(descriptor_size), C.byref(h)), "dliom_feature_index_create")
        self.h, self.descriptor_size = h, int(descriptor_size)

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_feature_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_int64()
        _check(self._L.dliom_feature_index_size(self.h, C.byref(n)), "dliom_feature_index_size")
        return int(n.value)

    def memory_stats(self):
        m = FeatureIndexMemory()
        _check(self._L.dliom_feature_index_memory_stats(self.h, C.byref(m)), "dliom_feature_index_memory_stats")
        return {k: getattr(m, k) for k, _ in FeatureIndexMemory._fields_}

    def add(self, key, descriptors, keypoints_xy, ox, oy, resolution):
        d = _f32(descriptors).reshape(-1, self.descriptor_size)
        k = _f32(keypoints_xy).reshape(-1, 2)
        if len(d) != len(k):
            raise ValueError("one descriptor a key point")
        _check(self._L.dliom_feature_index_add(self.h, int(key), _p(d, _f32p), _p(k, _f32p), len(d), float(ox), float(oy),
                                               float(resolution)), "dliom_feature_index_add")

    def add_from_grid(self, key, grid, pose, options):
        """dliom_feature_index_add_from_grid: project, binarise, erode, detect, describe and store, all in HBM (options:
        surf_options()) -> (count, ox, oy, resolution)"""
        p = _f64(pose)
        n, ox, oy, res = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        _check(self._L.dliom_feature_index_add_from_grid(self.h, int(key), grid.h, _p(p, _f64p), C.byref(options), C.byref(n),
                                                         C.byref(ox), C.byref(oy), C.byref(res)),
               "dliom_feature_index_add_from_grid")
        return int(n.value), ox.value, oy.value, res.value

    def remove(self, key):
        _check(self._L.dliom_feature_index_remove(self.h, int(key)), "dliom_feature_index_remove")

    def match(self, query_key, train_keys, options):
        """-> (results: a SUBMAP_MATCH_DTYPE array, one a train key; stats: dict)"""
        keys = np.ascontiguousarray(train_keys, dtype=np.int64)
        results = np.zeros(len(keys), dtype=SUBMAP_MATCH_DTYPE)
        stats = FeatureMatchStats()
        _check(self._L.dliom_feature_index_match(self.h, int(query_key), _p(keys, _i64p), len(keys), C.byref(options),
                                                 _p(results, C.POINTER(SubmapMatch)), C.byref(stats)),
               "dliom_feature_index_match")
        return results, {k: getattr(stats, k) for k, _ in FeatureMatchStats._fields_}

    def knn(self, query_key, train_key, num_queries):
        """-> (j0, j1, d0, d1) of the query set's num_queries key points"""
        j0, j1 = np.zeros(num_queries, np.int32), np.zeros(num_queries, np.int32)
        d0, d1 = np.zeros(num_queries, np.float32), np.zeros(num_queries, np.float32)
        _check(self._L.dliom_feature_index_knn(self.h, int(query_key), int(train_key), _p(j0, _i32p), _p(j1, _i32p),
                                               _p(d0, _f32p), _p(d1, _f32p)), "dliom_feature_index_knn")
        return j0, j1, d0, d1


def feature_ransac(ctx, from_xy, to_xy, threshold, seed=0):
    """dliom_feature_ransac -> (dict of the result's fields, inlier mask (M,) uint8)"""
    p, q = _f32(from_xy).reshape(-1, 2), _f32(to_xy).reshape(-1, 2)
    if len(p) != len(q):
        raise ValueError("one `to` point a `from` point")
    r, mask = FeatureRansacResult(), np.zeros(len(p), np.uint8)
    _check(ctx._L.dliom_feature_ransac(ctx.h, _p(p, _f32p), _p(q, _f32p), len(p), float(threshold), int(seed), C.byref(r),
                                       _p(mask, _u8p)), "dliom_feature_ransac")
    return {k: getattr(r, k) for k, _ in FeatureRansacResult._fields_}, mask


# ---- submap image features (dliom.h "submap image features") ------------------------------------------------------------
class SurfOptions(C.Structure):
    _fields_ = [("binary_threshold", C.c_int), ("structure_element_size", C.c_int), ("hessian_threshold", C.c_double),
                ("n_octaves", C.c_int), ("n_octave_layers", C.c_int), ("extended", C.c_int), ("upright", C.c_int)]


SURF_MAX_PIXELS, SURF_MAX_KEYPOINTS, SURF_MAX_STRUCTURE_ELEMENT = 1 << 23, 65536, 33
SURF_DESCRIPTOR_SIZE, SURF_KEYPOINT_FLOATS = 64, 7
SYMBOLS += [
    ("dliom_surf_default_options", SurfOptions, []),
    ("dliom_image_binarize_erode", C.c_int, [_vp, _u8p, C.c_int32, C.c_int32, C.POINTER(SurfOptions), _u8p]),
    ("dliom_surf_layer", C.c_int, [_vp, _u8p, C.c_int32, C.c_int32, C.c_int, C.c_int, _f32p, _f32p, _i32p, _i32p]),
    ("dliom_surf_detect_and_compute", C.c_int, [_vp, _u8p, C.c_int32, C.c_int32, C.POINTER(SurfOptions), _f32p, _f32p,
                                                C.c_int32, _i32p]),
    ("dliom_feature_index_add_from_grid", C.c_int, [_vp, C.c_int64, _vp, _f64p, C.POINTER(SurfOptions), _i32p, _f64p, _f64p,
                                                    _f64p]),
]


def surf_options(binary_threshold=200, structure_element_size=3, hessian_threshold=400.0, n_octaves=4, n_octave_layers=3,
                 extended=0, upright=0):
    """dliom_surf_options; the defaults are dliom_surf_default_options()'s (pose_graph.lua:27-28, constraint_builder_3d.h:206)"""
    return SurfOptions(int(binary_threshold), int(structure_element_size), float(hessian_threshold), int(n_octaves),
                       int(n_octave_layers), int(extended), int(upright))


def _image(image):
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim != 2:
        raise ValueError("an image is (height, width) bytes")
    return img


def image_binarize_erode(ctx, image, options):
    """dliom_image_binarize_erode -> the eroded image (height, width) uint8"""
    img = _image(image)
    out = np.zeros_like(img)
    _check(ctx._L.dliom_image_binarize_erode(ctx.h, _p(img, _u8p), img.shape[1], img.shape[0], C.byref(options), _p(out, _u8p)),
           "dliom_image_binarize_erode")
    return out


def surf_layer(ctx, image, octave, layer):
    """dliom_surf_layer -> (det, trace), each (rows, cols) float32"""
    img = _image(image)
    rows, cols = C.c_int32(), C.c_int32()
    args = (ctx.h, _p(img, _u8p), img.shape[1], img.shape[0], int(octave), int(layer))
    _check(ctx._L.dliom_surf_layer(*args, None, None, C.byref(rows), C.byref(cols)), "dliom_surf_layer")
    det, trace = np.zeros((rows.value, cols.value), np.float32), np.zeros((rows.value, cols.value), np.float32)
    if det.size:
        _check(ctx._L.dliom_surf_layer(*args, _p(det, _f32p), _p(trace, _f32p), C.byref(rows), C.byref(cols)), "dliom_surf_layer")
    return det, trace


def surf_detect_and_compute(ctx, image, options, capacity=None):
    """dliom_surf_detect_and_compute -> (keypoints (n, 7) float32: x, y, size, angle, response, octave, laplacian sign;
    descriptors (n, 64) float32).  capacity None: the size query first."""
    img = _image(image)
    n = C.c_int32()
    args = (ctx.h, _p(img, _u8p), img.shape[1], img.shape[0], C.byref(options))
    if capacity is None:
        _check(ctx._L.dliom_surf_detect_and_compute(*args, None, None, 0, C.byref(n)), "dliom_surf_detect_and_compute")
        capacity = n.value
    kp = np.zeros((capacity, SURF_KEYPOINT_FLOATS), np.float32)
    desc = np.zeros((capacity, SURF_DESCRIPTOR_SIZE), np.float32)
    _check(ctx._L.dliom_surf_detect_and_compute(*args, _p(kp, _f32p), _p(desc, _f32p), capacity, C.byref(n)),
           "dliom_surf_detect_and_compute")
    return kp[:n.value], desc[:n.value]


# ---- painting submap slices into one map (dliom.h "painting submap slices into one map") -------------------------------
class SubmapSliceDescription(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("resolution", C.c_double), ("slice_pose7", C.c_double * 7),
                ("pose7", C.c_double * 7)]


class SubmapPainterStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("texels_uploaded", C.c_int64), ("tile_slice_pairs", C.c_int64)]


SUBMAP_PAINTER_TILE, SUBMAP_PAINTER_MAX_PAIRS = 16, 1 << 30
_i8p = C.POINTER(C.c_int8)
_slicep = C.POINTER(SubmapSliceDescription)
SYMBOLS += [
    ("dliom_submap_slice_create", C.c_int, [_vp, _u8p, C.c_int32, C.c_int32, C.c_double, _f64p, _f64p, C.POINTER(_vp)]),
    ("dliom_submap_slice_create_from_grid", C.c_int, [_vp, _f64p, C.POINTER(_vp)]),
    ("dliom_submap_slice_set_pose", C.c_int, [_vp, _f64p]),
    ("dliom_submap_slice_info", C.c_int, [_vp, _slicep]),
    ("dliom_submap_slice_destroy", C.c_int, [_vp]),
    ("dliom_submap_slices_layout", C.c_int, [_slicep, C.c_int64, C.c_double, _i32p, _i32p, _f32p, _i64p]),
    ("dliom_submap_occupancy_table", C.c_int, [_i8p]),
    ("dliom_submap_slices_paint", C.c_int, [_vp, C.POINTER(_vp), C.c_int64, C.c_double, _u32p, C.c_int64, _i32p, _i32p, _f32p]),
    ("dliom_submap_slices_occupancy", C.c_int, [_vp, C.POINTER(_vp), C.c_int64, C.c_double, _i8p, C.c_int64, _i32p, _i32p,
                                                _f32p, _f64p]),
    ("dliom_ctx_submap_painter_stats", C.c_int, [_vp, C.POINTER(SubmapPainterStats)]),
]


def submap_slice_description(width, height, resolution, slice_pose, pose):
    return SubmapSliceDescription(int(width), int(height), float(resolution), (C.c_double * 7)(*_pose7(slice_pose)),
                                  (C.c_double * 7)(*_pose7(pose)))


def submap_slices_layout(descriptions, resolution):
    """dliom_submap_slices_layout (host only) -> (status, width, height, origin float32[2], fixed int64 (n, 6): A B E C D G);
    the status is returned, not raised: the sizes are filled under ERR_CAPACITY too."""
    n = len(descriptions)
    arr = (SubmapSliceDescription * max(n, 1))(*descriptions)
    w, h = C.c_int32(), C.c_int32()
    origin, fixed = np.zeros(2, np.float32), np.zeros((n, 6), np.int64)
    status = load_library().dliom_submap_slices_layout(arr if n else None, n, float(resolution), C.byref(w), C.byref(h),
                                                       _p(origin, _f32p), _p(fixed, _i64p))
    return status, w.value, h.value, origin, fixed


def submap_occupancy_table():
    out = np.zeros(256, np.int8)
    _check(load_library().dliom_submap_occupancy_table(_p(out, _i8p)), "dliom_submap_occupancy_table")
    return out


class SubmapSlice:
    """io::SubmapSlice with its texture in HBM (dliom_submap_slice).  SubmapSlice(ctx, cells, resolution, slice_pose, pose)
    uploads (height, width, 2) uint8 (intensity, alpha); SubmapSlice.from_grid(grid, global_submap_pose) is FillSubmapSlice."""

    def __init__(self, ctx, cells, resolution, slice_pose, pose, _handle=None):
        self._L = ctx._L
        self.ctx = ctx
        if _handle is not None:
            self.h = _handle
            return
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        if cells.ndim != 3 or cells.shape[2] != 2:
            raise ValueError("cells are (height, width, 2) bytes: intensity, alpha")
        h = _vp()
        _check(self._L.dliom_submap_slice_create(ctx.h, _p(cells, _u8p) if cells.size else None, cells.shape[1], cells.shape[0],
                                                 float(resolution), _p(_pose7(slice_pose), _f64p), _p(_pose7(pose), _f64p),
                                                 C.byref(h)), "dliom_submap_slice_create")
        self.h = h

    @classmethod
    def from_grid(cls, grid, global_submap_pose):
        h = _vp()
        _check(grid._L.dliom_submap_slice_create_from_grid(grid.h, _p(_pose7(global_submap_pose), _f64p), C.byref(h)),
               "dliom_submap_slice_create_from_grid")
        return cls(grid.ctx, None, 0.0, None, None, _handle=h)

    def set_pose(self, pose):
        _check(self._L.dliom_submap_slice_set_pose(self.h, _p(_pose7(pose), _f64p)), "dliom_submap_slice_set_pose")

    def info(self):
        d = SubmapSliceDescription()
        _check(self._L.dliom_submap_slice_info(self.h, C.byref(d)), "dliom_submap_slice_info")
        return d

    def close(self):
        if self.h is not None:
            self._L.dliom_submap_slice_destroy(self.h)
            self.h = None


def _slice_handles(slices):
    return (_vp * max(len(slices), 1))(*[s.h for s in slices])


def paint_submap_slices(ctx, slices, resolution):
    """io::PaintSubmapSlices on the device -> (pixels (height, width) uint32 ARGB, origin float32[2])"""
    hs, n = _slice_handles(slices), len(slices)
    w, h, origin = C.c_int32(), C.c_int32(), np.zeros(2, np.float32)
    _check(ctx._L.dliom_submap_slices_paint(ctx.h, hs, n, float(resolution), None, 0, C.byref(w), C.byref(h), _p(origin, _f32p)),
           "dliom_submap_slices_paint")
    pixels = np.zeros((h.value, w.value), np.uint32)
    _check(ctx._L.dliom_submap_slices_paint(ctx.h, hs, n, float(resolution), _p(pixels, _u32p), pixels.size, C.byref(w),
                                            C.byref(h), _p(origin, _f32p)), "dliom_submap_slices_paint")
    return pixels, origin


def submap_slices_occupancy(ctx, slices, resolution):
    """PaintSubmapSlices + CreateOccupancyGridMsg's cells -> (data (height, width) int8, origin_xy float64[2])"""
    hs, n = _slice_handles(slices), len(slices)
    w, h, origin_xy = C.c_int32(), C.c_int32(), np.zeros(2, np.float64)
    _check(ctx._L.dliom_submap_slices_occupancy(ctx.h, hs, n, float(resolution), None, 0, C.byref(w), C.byref(h), None,
                                                _p(origin_xy, _f64p)), "dliom_submap_slices_occupancy")
    data = np.zeros((h.value, w.value), np.int8)
    _check(ctx._L.dliom_submap_slices_occupancy(ctx.h, hs, n, float(resolution), _p(data, _i8p), data.size, C.byref(w),
                                                C.byref(h), None, _p(origin_xy, _f64p)), "dliom_submap_slices_occupancy")
    return data, origin_xy


def submap_painter_stats(ctx):
    s = SubmapPainterStats()
    _check(ctx._L.dliom_ctx_submap_painter_stats(ctx.h, C.byref(s)), "dliom_ctx_submap_painter_stats")
    return {k: getattr(s, k) for k, _ in SubmapPainterStats._fields_}


# ---- PointCloud2 messages decoded on the device (dliom.h "PointCloud2 messages decoded on the device") ----------------
POINT_FIELD_INT8, POINT_FIELD_UINT8, POINT_FIELD_INT16, POINT_FIELD_UINT16 = 1, 2, 3, 4
POINT_FIELD_INT32, POINT_FIELD_UINT32, POINT_FIELD_FLOAT32, POINT_FIELD_FLOAT64 = 5, 6, 7, 8
POINT_CLOUD2_SLAM_OUSTER, POINT_CLOUD2_SLAM_VELODYNE, POINT_CLOUD2_SLAM_ROBOSENSE, POINT_CLOUD2_SLAM_OTHER = 0, 1, 2, 3
POINT_CLOUD2_EXPORT, POINT_CLOUD2_EXPORT_RSLIDAR = 4, 5


class PointField(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("datatype", C.c_uint32), ("count", C.c_uint32)]


class PointCloud2Struct(C.Structure):
    _fields_ = [("height", C.c_uint32), ("width", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("is_bigendian", C.c_uint32), ("num_fields", C.c_int32), ("fields", C.POINTER(PointField)),
                ("data", C.c_void_p), ("data_size", C.c_uint64), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32)]


_pc2p = C.POINTER(PointCloud2Struct)
SYMBOLS += [
    ("dliom_point_cloud2_check", C.c_int, [_pc2p, C.c_int, _i64p, _f64p]),
    ("dliom_point_cloud2_decode", C.c_int, [_vp, _pc2p, C.c_int, _f64p, C.POINTER(_vp), _i64p, _f32p]),
    ("dliom_timed_cloud_destroy", C.c_int, [_vp]),
    ("dliom_timed_cloud_size", C.c_int, [_vp, _i64p]),
    ("dliom_timed_cloud_has_intensities", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_timed_cloud_front_back_time", C.c_int, [_vp, _f32p, _f32p]),
    ("dliom_timed_cloud_download", C.c_int, [_vp, _f32p, _f32p]),
    ("dliom_add_range_data_timed_cloud", C.c_int, [_vp, _f64p, _f64p, C.c_double, _vp, _f32p, C.c_float, C.c_float, C.c_float,
                                                   C.POINTER(_vp), _f32p, _f32p]),
    ("dliom_points_batch_from_timed_cloud", C.c_int, [_vp, _vp, C.c_int64, _vp, _f64p, C.POINTER(_vp)]),
    # two range sensors' clouds merged on the device (range_sync.hip)
    ("dliom_timed_cloud_has_origin_index", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("dliom_timed_cloud_download_origin_index", C.c_int, [_vp, _f32p]),
    ("dliom_timed_cloud_stamp", C.c_int, [_vp, _vp, C.c_double, C.POINTER(_vp)]),
    ("dliom_timed_clouds_merge", C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(_vp)]),
    ("dliom_range_accumulator_add_timed_cloud", C.c_int, [_vp, _f64p, _f64p, C.c_double, _vp, _f32p, C.c_int, C.c_float, C.c_float,
                                                          C.c_float, _f32p, C.POINTER(C.c_int)]),
]


class PointCloud2:
    """sensor_msgs/PointCloud2 as the library takes it: fields is a list of (name, offset, datatype, count); data any
    uint8 array (a view at any byte offset will do: nothing needs to be aligned), kept alive by this object."""

    def __init__(self, height, width, point_step, row_step, fields, data, stamp_sec=0, stamp_nsec=0, is_bigendian=0,
                 data_size=None):
        self.data = np.asarray(data, dtype=np.uint8)
        if self.data.ndim != 1 or (self.data.size > 1 and self.data.strides[0] != 1):
            raise ValueError("data is a one-dimensional run of bytes")
        self.fields = [(str(name), int(offset), int(datatype), int(count)) for name, offset, datatype, count in fields]
        self._table = (PointField * max(len(self.fields), 1))(*[PointField(name.encode(), offset, datatype, count)
                                                                 for name, offset, datatype, count in self.fields])
        self.struct = PointCloud2Struct(int(height), int(width), int(point_step), int(row_step), int(is_bigendian), len(self.fields),
                                        self._table if self.fields else None, self.data.ctypes.data if self.data.size else None,
                                        self.data.size if data_size is None else int(data_size), int(stamp_sec), int(stamp_nsec))

    def check(self, mode):
        """dliom_point_cloud2_check (host only) -> (status, time, rel_time_last); the status is returned, not raised."""
        time, rel = C.c_int64(), C.c_double()
        status = load_library().dliom_point_cloud2_check(C.byref(self.struct), int(mode), C.byref(time), C.byref(rel))
        return status, time.value, rel.value

    def decode(self, ctx, mode, sensor_to_tracking=None):
        """dliom_point_cloud2_decode -> (TimedCloud, time, origin float32[3])"""
        h, time, origin = _vp(), C.c_int64(), np.zeros(3, np.float32)
        _check(ctx._L.dliom_point_cloud2_decode(ctx.h, C.byref(self.struct), int(mode),
                                                None if sensor_to_tracking is None else _p(_f64(sensor_to_tracking), _f64p),
                                                C.byref(h), C.byref(time), _p(origin, _f32p)), "dliom_point_cloud2_decode")
        return TimedCloud(ctx, h), time.value, origin


class TimedCloud:
    """A decoded message in HBM (dliom_timed_cloud): packed (x, y, z, t) and, in the export modes, one intensity a point."""

    def __init__(self, ctx, handle):
        self._L, self.ctx, self.h = ctx._L, ctx, handle

    def __len__(self):
        n = C.c_int64()
        _check(self._L.dliom_timed_cloud_size(self.h, C.byref(n)), "dliom_timed_cloud_size")
        return int(n.value)

    @property
    def has_intensities(self):
        v = C.c_int()
        _check(self._L.dliom_timed_cloud_has_intensities(self.h, C.byref(v)), "dliom_timed_cloud_has_intensities")
        return bool(v.value)

    def front_back_time(self):
        t = np.zeros(2, np.float32)
        _check(self._L.dliom_timed_cloud_front_back_time(self.h, _p(t[:1], _f32p), _p(t[1:], _f32p)),
               "dliom_timed_cloud_front_back_time")
        return t[0], t[1]

    def download(self):
        """-> (xyzt float32 (n, 4), intensities float32 (n,) or None)"""
        n = len(self)
        xyzt = np.zeros((n, 4), np.float32)
        it = np.zeros(n, np.float32) if self.has_intensities else None
        _check(self._L.dliom_timed_cloud_download(self.h, _p(xyzt, _f32p), None if it is None else _p(it, _f32p)),
               "dliom_timed_cloud_download")
        return xyzt, it

    def add_range_data(self, prev_pose, predicted_pose, scan_period, origin, min_range, max_range, voxel_filter_size):
        """dliom_add_range_data_timed_cloud: add_range_data() with the ranges taken from this object.
        Returns (PointCloud returns_in_tracking, origin_in_tracking, current_pose)."""
        h = _vp()
        o = np.zeros(3, dtype=np.float32)
        cur = np.zeros(7, dtype=np.float32)
        _check(self._L.dliom_add_range_data_timed_cloud(self.ctx.h, _p(_f64(prev_pose), _f64p), _p(_f64(predicted_pose), _f64p),
                                                        scan_period, self.h, _p(_f32(origin), _f32p), C.c_float(min_range),
                                                        C.c_float(max_range), C.c_float(voxel_filter_size), C.byref(h),
                                                        _p(o, _f32p), _p(cur, _f32p)), "dliom_add_range_data_timed_cloud")
        return PointCloud(self.ctx, _handle=h), o, cur

    def to_points_batch(self, trajectory, cloud_time, sensor_to_tracking):
        """dliom_points_batch_from_timed_cloud -> PointsBatch, or None when no point is kept."""
        h = _vp()
        _check(self._L.dliom_points_batch_from_timed_cloud(self.ctx.h, trajectory.h, int(cloud_time), self.h,
                                                           _p(_f64(sensor_to_tracking), _f64p), C.byref(h)),
               "dliom_points_batch_from_timed_cloud")
        return PointsBatch(self.ctx, _handle=h) if h else None

    @property
    def has_origin_index(self):
        v = C.c_int()
        _check(self._L.dliom_timed_cloud_has_origin_index(self.h, C.byref(v)), "dliom_timed_cloud_has_origin_index")
        return bool(v.value)

    def download_origin_index(self):
        """-> float32 (n,): the origin index of every point of a merge's result"""
        oi = np.zeros(len(self), np.float32)
        _check(self._L.dliom_timed_cloud_download_origin_index(self.h, _p(oi, _f32p)), "dliom_timed_cloud_download_origin_index")
        return oi

    def stamp(self, scan_period):
        """dliom_timed_cloud_stamp (StampRangeData) -> TimedCloud"""
        h = _vp()
        _check(self._L.dliom_timed_cloud_stamp(self.ctx.h, self.h, float(scan_period), C.byref(h)), "dliom_timed_cloud_stamp")
        return TimedCloud(self.ctx, h)

    def close(self):
        if self.h is not None:
            self._L.dliom_timed_cloud_destroy(self.h)
            self.h = None


def merge_timed_clouds(ctx, primary, primary_time, secondary, secondary_time, primary_for_times=None):
    """dliom_timed_clouds_merge: the prior lidar's cloud with the overlapping part of the secondary's merged in, in
    std::sort's order of the times -> TimedCloud with the origin-index channel.  primary_for_times: the stamped copy of
    `primary` under manual de-skew."""
    h = _vp()
    _check(ctx._L.dliom_timed_clouds_merge(ctx.h, primary.h, None if primary_for_times is None else primary_for_times.h,
                                           int(primary_time), secondary.h, int(secondary_time), C.byref(h)),
           "dliom_timed_clouds_merge")
    return TimedCloud(ctx, h)


# ---- scan alignment by ICP, exact nearest neighbours (include/dliom.h "scan alignment by ICP") ---------------------------
NN_MAX_SHELLS, NN_MAX_CELLS_PER_AXIS, NN_MAX_CELLS, NN_MAX_POINTS = 3, 1024, 1 << 22, 1 << 24
ICP_JACOBI_SWEEPS, ICP_TREE_MIN_LEAVES = 12, 2048
NN_AUTO, NN_BRUTE_FORCE = 0, 1
ICP_NOT_CONVERGED, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES = range(6)


class NnIndexOptions(C.Structure):
    _fields_ = [("cell_edge", C.c_double), ("search", C.c_int), ("reserved", C.c_int)]


class NnQueryStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("queries", "non_finite", "settled_by_grid", "settled_by_brute_force", "read_backs")] + \
               [("search_ms", C.c_double)]


class NnIndexMemory(C.Structure):
    _fields_ = [("points", C.c_int64), ("finite_points", C.c_int64), ("cells", C.c_int64), ("dims", C.c_int64 * 3),
                ("index_bytes", C.c_int64), ("scratch_bytes", C.c_int64), ("cell_edge", C.c_double)]


class IcpOptions(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("max_correspondence_distance", "transformation_epsilon", "euclidean_fitness_epsilon",
                                          "rotation_epsilon", "relative_mse_epsilon")] + \
               [(f, C.c_int) for f in ("maximum_iterations", "min_correspondences", "search", "reserved")]


class IcpResult(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("converged", "reason", "iterations", "correspondences")] + \
               [("transform", C.c_double * 16), ("mse", C.c_double), ("fitness_score", C.c_double)] + \
               [(f, C.c_int64) for f in ("fitness_count", "read_backs", "settled_by_grid", "settled_by_brute_force")] + \
               [(f, C.c_double) for f in ("search_ms", "reduce_ms", "solve_ms", "transform_ms")]


SYMBOLS += [
    ("dliom_nn_index_create", C.c_int, [_vp, _vp, C.POINTER(NnIndexOptions), C.POINTER(_vp)]),
    ("dliom_nn_index_destroy", None, [_vp]),
    ("dliom_nn_index_memory_stats", C.c_int, [_vp, C.POINTER(NnIndexMemory)]),
    ("dliom_nn_index_query", C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_int, _i32p, _f32p, C.POINTER(NnQueryStats)]),
    ("dliom_icp_default_options", C.c_int, [C.POINTER(IcpOptions)]),
    ("dliom_icp_align", C.c_int, [_vp, _vp, _f64p, C.POINTER(IcpOptions), C.POINTER(IcpResult), C.POINTER(_vp)]),
    ("dliom_icp_step", C.c_int, [_vp, _vp, C.POINTER(IcpOptions), _i32p, _f32p, _f64p, _i64p, _f64p, _f64p]),
]


def _as_cloud(ctx, points):
    """(cloud, made here) of a PointCloud or an (n, 3) array"""
    if isinstance(points, PointCloud):
        return points, False
    return PointCloud(ctx, points), True


def icp_options(**overrides):
    """dliom_icp_default_options (the ground-truth tool's values) with fields replaced"""
    o = IcpOptions()
    _check(load_library().dliom_icp_default_options(C.byref(o)), "dliom_icp_default_options")
    for k, v in overrides.items():
        if k not in dict(IcpOptions._fields_):
            raise TypeError("no ICP option " + k)
        setattr(o, k, v)
    return o


def ground_truth_icp_options():
    """gen_ground_truth_by_ndt_match.cc:192-196"""
    return icp_options()


def match_by_icp_options():
    """LocalTrajectoryBuilder3D::MatchByICP, local_trajectory_builder_3d.cc:942-946: the same with 3 m"""
    return icp_options(max_correspondence_distance=3.0)


class NnIndex:
    """Exact nearest neighbours of 3-D points in HBM (dliom_nn_index): a cell grid over the target and a brute-force
    scan that give the same (j, d2) bits (dliom.h)."""

    def __init__(self, ctx, target, cell_edge=0.0, search=NN_AUTO):
        self.ctx, self._L = ctx, ctx._L
        cloud, mine = _as_cloud(ctx, target)
        h, o = _vp(), NnIndexOptions(float(cell_edge), int(search), 0)
        try:
            _check(self._L.dliom_nn_index_create(ctx.h, cloud.h, C.byref(o), C.byref(h)), "dliom_nn_index_create")
        finally:
            if mine:
                cloud.close()
        self.h = h

    @classmethod
    def _adopt(cls, ctx, handle):
        """an index that a batched build made (nn_indices_batch)"""
        index = cls.__new__(cls)
        index.ctx, index._L, index.h = ctx, ctx._L, handle
        return index

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_nn_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory_stats(self):
        m = NnIndexMemory()
        _check(self._L.dliom_nn_index_memory_stats(self.h, C.byref(m)), "dliom_nn_index_memory_stats")
        return {k: (list(getattr(m, k)) if k == "dims" else getattr(m, k)) for k, _ in NnIndexMemory._fields_}

    def query(self, queries, max_distance=np.inf, transform=None, search=NN_AUTO):
        """-> (j int32 (-1: none), d2 float32 (+inf: none), stats dict)"""
        cloud, mine = _as_cloud(self.ctx, queries)
        try:
            j, d2, st = np.zeros(max(cloud.n, 1), np.int32), np.zeros(max(cloud.n, 1), np.float32), NnQueryStats()
            t = None if transform is None else _f64(transform).reshape(16)
            _check(self._L.dliom_nn_index_query(self.h, cloud.h, None if t is None else _p(t, _f64p), float(max_distance),
                                                int(search), _p(j, _i32p), _p(d2, _f32p), C.byref(st)), "dliom_nn_index_query")
            return j[:cloud.n], d2[:cloud.n], {k: getattr(st, k) for k, _ in NnQueryStats._fields_}
        finally:
            if mine:
                cloud.close()


# many indices in one call (dliom_nn_index_create_batch): the K distinct target scans of the ground-truth tool's loop in
# one device chain a chunk
NN_INDEX_BATCH_MAX_INDICES = 256


class NnIndexBatchLimits(C.Structure):
    _fields_ = [("max_indices_in_flight", C.c_int), ("reserved", C.c_int), ("max_points_in_flight", C.c_int64),
                ("max_cells_in_flight", C.c_int64)]


class NnIndexBatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("indices", "chunks", "cell_runs", "points", "finite_points", "cells", "read_backs",
                                         "synchronizations", "max_in_flight", "scratch_bytes")] + \
               [(f, C.c_double) for f in ("box_ms", "sort_ms", "alloc_ms")]


SYMBOLS += [
    ("dliom_nn_index_batch_default_limits", C.c_int, [C.POINTER(NnIndexBatchLimits)]),
    ("dliom_nn_index_create_batch", C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(NnIndexOptions),
                                              C.POINTER(NnIndexBatchLimits), C.POINTER(_vp), C.POINTER(NnIndexBatchStats)]),
]


def nn_index_batch_default_limits(**overrides):
    """dliom_nn_index_batch_default_limits, with fields replaced"""
    lim = NnIndexBatchLimits()
    _check(load_library().dliom_nn_index_batch_default_limits(C.byref(lim)), "dliom_nn_index_batch_default_limits")
    for k, v in overrides.items():
        if k not in dict(NnIndexBatchLimits._fields_):
            raise TypeError("no index batch limit " + k)
        setattr(lim, k, v)
    return lim


def nn_indices_batch(ctx, clouds, cell_edge=0.0, search=NN_AUTO, limits=None):
    """dliom_nn_index_create_batch.  clouds: a list of PointClouds or (n, 3) arrays, as NnIndex takes them (an array that
    is named several times is uploaded once).  -> (indices, stats): an NnIndex a cloud that answers every query bit for
    bit as NnIndex(ctx, cloud, cell_edge, search) does, each closed on its own; stats a dict."""
    L = ctx._L
    count = len(clouds)
    table, handles, made = (_vp * max(count, 1))(), (_vp * max(count, 1))(), []
    try:
        uploaded = {}
        for i, source in enumerate(clouds):
            if isinstance(source, PointCloud):
                cloud = source
            elif id(source) in uploaded:
                cloud = uploaded[id(source)]
            else:
                cloud = uploaded[id(source)] = PointCloud(ctx, source)
                made.append(cloud)
            table[i] = cloud.h
        o, stats = NnIndexOptions(float(cell_edge), int(search), 0), NnIndexBatchStats()
        _check(L.dliom_nn_index_create_batch(ctx.h, table, count, C.byref(o), None if limits is None else C.byref(limits),
                                             handles, C.byref(stats)), "dliom_nn_index_create_batch")
        indices = [NnIndex._adopt(ctx, _vp(handles[i])) for i in range(count)]
        return indices, {k: getattr(stats, k) for k, _ in NnIndexBatchStats._fields_}
    finally:
        for cloud in made:
            cloud.close()


def _icp_result(r):
    out = {k: getattr(r, k) for k, _ in IcpResult._fields_ if k != "transform"}
    out["transform"] = np.array(r.transform, dtype=np.float64).reshape(4, 4)
    return out


class Icp:
    """pcl::IterativeClosestPoint as the ground-truth tool runs it, on an NnIndex of the target (dliom_icp_align).
    Parity unpinned against PCL (dliom.h)."""

    def __init__(self, index, options=None):
        self.index, self._L = index, index._L
        self.options = options if options is not None else icp_options()

    def align(self, source, guess=None, want_aligned=False):
        """-> result dict (transform: 4x4 float64), and the aligned points (n, 3) float32 if asked for"""
        cloud, mine = _as_cloud(self.index.ctx, source)
        try:
            g = _f64(np.eye(4) if guess is None else guess).reshape(16)
            r, h = IcpResult(), _vp()
            _check(self._L.dliom_icp_align(self.index.h, cloud.h, _p(g, _f64p), C.byref(self.options), C.byref(r),
                                           C.byref(h) if want_aligned else None), "dliom_icp_align")
            if not want_aligned:
                return _icp_result(r)
            aligned = PointCloud(self.index.ctx, _handle=h)
            try:
                return _icp_result(r), aligned.download()
            finally:
                aligned.close()
        finally:
            if mine:
                cloud.close()

    def step(self, points):
        """dliom_icp_step -> dict(j, d2, sums (16,), n, R (3, 3), t (3,))"""
        cloud, mine = _as_cloud(self.index.ctx, points)
        try:
            j, d2 = np.zeros(max(cloud.n, 1), np.int32), np.zeros(max(cloud.n, 1), np.float32)
            sums, R, t, n = np.zeros(16), np.zeros(9), np.zeros(3), C.c_int64()
            _check(self._L.dliom_icp_step(self.index.h, cloud.h, C.byref(self.options), _p(j, _i32p), _p(d2, _f32p),
                                          _p(sums, _f64p), C.byref(n), _p(R, _f64p), _p(t, _f64p)), "dliom_icp_step")
            return {"j": j[:cloud.n], "d2": d2[:cloud.n], "sums": sums, "n": int(n.value), "R": R.reshape(3, 3), "t": t}
        finally:
            if mine:
                cloud.close()


# many pairs in one call (dliom_icp_align_batch): the ground-truth tool's loop over a trajectory's constraints
ICP_BATCH_MAX_PAIRS = 256


class IcpPair(C.Structure):
    _fields_ = [("index", _vp), ("source", _vp), ("guess", C.c_double * 16)]


class IcpBatchLimits(C.Structure):
    _fields_ = [("max_pairs_in_flight", C.c_int), ("reserved", C.c_int), ("max_scratch_bytes", C.c_int64)]


class IcpBatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("pairs", "chunks", "steps", "read_backs", "synchronizations", "pair_searches",
                                         "max_in_flight")] + \
               [(f, C.c_double) for f in ("search_ms", "reduce_ms", "solve_ms", "transform_ms")]


SYMBOLS += [
    ("dliom_icp_batch_default_limits", C.c_int, [C.POINTER(IcpBatchLimits)]),
    ("dliom_icp_batch_scratch_bytes", C.c_int64, [C.c_int64]),
    ("dliom_icp_align_batch", C.c_int, [_vp, C.POINTER(IcpPair), C.c_int, C.POINTER(IcpOptions), C.POINTER(IcpBatchLimits),
                                        C.POINTER(IcpResult), C.POINTER(_vp), C.POINTER(IcpBatchStats)]),
]


def icp_batch_default_limits(**overrides):
    """dliom_icp_batch_default_limits, with fields replaced"""
    lim = IcpBatchLimits()
    _check(load_library().dliom_icp_batch_default_limits(C.byref(lim)), "dliom_icp_batch_default_limits")
    for k, v in overrides.items():
        if k not in dict(IcpBatchLimits._fields_):
            raise TypeError("no ICP batch limit " + k)
        setattr(lim, k, v)
    return lim


def icp_batch_scratch_bytes(n):
    """the device scratch one pair in flight with n source points reserves (host only)"""
    return int(load_library().dliom_icp_batch_scratch_bytes(int(n)))


def icp_align_batch(ctx, pairs, options=None, limits=None, want_aligned=False):
    """dliom_icp_align_batch.  pairs: a list of (NnIndex, PointCloud or (n, 3) array, guess 4x4 or None).  -> (results,
    stats) or (results, stats, clouds): results as Icp.align gives them, pair by pair and bit for bit; stats a dict; clouds
    the aligned points, (n, 3) float32 each."""
    L = ctx._L
    options = options if options is not None else icp_options()
    count = len(pairs)
    table, made = (IcpPair * max(count, 1))(), []
    handles = (_vp * max(count, 1))()
    try:
        uploaded = {}  # one upload for an array that several pairs name
        for i, (index, source, guess) in enumerate(pairs):
            if isinstance(source, PointCloud):
                cloud = source
            elif id(source) in uploaded:
                cloud = uploaded[id(source)]
            else:
                cloud = uploaded[id(source)] = PointCloud(ctx, source)
                made.append(cloud)
            table[i].index, table[i].source = index.h, cloud.h
            table[i].guess[:] = list(_f64(np.eye(4) if guess is None else guess).reshape(16))
        results, stats = (IcpResult * max(count, 1))(), IcpBatchStats()
        _check(L.dliom_icp_align_batch(ctx.h, table, count, C.byref(options), None if limits is None else C.byref(limits),
                                       results, handles if want_aligned else None, C.byref(stats)), "dliom_icp_align_batch")
        out = [_icp_result(results[i]) for i in range(count)]
        st = {k: getattr(stats, k) for k, _ in IcpBatchStats._fields_}
        if not want_aligned:
            return out, st
        clouds = []
        for i in range(count):
            aligned = PointCloud(ctx, _handle=_vp(handles[i]))
            handles[i] = None
            try:
                clouds.append(aligned.download())
            finally:
                aligned.close()
        return out, st, clouds
    finally:
        for i in range(count):
            if want_aligned and handles[i]:
                L.dliom_cloud_destroy(_vp(handles[i]))
        for cloud in made:
            cloud.close()


# ---- scan alignment by NDT (include/dliom.h "scan alignment by NDT") -----------------------------------------------------
NDT_JACOBI_SWEEPS, NDT_PINV_SWEEPS, NDT_MAX_CELL_INDEX = 8, 12, 1 << 20
NDT_STEP_CLAMPED, NDT_STEP_MORE_THUENTE = 0, 1
NDT_NOT_CONVERGED, NDT_ITERATIONS, NDT_EPSILON, NDT_ZERO_STEP = range(4)
NDT_EVAL_GRADIENT, NDT_EVAL_ALL, NDT_EVAL_HESSIAN = range(3)


class NdtOptions(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("resolution", "step_size", "transformation_epsilon", "outlier_ratio")] + \
               [(f, C.c_int) for f in ("maximum_iterations", "min_points_per_voxel", "step_mode", "reserved")]


class NdtCell(C.Structure):
    _fields_ = [("index", C.c_int32 * 3), ("valid", C.c_int32), ("n", C.c_int64), ("mean", C.c_double * 3),
                ("icov", C.c_double * 6)]


class NdtTargetMemory(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("points", "kept_points", "cells", "valid_cells", "target_bytes", "scratch_bytes",
                                         "read_backs")] + [("build_ms", C.c_double)]


class NdtResult(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("converged", "reason", "iterations", "reserved")] + \
               [(f, C.c_int64) for f in ("evaluations_with_hessian", "evaluations_without_hessian")] + \
               [("p", C.c_double * 6), ("transform", C.c_double * 16), ("score", C.c_double),
                ("transformation_probability", C.c_double), ("fitness_score", C.c_double)] + \
               [(f, C.c_int64) for f in ("fitness_count", "pairs", "read_backs")] + \
               [(f, C.c_double) for f in ("evaluate_ms", "reduce_ms", "host_ms")]


SYMBOLS += [
    ("dliom_ndt_default_options", C.c_int, [C.POINTER(NdtOptions)]),
    ("dliom_ndt_target_create", C.c_int, [_vp, _vp, C.POINTER(NdtOptions), C.POINTER(_vp)]),
    ("dliom_ndt_target_destroy", None, [_vp]),
    ("dliom_ndt_target_memory_stats", C.c_int, [_vp, C.POINTER(NdtTargetMemory)]),
    ("dliom_ndt_target_cells", C.c_int, [_vp, C.POINTER(NdtCell), C.c_int64, _i64p]),
    ("dliom_ndt_evaluate", C.c_int, [_vp, _vp, _f64p, C.POINTER(NdtOptions), C.c_int, _f64p, _f64p, _f64p, _i64p]),
    ("dliom_ndt_align", C.c_int, [_vp, _vp, _f64p, C.POINTER(NdtOptions), _vp, C.POINTER(NdtResult), C.POINTER(_vp)]),
]


def ndt_options(**overrides):
    """dliom_ndt_default_options (the ground-truth tool's and MatchByNDT's values) with fields replaced"""
    o = NdtOptions()
    _check(load_library().dliom_ndt_default_options(C.byref(o)), "dliom_ndt_default_options")
    for k, v in overrides.items():
        if k not in dict(NdtOptions._fields_):
            raise TypeError("no NDT option " + k)
        setattr(o, k, v)
    return o


class NdtTarget:
    """The target's cells in HBM (dliom_ndt_target): pcl::VoxelGridCovariance as dliom.h states it."""

    def __init__(self, ctx, target, options=None):
        self.ctx, self._L = ctx, ctx._L
        self.options = options if options is not None else ndt_options()
        cloud, mine = _as_cloud(ctx, target)
        h = _vp()
        try:
            _check(self._L.dliom_ndt_target_create(ctx.h, cloud.h, C.byref(self.options), C.byref(h)), "dliom_ndt_target_create")
        finally:
            if mine:
                cloud.close()
        self.h = h

    @classmethod
    def _adopt(cls, ctx, options, handle):
        """a target that a batched build made (ndt_targets_batch)"""
        t = cls.__new__(cls)
        t.ctx, t._L, t.options, t.h = ctx, ctx._L, options, handle
        return t

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_ndt_target_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory_stats(self):
        m = NdtTargetMemory()
        _check(self._L.dliom_ndt_target_memory_stats(self.h, C.byref(m)), "dliom_ndt_target_memory_stats")
        return {k: getattr(m, k) for k, _ in NdtTargetMemory._fields_}

    def cells(self):
        """-> dict(index (m, 3) int32, n (m,) int64, valid (m,) bool, mean (m, 3), icov (m, 6)), in key order (z, y, x)"""
        count = C.c_int64()
        _check(self._L.dliom_ndt_target_cells(self.h, None, 0, C.byref(count)), "dliom_ndt_target_cells")
        m = int(count.value)
        buf = (NdtCell * max(m, 1))()
        _check(self._L.dliom_ndt_target_cells(self.h, buf, m, C.byref(count)), "dliom_ndt_target_cells")
        a = np.frombuffer(buf, dtype=np.dtype([("index", np.int32, 3), ("valid", np.int32), ("n", np.int64),
                                               ("mean", np.float64, 3), ("icov", np.float64, 6)]))[:m]
        return {"index": a["index"].copy(), "n": a["n"].copy(), "valid": a["valid"] != 0, "mean": a["mean"].copy(),
                "icov": a["icov"].copy()}


def _ndt_result(r):
    out = {k: getattr(r, k) for k, _ in NdtResult._fields_ if k not in ("transform", "p", "reserved")}
    out["p"] = np.array(r.p, dtype=np.float64)
    out["transform"] = np.array(r.transform, dtype=np.float64).reshape(4, 4)
    return out


class Ndt:
    """pcl::NormalDistributionsTransform as the ground-truth tool and MatchByNDT run it, on an NdtTarget
    (dliom_ndt_align).  Parity unpinned against PCL (dliom.h)."""

    def __init__(self, target, options=None, fitness_index=None):
        self.target, self._L = target, target._L
        self.options = options if options is not None else target.options
        self.fitness_index = fitness_index

    def align(self, source, guess=None, want_aligned=False):
        """-> result dict (p: (6,), transform: 4x4 float64), and the aligned points (n, 3) float32 if asked for"""
        cloud, mine = _as_cloud(self.target.ctx, source)
        try:
            g = _f64(np.eye(4) if guess is None else guess).reshape(16)
            r, h = NdtResult(), _vp()
            _check(self._L.dliom_ndt_align(self.target.h, cloud.h, _p(g, _f64p), C.byref(self.options),
                                           None if self.fitness_index is None else self.fitness_index.h, C.byref(r),
                                           C.byref(h) if want_aligned else None), "dliom_ndt_align")
            if not want_aligned:
                return _ndt_result(r)
            aligned = PointCloud(self.target.ctx, _handle=h)
            try:
                return _ndt_result(r), aligned.download()
            finally:
                aligned.close()
        finally:
            if mine:
                cloud.close()

    def evaluate(self, source, p6, what=NDT_EVAL_ALL):
        """dliom_ndt_evaluate -> dict(score, gradient (6,), hessian (6, 6), pairs)"""
        cloud, mine = _as_cloud(self.target.ctx, source)
        try:
            p, score, g, H, pairs = _f64(p6).reshape(6), C.c_double(), np.zeros(6), np.zeros(36), C.c_int64()
            _check(self._L.dliom_ndt_evaluate(self.target.h, cloud.h, _p(p, _f64p), C.byref(self.options), int(what),
                                              C.byref(score), _p(g, _f64p), _p(H, _f64p), C.byref(pairs)), "dliom_ndt_evaluate")
            return {"score": score.value, "gradient": g, "hessian": H.reshape(6, 6), "pairs": int(pairs.value)}
        finally:
            if mine:
                cloud.close()


# many pairs in one call (dliom_ndt_align_batch): the ground-truth tool's loop under `--method ndt`
NDT_BATCH_MAX_PAIRS, NDT_BATCH_DEFAULT_POINTS = 256, 64 * 1024


class NdtPair(C.Structure):
    _fields_ = [("target", _vp), ("source", _vp), ("fitness_index", _vp), ("guess", C.c_double * 16)]


class NdtBatchLimits(C.Structure):
    _fields_ = [("max_pairs_in_flight", C.c_int), ("reserved", C.c_int), ("max_scratch_bytes", C.c_int64)]


class NdtBatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("pairs", "chunks", "steps", "read_backs", "synchronizations", "max_in_flight",
                                         "pair_evaluations", "pair_searches")] + \
               [("evaluation_launches", C.c_int64 * 3), ("mixed_steps", C.c_int64)] + \
               [(f, C.c_double) for f in ("evaluate_ms", "reduce_ms", "fitness_ms", "host_ms")]


SYMBOLS += [
    ("dliom_ndt_batch_default_limits", C.c_int, [C.POINTER(NdtBatchLimits)]),
    ("dliom_ndt_batch_scratch_bytes", C.c_int64, [C.c_int64]),
    ("dliom_ndt_align_batch", C.c_int, [_vp, C.POINTER(NdtPair), C.c_int, C.POINTER(NdtOptions), C.POINTER(NdtBatchLimits),
                                        C.POINTER(NdtResult), C.POINTER(_vp), C.POINTER(NdtBatchStats)]),
]


def ndt_batch_default_limits(**overrides):
    """dliom_ndt_batch_default_limits, with fields replaced"""
    lim = NdtBatchLimits()
    _check(load_library().dliom_ndt_batch_default_limits(C.byref(lim)), "dliom_ndt_batch_default_limits")
    for k, v in overrides.items():
        if k not in dict(NdtBatchLimits._fields_):
            raise TypeError("no NDT batch limit " + k)
        setattr(lim, k, v)
    return lim


def ndt_batch_scratch_bytes(n):
    """the device scratch one pair in flight with n source points reserves (host only)"""
    return int(load_library().dliom_ndt_batch_scratch_bytes(int(n)))


def ndt_align_batch(ctx, pairs, options=None, limits=None, want_aligned=False):
    """dliom_ndt_align_batch.  pairs: a list of (NdtTarget, PointCloud or (n, 3) array, guess 4x4 or None[, NnIndex or
    None]).  -> (results, stats) or (results, stats, clouds): results as Ndt.align gives them, pair by pair and bit for bit
    (read_backs: the pair's rounds); stats a dict (evaluation_launches: a list by NDT_EVAL_*); clouds the aligned points,
    (n, 3) float32 each."""
    L = ctx._L
    options = options if options is not None else ndt_options()
    count = len(pairs)
    table, made = (NdtPair * max(count, 1))(), []
    handles = (_vp * max(count, 1))()
    try:
        uploaded = {}  # one upload for an array that several pairs name
        for i, pair in enumerate(pairs):
            target, source, guess = pair[:3]
            index = pair[3] if len(pair) > 3 else None
            if isinstance(source, PointCloud):
                cloud = source
            elif id(source) in uploaded:
                cloud = uploaded[id(source)]
            else:
                cloud = uploaded[id(source)] = PointCloud(ctx, source)
                made.append(cloud)
            table[i].target, table[i].source = target.h, cloud.h
            table[i].fitness_index = None if index is None else index.h
            table[i].guess[:] = list(_f64(np.eye(4) if guess is None else guess).reshape(16))
        results, stats = (NdtResult * max(count, 1))(), NdtBatchStats()
        _check(L.dliom_ndt_align_batch(ctx.h, table, count, C.byref(options), None if limits is None else C.byref(limits),
                                       results, handles if want_aligned else None, C.byref(stats)), "dliom_ndt_align_batch")
        out = [_ndt_result(results[i]) for i in range(count)]
        st = {k: (list(getattr(stats, k)) if k == "evaluation_launches" else getattr(stats, k)) for k, _ in NdtBatchStats._fields_}
        if not want_aligned:
            return out, st
        clouds = []
        for i in range(count):
            aligned = PointCloud(ctx, _handle=_vp(handles[i]))
            handles[i] = None
            try:
                clouds.append(aligned.download())
            finally:
                aligned.close()
        return out, st, clouds
    finally:
        for i in range(count):
            if want_aligned and handles[i]:
                L.dliom_cloud_destroy(_vp(handles[i]))
        for cloud in made:
            cloud.close()


# many targets in one call (dliom_ndt_target_create_batch): the K distinct target scans of that loop in one device chain a chunk
NDT_TARGET_BATCH_MAX_TARGETS = 256


class NdtTargetBatchLimits(C.Structure):
    _fields_ = [("max_targets_in_flight", C.c_int), ("reserved", C.c_int), ("max_points_in_flight", C.c_int64)]


class NdtTargetBatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("targets", "chunks", "points", "kept_points", "cells", "valid_cells", "read_backs",
                                         "synchronizations", "max_in_flight", "scratch_bytes")] + \
               [(f, C.c_double) for f in ("sort_ms", "sums_ms", "host_ms", "upload_ms")]


SYMBOLS += [
    ("dliom_ndt_target_batch_default_limits", C.c_int, [C.POINTER(NdtTargetBatchLimits)]),
    ("dliom_ndt_target_create_batch", C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(NdtOptions),
                                                C.POINTER(NdtTargetBatchLimits), C.POINTER(_vp), C.POINTER(NdtTargetBatchStats)]),
]


def ndt_target_batch_default_limits(**overrides):
    """dliom_ndt_target_batch_default_limits, with fields replaced"""
    lim = NdtTargetBatchLimits()
    _check(load_library().dliom_ndt_target_batch_default_limits(C.byref(lim)), "dliom_ndt_target_batch_default_limits")
    for k, v in overrides.items():
        if k not in dict(NdtTargetBatchLimits._fields_):
            raise TypeError("no NDT target batch limit " + k)
        setattr(lim, k, v)
    return lim


def ndt_targets_batch(ctx, clouds, options=None, limits=None):
    """dliom_ndt_target_create_batch.  clouds: a list of PointClouds or (n, 3) arrays, as NdtTarget takes them (an array
    that is named several times is uploaded once).  -> (targets, stats): an NdtTarget a cloud, cell for cell and bit for
    bit what NdtTarget(ctx, cloud, options) builds, each closed on its own; stats a dict."""
    L = ctx._L
    options = options if options is not None else ndt_options()
    count = len(clouds)
    table, handles, made = (_vp * max(count, 1))(), (_vp * max(count, 1))(), []
    try:
        uploaded = {}
        for i, source in enumerate(clouds):
            if isinstance(source, PointCloud):
                cloud = source
            elif id(source) in uploaded:
                cloud = uploaded[id(source)]
            else:
                cloud = uploaded[id(source)] = PointCloud(ctx, source)
                made.append(cloud)
            table[i] = cloud.h
        stats = NdtTargetBatchStats()
        _check(L.dliom_ndt_target_create_batch(ctx.h, table, count, C.byref(options), None if limits is None else C.byref(limits),
                                               handles, C.byref(stats)), "dliom_ndt_target_create_batch")
        targets = [NdtTarget._adopt(ctx, options, _vp(handles[i])) for i in range(count)]
        return targets, {k: getattr(stats, k) for k, _ in NdtTargetBatchStats._fields_}
    finally:
        for cloud in made:
            cloud.close()


# ---- the approximate voxel grid and MatchByNDT over a stream of scans (include/dliom.h) ------------------------------------
SYMBOLS += [
    ("dliom_cloud_approximate_voxel_filter", C.c_int, [_vp, _vp, C.c_float, C.POINTER(_vp)]),
    ("dliom_timed_cloud_points", C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    ("dliom_ndt_scan_matcher_create", C.c_int, [_vp, C.POINTER(NdtOptions), C.c_float, C.POINTER(_vp)]),
    ("dliom_ndt_scan_matcher_destroy", None, [_vp]),
    ("dliom_ndt_scan_matcher_match", C.c_int, [_vp, _vp, _f64p, C.POINTER(NdtResult)]),
    ("dliom_ndt_scan_matcher_has_target", C.c_int, [_vp, C.POINTER(C.c_int)]),
]


def approximate_voxel_filter(ctx, points, leaf):
    """pcl::ApproximateVoxelGrid as PCL 1.8.0 runs it, on the device (dliom_cloud_approximate_voxel_filter) -> a new
    PointCloud: the sequential loop's centroids, bit for bit and in its order"""
    cloud, mine = _as_cloud(ctx, points)
    try:
        h = _vp()
        _check(ctx._L.dliom_cloud_approximate_voxel_filter(ctx.h, cloud.h, C.c_float(leaf), C.byref(h)),
               "dliom_cloud_approximate_voxel_filter")
        return PointCloud(ctx, _handle=h)
    finally:
        if mine:
            cloud.close()


def timed_cloud_points(ctx, timed_cloud):
    """cvtPointCloud: a TimedCloud's xyz as a PointCloud, copied on the device (dliom_timed_cloud_points)"""
    h = _vp()
    _check(ctx._L.dliom_timed_cloud_points(ctx.h, timed_cloud.h, C.byref(h)), "dliom_timed_cloud_points")
    return PointCloud(ctx, _handle=h)


class NdtScanMatcher:
    """MatchByNDT as InitilizeByNDT calls it (dliom_ndt_scan_matcher): every scan is filtered once and aligned to its
    predecessor, whose cells stay in HBM."""

    def __init__(self, ctx, options=None, leaf=0.2):
        self.ctx, self._L = ctx, ctx._L
        self.options = options if options is not None else ndt_options()
        h = _vp()
        _check(self._L.dliom_ndt_scan_matcher_create(ctx.h, C.byref(self.options), C.c_float(leaf), C.byref(h)),
               "dliom_ndt_scan_matcher_create")
        self.h = h
        self.num_scans = 0  # the scans taken (a failed match takes none): a count for the caller, not what match() decides by

    @property
    def has_target(self):
        v = C.c_int()
        _check(self._L.dliom_ndt_scan_matcher_has_target(self.h, C.byref(v)), "dliom_ndt_scan_matcher_has_target")
        return v.value != 0

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_ndt_scan_matcher_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def match(self, scan, guess=None):
        """-> None for the first scan, else the result dict of Ndt.align for (previous scan, this scan, guess)"""
        cloud, mine = _as_cloud(self.ctx, scan)
        try:
            first = not self.has_target
            g = _f64(np.eye(4) if guess is None else guess).reshape(16)
            r = NdtResult()
            _check(self._L.dliom_ndt_scan_matcher_match(self.h, cloud.h, None if first else _p(g, _f64p),
                                                        None if first else C.byref(r)), "dliom_ndt_scan_matcher_match")
            self.num_scans += 1
            return None if first else _ndt_result(r)
        finally:
            if mine:
                cloud.close()


# ---- IMU-LiDAR initialisation (include/dliom.h "IMU-LiDAR initialisation") -------------------------------------------------
SYMBOLS += [
    ("dliom_imu_static_initialization", C.c_int, [C.c_int64, _f64p, _f64p, C.c_double, _f64p, _f64p, _f64p, _f64p, _f64p]),
]


def imu_static_initialization(acc, gyr, gravity_norm):
    """InitializeStatic (dliom_imu_static_initialization) on n accelerometer and gyroscope samples (n, 3)
    -> dict(R (3, 3) IMU frame to world, ba, bg, P, V)"""
    a, g = _f64(acc).reshape(-1, 3), _f64(gyr).reshape(-1, 3)
    if len(a) != len(g):
        raise ValueError("one gyroscope sample an accelerometer sample")
    R, ba, bg, P, V = np.zeros(9), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    _check(load_library().dliom_imu_static_initialization(len(a), _p(a, _f64p), _p(g, _f64p), float(gravity_norm), _p(R, _f64p),
                                                          _p(ba, _f64p), _p(bg, _f64p), _p(P, _f64p), _p(V, _f64p)),
           "dliom_imu_static_initialization")
    return {"R": R.reshape(3, 3), "ba": ba, "bg": bg, "P": P, "V": V}


INIT_OK, INIT_NO_EXCITATION, INIT_TOO_FEW_FRAMES, INIT_GRAVITY_NORM, INIT_SINGULAR = range(5)
INIT_MAX_FRAMES = 64


class InitFrame(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("has_preintegration", C.c_int), ("reserved", C.c_int), ("sum_dt", C.c_double),
                ("delta_p", C.c_double * 3), ("delta_v", C.c_double * 3)]


SYMBOLS += [
    ("dliom_imu_lidar_initialization", C.c_int, [C.POINTER(InitFrame), C.c_int, _f64p, C.c_double, _f64p, _f64p, C.POINTER(C.c_int)]),
    ("dliom_imu_lidar_align_with_world", C.c_int, [C.POINTER(InitFrame), C.c_int, _f64p, C.c_double, _f64p, _f64p, _f64p, _f64p, _f64p,
                                                   _f64p, C.POINTER(C.c_int)]),
]


def _init_frames(frames):
    """frames: (pose7, preintegration or None), the preintegration a dict with sum_dt, delta_p, delta_v (ImuIntegrator.get)"""
    out = (InitFrame * max(len(frames), 1))()
    for f, (pose, pre) in zip(out, frames):
        f.pose[:] = [float(v) for v in pose]
        f.has_preintegration = 0 if pre is None else 1
        if pre is not None:
            f.sum_dt = float(pre["sum_dt"])
            f.delta_p[:] = [float(v) for v in pre["delta_p"]]
            f.delta_v[:] = [float(v) for v in pre["delta_v"]]
    return out


def imu_lidar_initialization(frames, transform_lb, gravity_norm):
    """Initializer::Initialization (dliom_imu_lidar_initialization) -> dict(outcome INIT_*, velocities (n, 3) each in its own
    frame, gravity (3,) in the first laser frame)"""
    n = len(frames)
    V, g, outcome = np.zeros(3 * max(n, 1)), np.zeros(3), C.c_int(-1)
    _check(load_library().dliom_imu_lidar_initialization(_init_frames(frames), n, _p(_f64(transform_lb), _f64p), float(gravity_norm),
                                                         _p(V, _f64p), _p(g, _f64p), C.byref(outcome)), "dliom_imu_lidar_initialization")
    return {"outcome": outcome.value, "velocities": V[:3 * n].reshape(n, 3), "gravity": g}


def imu_lidar_align_with_world(frames, transform_lb, gravity_norm):
    """AlignWithWorld (dliom_imu_lidar_align_with_world) -> dict(outcome INIT_*, excitation, P (n, 3), R (n, 3, 3), V (n, 3) in
    the world frame, gravity_in_laser, world_rotation (3, 3))"""
    n = len(frames)
    P, R, V, g, Rw = np.zeros(3 * max(n, 1)), np.zeros(9 * max(n, 1)), np.zeros(3 * max(n, 1)), np.zeros(3), np.zeros(9)
    excitation, outcome = np.zeros(1), C.c_int(-1)
    _check(load_library().dliom_imu_lidar_align_with_world(_init_frames(frames), n, _p(_f64(transform_lb), _f64p), float(gravity_norm),
                                                           _p(P, _f64p), _p(R, _f64p), _p(V, _f64p), _p(g, _f64p), _p(Rw, _f64p),
                                                           _p(excitation, _f64p), C.byref(outcome)), "dliom_imu_lidar_align_with_world")
    return {"outcome": outcome.value, "excitation": float(excitation[0]), "P": P[:3 * n].reshape(n, 3), "R": R[:9 * n].reshape(n, 3, 3),
            "V": V[:3 * n].reshape(n, 3), "gravity_in_laser": g, "world_rotation": Rw.reshape(3, 3)}


# ---- node clouds kept in HBM (include/dliom.h "node clouds kept in HBM") ---------------------------------------------------
class NodeCloudInfo(C.Structure):
    _fields_ = [("timestamp", C.c_int64), ("trajectory_id", C.c_int32), ("node_index", C.c_int32), ("local_pose7", C.c_double * 7),
                ("origin_in_local", C.c_float * 3)]

    def as_dict(self):
        return {"timestamp": int(self.timestamp), "trajectory_id": int(self.trajectory_id), "node_index": int(self.node_index),
                "local_pose7": np.array(self.local_pose7[:], dtype=np.float64),
                "origin_in_local": np.array(self.origin_in_local[:], dtype=np.float32)}


class NodeCloudsMemory(C.Structure):
    _fields_ = [("slabs", C.c_int64), ("bytes_used", C.c_int64), ("bytes_reserved", C.c_int64), ("table_bytes", C.c_int64),
                ("scratch_bytes", C.c_int64)]


class NodeCloudsTransform(C.Structure):
    _fields_ = [("num_poses", C.c_int), ("per_node", C.c_int), ("poses7", _f32p)]


class NodeCloudsLimits(C.Structure):
    _fields_ = [("max_points_per_chunk", C.c_int64)]


class NodeCloudsStats(C.Structure):
    _fields_ = [("chunks", C.c_int), ("launches", C.c_int), ("readbacks", C.c_int), ("points", C.c_int64), ("bytes", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


NODE_RANGE_MAX_RECORD = 17  # DLIOM_NODE_RANGE_MAX_RECORD: tag, length, three tagged floats
SYMBOLS += [
    ("dliom_node_clouds_create", C.c_int, [_vp, C.POINTER(_vp)]),
    ("dliom_node_clouds_create_sized", C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    ("dliom_node_clouds_destroy", C.c_int, [_vp]),
    ("dliom_node_clouds_clear", C.c_int, [_vp]),
    ("dliom_node_clouds_add", C.c_int, [_vp, C.POINTER(NodeCloudInfo), _vp, _vp, _f32p, _i64p]),
    ("dliom_node_clouds_size", C.c_int, [_vp, _i64p, _i64p, _i64p]),
    ("dliom_node_clouds_info", C.c_int, [_vp, C.c_int64, C.POINTER(NodeCloudInfo), _i64p, _i64p]),
    ("dliom_node_clouds_memory_stats", C.c_int, [_vp, C.POINTER(NodeCloudsMemory)]),
    ("dliom_node_clouds_download", C.c_int, [_vp, C.c_int64, _f32p, _f32p]),
    ("dliom_node_clouds_pack_point_cloud2", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(NodeCloudsTransform), C.POINTER(NodeCloudsLimits),
                                                      _u8p, C.c_int64, _i64p, C.POINTER(NodeCloudsStats)]),
    ("dliom_cloud_pack_point_cloud2", C.c_int, [_vp, _f32p, _u8p, C.c_int64, _i64p]),
    ("dliom_rigid3f_inverse", C.c_int, [_f32p, _f32p]),
    ("dliom_node_clouds_to_proto", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(NodeCloudsLimits), _u8p, C.c_int64, _i64p,
                                             C.POINTER(NodeCloudsStats)]),
    ("dliom_node_range_data_check", C.c_int, [_u8p, C.c_int64, C.POINTER(NodeCloudInfo), _i64p, _i64p]),
    ("dliom_node_range_data_from_proto", C.c_int, [_vp, _u8p, C.c_int64, C.POINTER(NodeCloudInfo), C.POINTER(_vp), C.POINTER(_vp)]),
]


def rigid3f_inverse(pose7):
    """Rigid3f::inverse of a float pose [t, q] (dliom_rigid3f_inverse; host) -> float32[7]."""
    out = np.zeros(7, dtype=np.float32)
    _check(load_library().dliom_rigid3f_inverse(_p(_f32(pose7).reshape(7), _f32p), _p(out, _f32p)), "dliom_rigid3f_inverse")
    return out


def _node_cloud_info(timestamp=0, trajectory_id=0, node_index=0, local_pose7=(0, 0, 0, 1, 0, 0, 0), origin_in_local=(0, 0, 0)):
    info = NodeCloudInfo()
    info.timestamp, info.trajectory_id, info.node_index = int(timestamp), int(trajectory_id), int(node_index)
    info.local_pose7[:] = [float(v) for v in local_pose7]
    info.origin_in_local[:] = [float(np.float32(v)) for v in origin_in_local]
    return info


def _cloud_pack_point_cloud2(self, pose7=None, capacity=None, fill=0):
    """msg.data of ToPointCloud2Message(TransformPointCloud(cloud, pose7)): x, y, z, 1.0f a point (dliom_cloud_pack_point_cloud2)
    -> (uint8 array of `capacity` bytes, default the exact size; the size)."""
    pose = None if pose7 is None else _p(_f32(pose7).reshape(7), _f32p)
    out = np.full(16 * self.n if capacity is None else int(capacity), fill, dtype=np.uint8)
    n = C.c_int64()
    _check(self._L.dliom_cloud_pack_point_cloud2(self.h, pose, _p(out, _u8p), len(out), C.byref(n)), "dliom_cloud_pack_point_cloud2")
    return out, int(n.value)


PointCloud.pack_point_cloud2 = _cloud_pack_point_cloud2


class NodeClouds:
    """Every scan's range_data_in_local kept in HBM (dliom_node_clouds): MapBuilderBridge's range_data_local_all_."""

    def __init__(self, ctx, slab_floats=0):
        self._L = ctx._L
        self.ctx = ctx
        h = _vp()
        _check(self._L.dliom_node_clouds_create_sized(ctx.h, int(slab_floats), C.byref(h)), "dliom_node_clouds_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._L.dliom_node_clouds_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.size()[0]

    def clear(self):
        _check(self._L.dliom_node_clouds_clear(self.h), "dliom_node_clouds_clear")

    def add(self, returns, misses=None, pose_to_local=None, **info):
        """Keeps a scan (PointCloud objects of this context; pose_to_local: a float pose applied on the way in) -> its index.
        info: timestamp, trajectory_id, node_index, local_pose7, origin_in_local."""
        index = C.c_int64(-1)
        pose = None if pose_to_local is None else _p(_f32(pose_to_local).reshape(7), _f32p)
        _check(self._L.dliom_node_clouds_add(self.h, C.byref(_node_cloud_info(**info)), returns.h, None if misses is None else misses.h,
                                             pose, C.byref(index)), "dliom_node_clouds_add")
        return int(index.value)

    def size(self):
        """(nodes, returns, misses)"""
        v = [C.c_int64() for _ in range(3)]
        _check(self._L.dliom_node_clouds_size(self.h, *[C.byref(x) for x in v]), "dliom_node_clouds_size")
        return tuple(int(x.value) for x in v)

    def info(self, index):
        """dict of the node's info, with num_returns and num_misses"""
        info, r, m = NodeCloudInfo(), C.c_int64(), C.c_int64()
        _check(self._L.dliom_node_clouds_info(self.h, int(index), C.byref(info), C.byref(r), C.byref(m)), "dliom_node_clouds_info")
        return dict(info.as_dict(), num_returns=int(r.value), num_misses=int(m.value))

    def memory_stats(self):
        m = NodeCloudsMemory()
        _check(self._L.dliom_node_clouds_memory_stats(self.h, C.byref(m)), "dliom_node_clouds_memory_stats")
        return {name: int(getattr(m, name)) for name, _ in m._fields_}

    def download(self, index):
        """(returns (n, 3), misses (m, 3)) of a node as kept"""
        i = self.info(index)
        r, m = np.zeros((i["num_returns"], 3), dtype=np.float32), np.zeros((i["num_misses"], 3), dtype=np.float32)
        _check(self._L.dliom_node_clouds_download(self.h, int(index), _p(r, _f32p), _p(m, _f32p)), "dliom_node_clouds_download")
        return r, m

    def _range(self, first, count):
        first = int(first)
        return first, (len(self) - first if count is None else int(count))

    def _batched(self, call, count, capacity, fill):
        """query-then-fill of a batched call -> (uint8 bytes, int64 offsets (count + 1), stats dict, status)"""
        offsets, stats = np.zeros(count + 1, dtype=np.int64), NodeCloudsStats()
        if capacity is None:
            _check(call(None, 0, _p(offsets, _i64p), C.byref(stats)), "node clouds size query")
            capacity = int(offsets[count])
        out = np.full(int(capacity), fill, dtype=np.uint8)
        status = call(_p(out, _u8p), len(out), _p(offsets, _i64p), C.byref(stats))
        if status not in (OK, ERR_CAPACITY):
            _check(status, "node clouds batched call")
        return out, offsets, stats.as_dict(), status

    def pack_point_cloud2(self, first=0, count=None, poses=None, per_node=False, max_points_per_chunk=0, capacity=None, fill=0):
        """msg.data of the nodes [first, first + count): x, y, z, 1.0f a return (dliom_node_clouds_pack_point_cloud2).
        poses: None, or float poses [t, q] -- (7,) or (2, 7) shared by all nodes, (count, 7) or (count, 2, 7) with per_node.
        -> (bytes, offsets, stats, status OK or ERR_CAPACITY)"""
        first, count = self._range(first, count)
        t = NodeCloudsTransform(0, 0, None)
        if poses is not None:
            p = _f32(poses)
            num = p.size // 7 // max(count, 1) if per_node else p.size // 7
            if num not in (1, 2) or p.size != 7 * num * (count if per_node else 1):
                raise ValueError("one or two poses, for all nodes or for each")
            t = NodeCloudsTransform(num, 1 if per_node else 0, _p(p, _f32p))
        limits = NodeCloudsLimits(int(max_points_per_chunk))
        return self._batched(lambda b, c, o, s: self._L.dliom_node_clouds_pack_point_cloud2(
            self.h, first, count, C.byref(t), C.byref(limits), b, c, o, s), count, capacity, fill)

    def to_proto(self, first=0, count=None, max_points_per_chunk=0, capacity=None, fill=0):
        """The nodes' mapping::proto::NodeRangeData messages back to back (dliom_node_clouds_to_proto)
        -> (bytes, offsets, stats, status OK or ERR_CAPACITY)"""
        first, count = self._range(first, count)
        limits = NodeCloudsLimits(int(max_points_per_chunk))
        return self._batched(lambda b, c, o, s: self._L.dliom_node_clouds_to_proto(self.h, first, count, C.byref(limits), b, c, o, s),
                             count, capacity, fill)


def node_range_data_from_proto(ctx, data):
    """A NodeRangeData message (bytes) -> (info dict, returns PointCloud, misses PointCloud) (dliom_node_range_data_from_proto)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info, r, m = NodeCloudInfo(), _vp(), _vp()
    _check(ctx._L.dliom_node_range_data_from_proto(ctx.h, _p(buf, _u8p) if len(buf) else None, len(buf), C.byref(info), C.byref(r), C.byref(m)),
           "dliom_node_range_data_from_proto")
    return info.as_dict(), PointCloud(ctx, _handle=r), PointCloud(ctx, _handle=m)


def node_range_data_check(data):
    """The host parse of a NodeRangeData message alone -> (info dict, num_returns, num_misses); DliomError if malformed."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info, r, m = NodeCloudInfo(), C.c_int64(), C.c_int64()
    _check(load_library().dliom_node_range_data_check(_p(buf, _u8p) if len(buf) else None, len(buf), C.byref(info), C.byref(r), C.byref(m)),
           "dliom_node_range_data_check")
    return info.as_dict(), int(r.value), int(m.value)


# ---- gzip on the device (dliom.h "gzip on the device"; csrc/gzip.hip, csrc/gzip_host.cc) ----
GZIP_CHUNK = 4096  # DLIOM_GZIP_CHUNK
ERR_TOO_LARGE = -14


class GzipStats(C.Structure):
    _fields_ = [("chunks", C.c_int64), ("chunks_stored", C.c_int64), ("read_backs", C.c_int64), ("bytes_downloaded", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


SYMBOLS += [
    ("dliom_gzip_bound", C.c_int64, [C.c_int64]),
    ("dliom_gzip_host", C.c_int, [_u8p, C.c_int64, _u8p, C.c_int64, _i64p]),
    ("dliom_gzip", C.c_int, [_vp, _u8p, C.c_int64, _u8p, C.c_int64, _i64p, C.POINTER(GzipStats)]),
    ("dliom_gzip_segments", C.c_int, [_vp, _u8p, _i64p, C.c_int64, _u8p, C.c_int64, _i64p, C.POINTER(GzipStats)]),
    ("dliom_grid_xray_texture_gzip", C.c_int, [_vp, _f64p, _u8p, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, C.POINTER(GzipStats)]),
    ("dliom_node_clouds_to_pbstream", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(NodeCloudsLimits), _u8p, C.c_int64, _i64p,
                                                C.POINTER(NodeCloudsStats), C.POINTER(GzipStats)]),
]


def gzip_bound(n):
    """dliom_gzip_bound: 18 + n + 5 * max(1, ceil(n / 4096)); a buffer of that size is never too small."""
    return int(load_library().dliom_gzip_bound(int(n)))


def _gzip_input(data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    return buf, (_p(buf, _u8p) if buf.size else None)


def gzip_host(data, capacity=None):
    """One gzip member of `data` by the statement of dliom.h "gzip on the device", on one host thread (dliom_gzip_host)
    -> bytes.  capacity: the output buffer's size (default the bound); too small raises DliomError(ERR_CAPACITY)."""
    buf, ptr = _gzip_input(data)
    out = np.zeros(gzip_bound(buf.size) if capacity is None else int(capacity), dtype=np.uint8)
    size = C.c_int64()
    _check(load_library().dliom_gzip_host(ptr, buf.size, _p(out, _u8p), out.size, C.byref(size)), "dliom_gzip_host")
    return out[:size.value].tobytes()


def gzip(ctx, data, capacity=None, with_stats=False):
    """One gzip member of `data`, compressed on the device (dliom_gzip): upload, one launch chain, one polled read-back, one
    download of exactly the compressed bytes -> bytes, or (bytes, stats dict)."""
    buf, ptr = _gzip_input(data)
    out = np.zeros(gzip_bound(buf.size) if capacity is None else int(capacity), dtype=np.uint8)
    size, stats = C.c_int64(), GzipStats()
    _check(ctx._L.dliom_gzip(ctx.h, ptr, buf.size, _p(out, _u8p), out.size, C.byref(size), C.byref(stats)), "dliom_gzip")
    member = out[:size.value].tobytes()
    return (member, stats.as_dict()) if with_stats else member


def gzip_segments(ctx, data, offsets, capacity=None, with_stats=False):
    """K gzip members in one launch chain (dliom_gzip_segments): segment s is data[offsets[s]:offsets[s + 1]]
    -> list of K bytes objects, or (list, stats dict)."""
    buf, ptr = _gzip_input(data)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    k = off.size - 1
    if k < 0 or (k >= 0 and off.size and (off[0] < 0 or off[-1] > buf.size)):
        raise ValueError("offsets must hold k + 1 entries inside the data")
    if capacity is None:
        capacity = sum(gzip_bound(int(off[s + 1] - off[s])) for s in range(k) if off[s + 1] >= off[s])
    out = np.zeros(max(int(capacity), 1), dtype=np.uint8)
    out_off, stats = np.zeros(k + 1, dtype=np.int64), GzipStats()
    _check(ctx._L.dliom_gzip_segments(ctx.h, ptr, _p(off, _i64p), k, _p(out, _u8p), int(capacity), _p(out_off, _i64p), C.byref(stats)),
           "dliom_gzip_segments")
    members = [out[out_off[s]:out_off[s + 1]].tobytes() for s in range(k)]
    return (members, stats.as_dict()) if with_stats else members


def grid_xray_texture_gzip(grid, pose, with_stats=False):
    """grid_xray_texture with `cells` leaving HBM as one gzip member, ready for the proto field (dliom_grid_xray_texture_gzip)
    -> (width, height, resolution, slice_pose7, cells_gz bytes), with the gzip stats dict behind them if with_stats."""
    p = _pose7(pose)
    w, h, res, size, stats = C.c_int32(), C.c_int32(), C.c_double(), C.c_int64(), GzipStats()
    slice_pose = np.zeros(7, dtype=np.float64)
    L = grid._L
    _check(L.dliom_grid_xray_texture_gzip(grid.h, _p(p, _f64p), None, 0, C.byref(size), C.byref(w), C.byref(h), C.byref(res),
                                          _p(slice_pose, _f64p), None), "dliom_grid_xray_texture_gzip")
    out = np.zeros(size.value, dtype=np.uint8)
    _check(L.dliom_grid_xray_texture_gzip(grid.h, _p(p, _f64p), _p(out, _u8p), out.size, C.byref(size), C.byref(w), C.byref(h),
                                          C.byref(res), _p(slice_pose, _f64p), C.byref(stats)), "dliom_grid_xray_texture_gzip")
    result = (w.value, h.value, res.value, slice_pose, out[:size.value].tobytes())
    return result + (stats.as_dict(),) if with_stats else result


def _node_clouds_to_pbstream(self, first=0, count=None, max_points_per_chunk=0, capacity=None, fill=0):
    """The nodes' NodeRangeData messages as ProtoStreamWriter::WriteProto writes them: the 8-byte little-endian size of the
    gzip member, then the member, a record a node (dliom_node_clouds_to_pbstream).  capacity: default the bound that never
    fails -> (bytes, offsets (count + 1), stats, gzip stats, status OK or ERR_CAPACITY)"""
    first, count = self._range(first, count)
    if capacity is None:
        capacity = 0
        for i in range(first, first + count):
            info = self.info(i)
            capacity += 8 + gzip_bound(192 + NODE_RANGE_MAX_RECORD * (info["num_returns"] + info["num_misses"]))
    limits = NodeCloudsLimits(int(max_points_per_chunk))
    out = np.full(max(int(capacity), 1), fill, dtype=np.uint8)
    offsets, stats, gz = np.zeros(count + 1, dtype=np.int64), NodeCloudsStats(), GzipStats()
    status = self._L.dliom_node_clouds_to_pbstream(self.h, first, count, C.byref(limits), _p(out, _u8p), int(capacity), _p(offsets, _i64p),
                                                   C.byref(stats), C.byref(gz))
    if status not in (OK, ERR_CAPACITY):
        _check(status, "dliom_node_clouds_to_pbstream")
    return out, offsets, stats.as_dict(), gz.as_dict(), status


NodeClouds.to_pbstream = _node_clouds_to_pbstream
