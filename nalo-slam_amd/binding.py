"""ctypes binding of libnalo_gpu.so (the C-ABI in include/nalo_gpu.h). The product path: it fails loudly when
the HIP library is missing or no gfx950 device is present — there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

c_dp = C.POINTER(C.c_double)
c_fp = C.POINTER(C.c_float)
c_ip = C.POINTER(C.c_int)
c_u8p = C.POINTER(C.c_uint8)
c_i8p = C.POINTER(C.c_int8)


class FrameState(C.Structure):
    _fields_ = [("slot", C.c_int), ("frame_id", C.c_int), ("worldToCam_evalPT", C.c_double * 12), ("state", C.c_double * 10),
                ("state_zero", C.c_double * 10), ("ab_exposure", C.c_float), ("frameEnergyTH", C.c_float)]


ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)
INJECT_LM_LOST_BLOCK, INJECT_GATED_SOLVE = 1, 2       # nalo_test_inject's `what` (include/nalo_gpu.h)

EXPORTS = [
    "nalo_create", "nalo_destroy", "nalo_last_error", "nalo_levels", "nalo_sync", "nalo_stream", "nalo_test_inject",
    "nalo_frame_upload", "nalo_frame_upload_raw", "nalo_frame_upload_raw_async", "nalo_undist_set", "nalo_frame_upload_async", "nalo_frame_wait", "nalo_frame_ingest_device", "nalo_frame_release", "nalo_dev_plane_check", "nalo_frame_attach", "nalo_host_alloc", "nalo_host_free", "nalo_frame_rebuild", "nalo_frame_download", "nalo_frame_download_mask", "nalo_frame_plane",
    "nalo_trk_make_k", "nalo_trk_set_ref", "nalo_trk_ref_upload", "nalo_trk_set_ref_resident", "nalo_trk_set_ref_from_window", "nalo_trk_set_ref_from_depth", "nalo_trk_set_pc", "nalo_trk_get_pc", "nalo_trk_append_plane_points", "nalo_trk_get_depth", "nalo_trk_set_depth", "nalo_trk_ref_export", "nalo_trk_ref_import", "nalo_trk_ref_release", "nalo_trk_depth_image", "nalo_trk_eval", "nalo_trk_track", "nalo_trk_track_tries", "nalo_trk_motion_tries", "nalo_trk_last_evals", "nalo_trk_get_launch_config", "nalo_trk_set_shard",
    "nalo_ba_set_window", "nalo_ba_set_points", "nalo_ba_set_residuals", "nalo_ba_set_prior", "nalo_ba_get_prior",
    "nalo_ba_linearize", "nalo_ba_accumulate", "nalo_ba_accumulate_sc", "nalo_ba_solve_system", "nalo_ba_backup_state",
    "nalo_ba_do_step", "nalo_ba_optimize", "nalo_ba_marginalize_points", "nalo_ba_marginalize_frame", "nalo_ba_set_prior_carry", "nalo_ba_calc_l_energy", "nalo_ba_calc_m_energy", "nalo_ba_plane_scale_fix", "nalo_ba_sw_gray_optimize", "nalo_ba_optimize_stats", "nalo_get_settings", "nalo_set_settings", "nalo_constants", "nalo_constants_device", "nalo_ba_get_frames", "nalo_ba_get_points",
    "nalo_ba_get_residuals", "nalo_ba_get_pattern_projections", "nalo_ba_residual_plot", "nalo_ba_get_idepth_zero", "nalo_ba_get_acc13", "nalo_ba_counts", "nalo_ba_get_launch_config", "nalo_ba_set_allreduce", "nalo_ba_set_allreduce_mode", "nalo_ba_set_allreduce_side", "nalo_ba_exchange_failed", "nalo_side_stream", "nalo_rccl_unique_id", "nalo_ba_rccl_init", "nalo_ba_set_rccl_comm", "nalo_ba_rccl_ranks", "nalo_shard_points", "nalo_ba_snapshot", "nalo_ba_restore",
    "nalo_ba_set_point_history", "nalo_ba_get_point_history", "nalo_ba_flag_points", "nalo_ba_marginalize_flagged",
    "nalo_ba_carry_window", "nalo_ba_carry_map", "nalo_ba_carry_last",
    "nalo_ba_window_from_initializer", "nalo_ba_init_window_map", "nalo_ba_init_window_last",
    "nalo_map_enable", "nalo_map_reset", "nalo_map_counts", "nalo_map_get_frame", "nalo_map_world_points", "nalo_map_world_points_host", "nalo_map_frame_cloud",
    "nalo_map_graph_enable", "nalo_map_graph", "nalo_map_graph_connections", "nalo_map_window_plot", "nalo_map_render", "nalo_view_look_at", "nalo_map_render_mesh", "nalo_view_triangle",
    "nalo_dense_update_map", "nalo_map_dense_enable", "nalo_map_dense_counts", "nalo_map_dense_get", "nalo_map_dense_world_points", "nalo_map_dense_cloud",
    "nalo_tsdf_create", "nalo_tsdf_reset", "nalo_tsdf_destroy", "nalo_tsdf_integrate_depth", "nalo_tsdf_release", "nalo_tsdf_integrate_frame", "nalo_tsdf_last", "nalo_tsdf_get", "nalo_tsdf_set", "nalo_tsdf_view", "nalo_tsdf_surface_points", "nalo_tsdf_frustum_box", "nalo_tsdf_mesh", "nalo_tsdf_mesh_view", "nalo_tsdf_mesh_table",
    "nalo_tsdf_color_enable", "nalo_tsdf_color_disable", "nalo_tsdf_integrate_depth_color", "nalo_tsdf_color_get", "nalo_tsdf_color_set", "nalo_tsdf_color_view", "nalo_tsdf_mesh_color", "nalo_tsdf_mesh_color_view",
    "nalo_tsdf_raycast", "nalo_tsdf_raycast_view", "nalo_tsdf_raycast_steps",
    "nalo_tsdf_align_eval", "nalo_tsdf_align_depth", "nalo_tsdf_align_frame", "nalo_tsdf_align_step",
    "nalo_tsdf_shift", "nalo_tsdf_geometry", "nalo_tsdf_shift_for", "nalo_tsdf_shift_boxes",
    "nalo_tsdf_replace_depth", "nalo_tsdf_replace_last", "nalo_tsdf_replace_frame", "nalo_tsdf_log_enable", "nalo_tsdf_log_get", "nalo_tsdf_est_world_to_cam", "nalo_tsdf_frustum_box_est",
    "nalo_tsdf_box_shift",
    "nalo_tsdf_replace_depth_n", "nalo_tsdf_replace_last_n", "nalo_tsdf_replace_frames", "nalo_tsdf_replace_frames_plan",
    "nalo_tsdf_archive_enable", "nalo_tsdf_archive_disable", "nalo_tsdf_archive_reset", "nalo_tsdf_archive_mesh", "nalo_tsdf_archive_stats", "nalo_tsdf_archive_get", "nalo_tsdf_archive_view", "nalo_tsdf_follow",
    "nalo_imm_create", "nalo_imm_trace", "nalo_imm_optimize", "nalo_imm_resident_set", "nalo_imm_resident_optimize", "nalo_imm_resident_trace", "nalo_imm_resident_get", "nalo_imm_resident_set_type", "nalo_imm_resident_activate", "nalo_imm_activate_last",
    "nalo_imm_resident_carry", "nalo_imm_resident_carry_map", "nalo_imm_resident_carry_last", "nalo_imm_resident_get_points", "nalo_init_calc_res_and_gs", "nalo_init_do_step", "nalo_init_set_first", "nalo_init_track_frame", "nalo_init_get_state", "nalo_init_get_points", "nalo_init_set_state", "nalo_init_set_points", "nalo_init_get_carried", "nalo_init_sweep", "nalo_init_depth_image", "nalo_dist_make_map", "nalo_pixsel_make_hists",
    "nalo_pixsel_set_random", "nalo_pixsel_select", "nalo_pixsel_make_maps", "nalo_pixsel_make_maps_lidar", "nalo_pixsel_get_selected",
    "nalo_dense_make_map", "nalo_trk_fit_planes", "nalo_trk_fit_ground", "nalo_ground_tracker_init", "nalo_ground_globals_init", "nalo_ground_frame_init", "nalo_ground_update",
    "nalo_ground_set_global_plane", "nalo_ground_local_scale", "nalo_ground_reset_global_plane", "nalo_dense_fit_planes", "nalo_plane_fit_members", "nalo_profile_enable", "nalo_profile_select", "nalo_profile_reset", "nalo_profile_get", "nalo_profile_samples", "nalo_profile_sample", "nalo_hbm_calibrate",
]


DT_U8, DT_U16, DT_I32, DT_F32 = 1, 2, 3, 4               # NALO_DT_* (include/nalo_gpu.h)


class DevPlane(C.Structure):                              # nalo_dev_plane; dev_plane() builds one from a device array
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("w", C.c_int), ("h", C.c_int), ("channels", C.c_int),
                ("stride_y", C.c_longlong), ("stride_x", C.c_longlong), ("stride_c", C.c_longlong)]


class FrameIngestArgs(C.Structure):                       # nalo_frame_ingest_args
    _fields_ = [("image", C.POINTER(DevPlane)), ("exposure_time", C.c_float), ("factor", C.c_float), ("mask", C.POINTER(DevPlane)), ("colour", C.POINTER(DevPlane)),
                ("colour_is_rgb", C.c_int), ("gammaB", c_fp), ("producer_stream", C.c_void_p)]


class TrkDepthRefArgs(C.Structure):                       # nalo_trk_depth_ref_args
    _fields_ = [("depth", DevPlane), ("min_depth", C.c_float), ("max_depth", C.c_float), ("hdi", C.c_float), ("step", C.c_int), ("min_grad", C.c_float),
                ("producer_stream", C.c_void_p), ("n_seeded", C.c_int)]


MAX_LEVELS = 6                                           # NALO_MAX_LEVELS
PLANE_IRRADIANCE, PLANE_MASK, PLANE_COLOUR = 0, 1, 2      # NALO_PLANE_* (nalo_frame_plane's `which`)
_PLANE_NAMES = {"irradiance": PLANE_IRRADIANCE, "mask": PLANE_MASK, "colour": PLANE_COLOUR}


class TrkRefView(C.Structure):                            # nalo_trk_ref_view; trk_ref_view() builds one from device arrays
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("levels", C.c_int), ("slot_ref", C.c_int), ("n", C.c_int * MAX_LEVELS),
                ("u", C.c_void_p * MAX_LEVELS), ("v", C.c_void_p * MAX_LEVELS), ("idepth", C.c_void_p * MAX_LEVELS), ("color", C.c_void_p * MAX_LEVELS),
                ("idepth_map", C.c_void_p * MAX_LEVELS), ("weight_sums", C.c_void_p * MAX_LEVELS),
                ("fx", C.c_float * MAX_LEVELS), ("fy", C.c_float * MAX_LEVELS), ("cx", C.c_float * MAX_LEVELS), ("cy", C.c_float * MAX_LEVELS), ("stream", C.c_void_p)]


class InitWindowArgs(C.Structure):
    """nalo_init_window_args (include/nalo_gpu.h)"""
    _fields_ = [("first", FrameState), ("entering", FrameState), ("calib", C.c_double * 4), ("calib_zero", C.c_double * 4),
                ("desired_point_density", C.c_float), ("n_draws", C.c_int), ("draws", c_ip)]


class ImmCarryArgs(C.Structure):
    """nalo_imm_carry_args (include/nalo_gpu.h)"""
    _fields_ = [("fate", c_ip), ("n_sel", C.c_int), ("sel", c_ip), ("result", c_ip), ("host_map", c_ip), ("n_hosts_old", C.c_int),
                ("append_slot", C.c_int), ("append_host", C.c_int), ("append_n", C.c_int), ("append_idx", c_ip), ("append_status", c_u8p)]


class PlaneCluster(C.Structure):
    """nalo_plane_cluster (include/nalo_gpu.h)"""
    _fields_ = [("mask_value", C.c_float), ("n", C.c_int), ("n_cloud", C.c_int), ("rect", C.c_int * 4), ("fitted", C.c_int), ("plane", C.c_float * 4),
                ("best_sample", C.c_int), ("inliers", C.c_int), ("appended", C.c_int)]


class PlaneFitArgs(C.Structure):
    """nalo_plane_fit_args (include/nalo_gpu.h)"""
    _fields_ = [("threshold", C.c_float), ("min_points", C.c_int), ("n_samples", C.c_int), ("draws", C.POINTER(C.c_uint32)), ("append", C.c_int)]


PLANE_DTYPE = np.dtype([("mask_value", np.float32), ("n", np.int32), ("n_cloud", np.int32), ("rect", np.int32, 4), ("fitted", np.int32), ("plane", np.float32, 4),
                        ("best_sample", np.int32), ("inliers", np.int32), ("appended", np.int32)])
assert PLANE_DTYPE.itemsize == C.sizeof(PlaneCluster)


class GroundPick(C.Structure):
    """nalo_ground_pick (include/nalo_gpu.h)"""
    _fields_ = [("ran", C.c_int), ("cluster", C.c_int), ("gp_raw", C.c_float * 4), ("ground_height", C.c_float), ("n_ground_points", C.c_int)]


class GroundArgs(C.Structure):
    """nalo_ground_args (include/nalo_gpu.h)"""
    _fields_ = [("mark_window_points", C.c_int), ("onground", c_u8p), ("onground_cap", C.c_int), ("scores", C.c_void_p)]


class GroundTracker(C.Structure):
    """nalo_ground_tracker: one per CoarseTracker object (the reference swaps two every keyframe)"""
    _fields_ = [("ground_height", C.c_float), ("last_height", C.c_float), ("suc_num", C.c_int)]


class GroundGlobals(C.Structure):
    """nalo_ground_globals: util/settings.cpp:36-40"""
    _fields_ = [("scale_fix", C.c_int), ("init_height", C.c_float), ("last_ScaleRate", C.c_float), ("last_gp", C.c_float * 4), ("n_old", C.c_int),
                ("old_rate", C.c_float * 7)]


class GroundFrame(C.Structure):
    """nalo_ground_frame: one per window frame"""
    _fields_ = [("groundP", C.c_float * 4), ("last_ground", C.c_float * 4), ("haveground", C.c_int), ("scaleFixed", C.c_int)]


GROUND_SCORE_DTYPE = np.dtype([("mid_z", np.float32), ("score", np.float32), ("scored", np.int32)])     # nalo_ground_score
assert GROUND_SCORE_DTYPE.itemsize == 12 and C.sizeof(GroundPick) == 32


class MapCloudArgs(C.Structure):
    """nalo_map_cloud_args (include/nalo_gpu.h)"""
    _fields_ = [("frame_id", C.c_int), ("display_mode", C.c_int), ("with_immature", C.c_int), ("sparsity", C.c_int), ("scaledTH", C.c_float), ("absTH", C.c_float),
                ("minRelBS", C.c_float), ("n_draws", C.c_int), ("draws", c_ip), ("cap", C.c_int), ("xyz", c_fp), ("rgb", c_u8p), ("n", C.c_int), ("n_needed", C.c_int),
                ("records", C.c_int * 4), ("survivors", C.c_int * 4)]


# nalo_map_record (include/nalo_gpu.h)
MAP_RECORD_DTYPE = np.dtype([("u", np.float32), ("v", np.float32), ("idepth", np.float32), ("idepth_hessian", np.float32), ("maxRelBaseline", np.float32),
                             ("status", np.int32), ("decision", np.int32), ("frame_id", np.int32), ("color", np.float32, 8)])
assert MAP_RECORD_DTYPE.itemsize == 64
GRAPH_EDGE_DTYPE = np.dtype([("host_id", np.int32), ("target_id", np.int32), ("act", np.int32), ("marg", np.int32)])                       # nalo_graph_edge
GRAPH_CONNECTION_DTYPE = np.dtype([("from_id", np.int32), ("to_id", np.int32), ("fwdAct", np.int32), ("bwdAct", np.int32), ("fwdMarg", np.int32),
                                   ("bwdMarg", np.int32)])                                                                                    # nalo_graph_connection
assert GRAPH_EDGE_DTYPE.itemsize == 16 and GRAPH_CONNECTION_DTYPE.itemsize == 24


class MapDenseCloudArgs(C.Structure):
    """nalo_map_dense_cloud_args (include/nalo_gpu.h)"""
    _fields_ = [("frame_id", C.c_int), ("n_draws", C.c_int), ("draws", c_ip), ("cap", C.c_int), ("xyz", c_fp), ("rgb", c_u8p), ("n", C.c_int), ("n_needed", C.c_int),
                ("records", C.c_int), ("survivors", C.c_int)]


# nalo_dense_run, nalo_dense_point (include/nalo_gpu.h)
DENSE_RUN_DTYPE = np.dtype([("rect", np.int32, 4), ("n", np.int32), ("accept", np.int32), ("first", np.int64)])
DENSE_POINT_DTYPE = np.dtype([("u", np.uint16), ("v", np.uint16), ("idepth", np.float32), ("color", np.float32), ("bgr", np.uint8, 3), ("pad", np.uint8)])
assert DENSE_RUN_DTYPE.itemsize == 32 and DENSE_POINT_DTYPE.itemsize == 16


class TsdfDesc(C.Structure):                              # nalo_tsdf_desc; tsdf_desc() builds one
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("dims", C.c_int * 3), ("trunc", C.c_float), ("max_weight", C.c_float)]


class TsdfIntegrateArgs(C.Structure):                     # nalo_tsdf_integrate_args
    _fields_ = [("depth", DevPlane), ("K", C.c_float * 4), ("camToWorld", C.c_double * 12), ("min_depth", C.c_float), ("max_depth", C.c_float), ("producer_stream", C.c_void_p)]


class TsdfStats(C.Structure):                             # nalo_tsdf_stats
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("visited", C.c_longlong), ("updated", C.c_longlong)]


class TsdfVolumeView(C.Structure):                        # nalo_tsdf_volume_view
    _fields_ = [("tsdf", C.c_void_p), ("weight", C.c_void_p), ("dims", C.c_int * 3), ("stream", C.c_void_p)]


class TsdfSurfaceArgs(C.Structure):                       # nalo_tsdf_surface_args
    _fields_ = [("use_box", C.c_int), ("lo", C.c_int * 3), ("size", C.c_int * 3), ("min_weight", C.c_float), ("cap", C.c_longlong), ("xyz", c_fp),
                ("n", C.c_longlong), ("n_needed", C.c_longlong)]


class TsdfMeshArgs(C.Structure):                          # nalo_tsdf_mesh_args
    _fields_ = [("use_box", C.c_int), ("lo", C.c_int * 3), ("size", C.c_int * 3), ("min_weight", C.c_float), ("cap_vertices", C.c_longlong), ("cap_triangles", C.c_longlong),
                ("xyz", c_fp), ("tri", c_ip), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong)]


class TsdfMeshDev(C.Structure):                           # nalo_tsdf_mesh_dev
    _fields_ = [("xyz", C.c_void_p), ("tri", C.c_void_p), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong), ("stream", C.c_void_p)]


class TsdfColorVolumeView(C.Structure):                   # nalo_tsdf_color_volume_view
    _fields_ = [("bgr", C.c_void_p), ("dims", C.c_int * 3), ("stream", C.c_void_p)]


class TsdfMeshColorArgs(C.Structure):                     # nalo_tsdf_mesh_color_args
    _fields_ = [("cap", C.c_longlong), ("rgba", c_u8p)]


class TsdfMeshColorDev(C.Structure):                      # nalo_tsdf_mesh_color_dev
    _fields_ = [("rgba", C.c_void_p), ("n_vertices", C.c_longlong), ("stream", C.c_void_p)]


class TsdfRaycastArgs(C.Structure):                       # nalo_tsdf_raycast_args
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("K", C.c_float * 4), ("camToWorld", C.c_double * 12), ("min_depth", C.c_float), ("max_depth", C.c_float), ("step", C.c_float),
                ("min_weight", C.c_float), ("with_normals", C.c_int), ("with_colour", C.c_int), ("depth", c_fp), ("normal", c_fp), ("rgba", c_u8p),
                ("n_hit", C.c_longlong), ("n_back", C.c_longlong), ("n_normal", C.c_longlong), ("n_steps", C.c_int)]


class TsdfRaycastDev(C.Structure):                        # nalo_tsdf_raycast_dev
    _fields_ = [("depth", DevPlane), ("normal", DevPlane), ("rgba", DevPlane), ("w", C.c_int), ("h", C.c_int), ("stream", C.c_void_p)]


class TsdfAlignEst(C.Structure):                          # nalo_tsdf_align_est
    _fields_ = [("camToWorld", C.c_double * 12), ("s", C.c_double)]


class TsdfAlignArgs(C.Structure):                         # nalo_tsdf_align_args
    _fields_ = [("depth", DevPlane), ("K", C.c_float * 4), ("min_depth", C.c_float), ("max_depth", C.c_float), ("min_weight", C.c_float), ("huber", C.c_float),
                ("step", C.c_int), ("dof", C.c_int), ("producer_stream", C.c_void_p), ("records", C.c_void_p), ("records_cap", C.c_longlong),
                ("max_iterations", C.c_int), ("min_used", C.c_int), ("lambda0", C.c_double), ("eps", C.c_double)]


class TsdfAlignSums(C.Structure):                         # nalo_tsdf_align_sums
    _fields_ = [("H", C.c_double * 28), ("b", C.c_double * 7), ("E", C.c_double), ("rr", C.c_double), ("count", C.c_longlong * 4)]


class TsdfAlignTrace(C.Structure):                        # nalo_tsdf_align_trace
    _fields_ = [("est", TsdfAlignEst), ("lambda_", C.c_double), ("E", C.c_double), ("count", C.c_longlong * 4), ("accepted", C.c_int)]


class TsdfAlignResult(C.Structure):                       # nalo_tsdf_align_result
    _fields_ = [("est", TsdfAlignEst), ("status", C.c_int), ("iterations", C.c_int), ("evaluations", C.c_int), ("E_first", C.c_double), ("E_last", C.c_double),
                ("n_first", C.c_longlong), ("n_last", C.c_longlong), ("last", TsdfAlignSums), ("trace", C.POINTER(TsdfAlignTrace)), ("trace_cap", C.c_int),
                ("n_trace", C.c_int)]


ALIGN_CONVERGED, ALIGN_ITERATION_LIMIT, ALIGN_TOO_FEW, ALIGN_SOLVE_FAILED = 0, 1, 2, 3      # NALO_TSDF_ALIGN_*
ALIGN_MAX_EVALUATIONS = 65                               # the first evaluation and one per iteration, at most 64 of them


class TsdfSide(C.Structure):                              # nalo_tsdf_side; tsdf_side() builds one
    _fields_ = [("depth", DevPlane), ("colour", DevPlane), ("colour_is_rgb", C.c_int), ("K", C.c_float * 4), ("est", TsdfAlignEst), ("min_depth", C.c_float), ("max_depth", C.c_float)]


class TsdfReplaceArgs(C.Structure):                       # nalo_tsdf_replace_args
    _fields_ = [("remove", C.POINTER(TsdfSide)), ("add", C.POINTER(TsdfSide)), ("use_box", C.c_int), ("lo", C.c_int * 3), ("size", C.c_int * 3), ("producer_stream", C.c_void_p)]


class TsdfReplaceStats(C.Structure):                      # nalo_tsdf_replace_stats
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("visited", C.c_longlong), ("removed", C.c_longlong), ("reset", C.c_longlong), ("added", C.c_longlong),
                ("written", C.c_longlong)]


class TsdfLogEntry(C.Structure):                          # nalo_tsdf_log_entry
    _fields_ = [("frame_id", C.c_int), ("n_records", C.c_int), ("est", TsdfAlignEst), ("K", C.c_float * 4), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("lo", C.c_int * 3), ("size", C.c_int * 3), ("coloured", C.c_int)]


class TsdfReplacePairStats(C.Structure):                  # nalo_tsdf_replace_pair_stats
    _fields_ = [("removed", C.c_longlong), ("reset", C.c_longlong), ("added", C.c_longlong), ("written", C.c_longlong)]


class TsdfReplaceFramesArgs(C.Structure):                 # nalo_tsdf_replace_frames_args; tsdf_replace_frames_args() builds one
    _fields_ = [("n", C.c_int), ("frame_id", c_ip), ("est_new", C.POINTER(TsdfAlignEst)), ("has_est", c_u8p), ("K", C.c_float * 4), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("skip_unchanged", C.c_int), ("n_skipped", C.c_int)]


class TsdfGeometry(C.Structure):                          # struct nalo_tsdf_geometry
    _fields_ = [("desc", TsdfDesc), ("origin0", C.c_float * 3), ("base", C.c_int * 3)]


class TsdfShiftBoxes(C.Structure):                        # struct nalo_tsdf_shift_boxes
    _fields_ = [("n_boxes", C.c_int), ("lo", (C.c_int * 3) * 3), ("size", (C.c_int * 3) * 3), ("kept_lo", C.c_int * 3), ("kept_size", C.c_int * 3)]


class TsdfArchiveStats(C.Structure):                      # struct nalo_tsdf_archive_stats
    _fields_ = [("added_vertices", C.c_longlong), ("welded_vertices", C.c_longlong), ("added_triangles", C.c_longlong), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong),
                ("cap_vertices", C.c_longlong), ("cap_triangles", C.c_longlong), ("table_slots", C.c_longlong), ("coloured", C.c_int), ("have_lattice", C.c_int),
                ("origin0", C.c_float * 3), ("voxel_size", C.c_float)]


class TsdfArchiveGetArgs(C.Structure):                    # nalo_tsdf_archive_get_args
    _fields_ = [("cap_vertices", C.c_longlong), ("cap_triangles", C.c_longlong), ("cap_rgba", C.c_longlong), ("cap_key", C.c_longlong),
                ("xyz", c_fp), ("tri", c_ip), ("rgba", c_u8p), ("key", c_ip), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong)]


class TsdfArchiveDev(C.Structure):                        # nalo_tsdf_archive_dev
    _fields_ = [("xyz", C.c_void_p), ("tri", C.c_void_p), ("rgba", C.c_void_p), ("key", C.c_void_p), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong), ("stream", C.c_void_p)]


class TsdfFollowStats(C.Structure):                       # nalo_tsdf_follow_stats
    _fields_ = [("n_boxes", C.c_int), ("added_vertices", C.c_longlong), ("welded_vertices", C.c_longlong), ("added_triangles", C.c_longlong), ("n_vertices", C.c_longlong),
                ("n_triangles", C.c_longlong)]


class DepthImageArgs(C.Structure):
    """nalo_depth_image_args (include/nalo_gpu.h)"""
    _fields_ = [("minmax_io", c_fp), ("bgr", c_u8p), ("idepth", c_fp), ("n_positive", C.c_int), ("min_new", C.c_float), ("max_new", C.c_float),
                ("min_used", C.c_float), ("max_used", C.c_float)]


class WindowPlotArgs(C.Structure):
    """nalo_window_plot_args (include/nalo_gpu.h)"""
    _fields_ = [("mode", C.c_int), ("rainbow_scale", C.c_float), ("quality_scale", C.c_float), ("frame_mask", C.c_uint), ("minmax_io", c_fp), ("bgr", c_u8p),
                ("n_frames", C.c_int), ("frame_id", C.c_int * 16), ("sources", (C.c_int * 4) * 16), ("n_values", C.c_int), ("min_new", C.c_float), ("max_new", C.c_float),
                ("min_used", C.c_float), ("max_used", C.c_float)]


class ResidualPlotArgs(C.Structure):
    """nalo_residual_plot_args (include/nalo_gpu.h)"""
    _fields_ = [("host", C.c_int), ("free_debug_param5", C.c_float), ("rainbow_scale", C.c_float), ("frame_mask", C.c_uint), ("bgr", c_u8p), ("n_frames", C.c_int),
                ("frame_id", C.c_int * 16), ("aff", (C.c_double * 2) * 16), ("n_points", C.c_int), ("n_residuals", C.c_int), ("n_pattern_pixels", C.c_int)]


class InitPlotArgs(C.Structure):
    """nalo_init_plot_args (include/nalo_gpu.h)"""
    _fields_ = [("lvl", C.c_int), ("rainbow_scale", C.c_float), ("bgr", c_u8p), ("w", C.c_int), ("h", C.c_int), ("n_points", C.c_int), ("n_good", C.c_int),
                ("sum_iR", C.c_float), ("fac", C.c_float)]


class ViewFrame(C.Structure):
    """nalo_view_frame (include/nalo_gpu.h)"""
    _fields_ = [("frame_id", C.c_int), ("camToWorld", C.c_double * 12)]


class MapRenderArgs(C.Structure):
    """nalo_map_render_args (include/nalo_gpu.h)"""
    _fields_ = [("vw", C.c_int), ("vh", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("viewFromWorld", C.c_double * 12), ("n_frames", C.c_int), ("frames", C.POINTER(ViewFrame)), ("display_mode", C.c_int), ("with_immature", C.c_int),
                ("sparsity", C.c_int), ("scaledTH", C.c_float), ("absTH", C.c_float), ("minRelBS", C.c_float), ("with_dense", C.c_int), ("show_kf_cams", C.c_int),
                ("show_current_cam", C.c_int), ("currentCamToWorld", C.c_double * 12), ("show_active_constraints", C.c_int), ("show_all_constraints", C.c_int),
                ("show_trajectory", C.c_int), ("show_full_trajectory", C.c_int), ("n_all_poses", C.c_int), ("all_poses", c_fp), ("background", C.c_uint8 * 3),
                ("rgb", c_u8p), ("depth", c_fp), ("n_vertices", C.c_longlong), ("n_drawn_points", C.c_longlong), ("n_segments", C.c_longlong),
                ("n_line_samples", C.c_longlong)]


class RenderMeshSrc(C.Structure):
    """nalo_render_mesh_src (include/nalo_gpu.h)"""
    _fields_ = [("xyz", C.c_void_p), ("tri", C.c_void_p), ("rgba", C.c_void_p), ("n_vertices", C.c_longlong), ("n_triangles", C.c_longlong), ("producer_stream", C.c_void_p)]


class MapRenderMeshArgs(C.Structure):
    """nalo_map_render_mesh_args (include/nalo_gpu.h)"""
    _fields_ = [("with_archive", C.c_int), ("with_live_mesh", C.c_int), ("user", C.POINTER(RenderMeshSrc)), ("colour_mode", C.c_int), ("max_box_pixels", C.c_longlong),
                ("n_triangles", C.c_longlong), ("n_tri_bad_index", C.c_longlong), ("n_tri_near", C.c_longlong), ("n_tri_guard", C.c_longlong),
                ("n_tri_degenerate", C.c_longlong), ("n_tri_large", C.c_longlong), ("n_tri_pixels", C.c_longlong)]


MESH_COUNTS = ("n_triangles", "n_tri_bad_index", "n_tri_near", "n_tri_guard", "n_tri_degenerate", "n_tri_large", "n_tri_pixels")

TRK_MAX_TRIES = 64                                        # NALO_TRK_MAX_TRIES


class TrkTryRecord(C.Structure):                          # nalo_trk_try_record
    _fields_ = [("ok", C.c_int), ("taken", C.c_int), ("abort_lvl", C.c_int), ("have_repeated", C.c_int), ("n_evals", C.c_int), ("evals", C.c_int * 5),
                ("lastResiduals", C.c_double * 5), ("flow", C.c_double * 3), ("T", C.c_double * 12), ("aff", C.c_double * 2)]


TRY_RECORD_DTYPE = np.dtype([("ok", np.int32), ("taken", np.int32), ("abort_lvl", np.int32), ("have_repeated", np.int32), ("n_evals", np.int32), ("evals", np.int32, 5),
                             ("lastResiduals", np.float64, 5), ("flow", np.float64, 3), ("T", np.float64, 12), ("aff", np.float64, 2)], align=True)
assert TRY_RECORD_DTYPE.itemsize == C.sizeof(TrkTryRecord)


class TrkTriesArgs(C.Structure):                          # nalo_trk_tries_args
    _fields_ = [("slot_new", C.c_int), ("n_tries", C.c_int), ("coarsestLvl", C.c_int), ("tries", C.POINTER(C.c_double)), ("aff_init", C.c_double * 2),
                ("ref_aff", C.c_double * 2), ("exposures", C.c_float * 2), ("lastCoarseRMSE_io", C.c_double * 5), ("reTrackThreshold", C.c_double),
                ("T", C.c_double * 12), ("aff", C.c_double * 2), ("flow", C.c_double * 3), ("achievedRes", C.c_double * 5),
                ("have_one_good", C.c_int), ("try_iterations", C.c_int), ("winner", C.c_int), ("driver", C.c_int),
                ("records", C.POINTER(TrkTryRecord)), ("records_cap", C.c_int)]


class Settings(C.Structure):
    """nalo_settings (include/nalo_gpu.h)"""
    _fields_ = [("forceAcceptStep", C.c_int), ("affineOptModeA", C.c_double), ("affineOptModeB", C.c_double), ("minOptIterations", C.c_int)]


def lib_path():
    return os.path.join(_HERE, "libnalo_gpu.so")


def constants():
    """{reference name: value} of the constants the library was compiled with (nalo_constants; needs no device)"""
    L = C.CDLL(lib_path())
    L.nalo_constants.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double)]
    n = L.nalo_constants(0, None, None)
    names, vals = (C.c_char_p * n)(), (C.c_double * n)()
    assert L.nalo_constants(n, names, vals) == n
    return {names[i].decode(): vals[i] for i in range(n)}


_HOST_LIB = None


def host_lib():
    """the library for its context-free host functions (nalo_ground_*): dlopen only, no device call, works on a machine without a GPU"""
    global _HOST_LIB
    if _HOST_LIB is None:
        L = C.CDLL(lib_path())
        _ground_argtypes(L)
        L.nalo_view_look_at.argtypes = [c_dp, c_dp, c_dp, c_dp]
        L.nalo_view_triangle.argtypes = [C.POINTER(MapRenderArgs), c_fp, C.c_longlong, c_ip, c_ip, c_ip, c_ip]
        L.nalo_trk_motion_tries.argtypes = [c_dp, c_dp, C.c_int, c_dp]
        L.nalo_tsdf_frustum_box.argtypes = [C.POINTER(TsdfDesc), C.c_int, C.c_int, c_fp, c_dp, C.c_float, c_ip, c_ip]
        L.nalo_tsdf_mesh_table.argtypes = [C.c_void_p]
        L.nalo_tsdf_raycast_steps.argtypes = [C.c_float, C.c_float, C.c_float, c_ip]
        L.nalo_tsdf_shift_for.argtypes = [C.POINTER(TsdfDesc), c_dp, c_ip, c_ip]
        L.nalo_tsdf_align_step.argtypes = [c_dp, c_dp, C.c_double, C.c_int, C.POINTER(TsdfAlignEst), c_dp, C.POINTER(TsdfAlignEst)]
        L.nalo_tsdf_shift_boxes.argtypes = [c_ip, c_ip, C.POINTER(TsdfShiftBoxes)]
        L.nalo_tsdf_est_world_to_cam.argtypes = [C.POINTER(TsdfAlignEst), c_fp]
        L.nalo_tsdf_frustum_box_est.argtypes = [C.POINTER(TsdfDesc), C.c_int, C.c_int, c_fp, C.POINTER(TsdfAlignEst), C.c_float, c_ip, c_ip]
        L.nalo_tsdf_box_shift.argtypes = [c_ip, c_ip, c_ip, c_ip]
        L.nalo_tsdf_replace_frames_plan.argtypes = [C.POINTER(TsdfReplaceFramesArgs), C.POINTER(TsdfLogEntry), C.c_int, c_ip, c_u8p]
        L.nalo_io_write_ply_mesh.argtypes = [C.c_char_p, C.c_longlong, c_fp, C.c_longlong, c_ip]
        L.nalo_io_write_ply_mesh_rgba.argtypes = [C.c_char_p, C.c_longlong, c_fp, c_u8p, C.c_longlong, c_ip]
        _HOST_LIB = L
    return _HOST_LIB


def trk_motion_tries(slast_2_sprelast, lastF_2_slast, poses_valid=True):
    """nalo_trk_motion_tries: trackNewCoarse's hypothesis list (FullSystem.cpp:535-579) as [n, 3, 4], n = 31, or the single identity when a pose is not valid;
    needs no device"""
    out = np.zeros(31 * 12)
    a, b = (np.ascontiguousarray(x, np.float64).reshape(-1) for x in (slast_2_sprelast, lastF_2_slast))
    assert a.size == 12 and b.size == 12
    n = host_lib().nalo_trk_motion_tries(_d(a), _d(b), int(bool(poses_valid)), _d(out))
    if n < 0:
        raise NaloError("nalo_trk_motion_tries: error %d" % n)
    return out[:12 * n].reshape(n, 3, 4).copy()


def view_look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0)):
    """nalo_view_look_at: pangolin::ModelViewLookAt as viewFromWorld [3][4] (x right, y down, z forward) for map_render; needs no device. The viewer starts at
    eye (0, -5, -10)"""
    e, t, u = (np.ascontiguousarray(x, np.float64).reshape(3) for x in (eye, target, up))
    out = np.zeros(12, np.float64)
    if host_lib().nalo_view_look_at(e.ctypes.data_as(c_dp), t.ctypes.data_as(c_dp), u.ctypes.data_as(c_dp), out.ctypes.data_as(c_dp)) != 0:
        raise NaloError("nalo_view_look_at: degenerate view (up parallel to the viewing direction, eye == target, or a value that is not finite)")
    return out.reshape(3, 4)


def view_triangle(vw, vh, view_xyz, fx=400.0, fy=400.0, cx=None, cy=None, znear=0.1, max_box_pixels=0):
    """nalo_view_triangle: rules 2-5 of nalo_map_render_mesh for one triangle given by its view-space vertices [3][3], through the function the kernel calls ->
    dict(cls 0 drawn or 2..5, X [3], Y [3] snapped coordinates after the exchange, box (x0, x1, y0, y1), x1 < x0 when empty); needs no device"""
    a = MapRenderArgs()
    a.vw, a.vh, a.fx, a.fy, a.znear = int(vw), int(vh), float(fx), float(fy), float(znear)
    a.cx, a.cy = float(vw / 2 if cx is None else cx), float(vh / 2 if cy is None else cy)
    P = np.ascontiguousarray(view_xyz, np.float32).reshape(9)
    cls, X, Y, box = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(4, np.int32)
    rc = host_lib().nalo_view_triangle(C.byref(a), _f(P), int(max_box_pixels), _i(cls), _i(X), _i(Y), _i(box))
    if rc != 0:
        raise NaloError("nalo_view_triangle: bad argument (%d)" % rc)
    return dict(cls=int(cls[0]), X=X.tolist(), Y=Y.tolist(), box=tuple(box.tolist()))


def tsdf_desc(origin, voxel_size, dims, trunc, max_weight):
    """nalo_tsdf_desc (a TsdfDesc): origin = world position of the corner of voxel (0, 0, 0), dims = (nx, ny, nz)"""
    d = TsdfDesc()
    d.origin[:] = [float(v) for v in origin]
    d.dims[:] = [int(v) for v in dims]
    d.voxel_size, d.trunc, d.max_weight = float(voxel_size), float(trunc), float(max_weight)
    return d


def tsdf_frustum_box(desc, w, h, K, cam_to_world, max_depth):
    """nalo_tsdf_frustum_box: the culling box (lo, hi) of an integration, hi exclusive, all zeros when it is empty; needs no device"""
    Kf = np.ascontiguousarray(K, np.float32).reshape(-1)
    m = np.ascontiguousarray(cam_to_world, np.float64).reshape(-1)
    assert Kf.size == 4 and m.size == 12
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    rc = host_lib().nalo_tsdf_frustum_box(C.byref(desc), int(w), int(h), _f(Kf), _d(m), C.c_float(max_depth), _i(lo), _i(hi))
    if rc != 0:
        raise NaloError("nalo_tsdf_frustum_box: bad argument (%d)" % rc)
    return lo, hi


def tsdf_mesh_table():
    """nalo_tsdf_mesh_table: int8 [6][16][6], for tetrahedron t and sign mask the vertices of up to two triangles in output order, each coded 8 p + (q ^ p), -1
    as padding; needs no device"""
    out = np.zeros((6, 16, 6), np.int8)
    rc = host_lib().nalo_tsdf_mesh_table(out.ctypes.data)
    if rc != 0:
        raise NaloError("nalo_tsdf_mesh_table: error %d" % rc)
    return out


def tsdf_raycast_steps(min_depth, max_depth, step):
    """nalo_tsdf_raycast_steps: N, the number of samples z_n = min_depth + (float)n * step <= max_depth of a ray-cast (1 .. 4096); NaloError for values
    nalo_tsdf_raycast refuses, more than 4096 steps among them. Needs no device"""
    n = np.zeros(1, np.int32)
    rc = host_lib().nalo_tsdf_raycast_steps(C.c_float(min_depth), C.c_float(max_depth), C.c_float(step), _i(n))
    if rc != 0:
        raise NaloError("nalo_tsdf_raycast_steps: bad argument (%d)" % rc)
    return int(n[0])


def tsdf_align_est(cam_to_world, s=1.0):
    """nalo_tsdf_align_est (a TsdfAlignEst): camToWorld [3][4] and the scale"""
    e = TsdfAlignEst()
    m = np.asarray(cam_to_world, np.float64).reshape(-1)
    if m.size != 12:
        raise NaloError("tsdf_align_est: camToWorld is 3 x 4")
    e.camToWorld[:] = [float(v) for v in m]
    e.s = float(s)
    return e


def _align_sums(S):
    return dict(H=np.array(S.H[:], np.float64), b=np.array(S.b[:], np.float64), E=float(S.E), rr=float(S.rr), count=tuple(int(v) for v in S.count))


def _align_est(e):
    return np.array(e.camToWorld[:], np.float64).reshape(3, 4), float(e.s)


def tsdf_align_step(H, b, lam, dof, cam_to_world, s=1.0):
    """nalo_tsdf_align_step: one Levenberg-Marquardt step in fp64 -> (inc float64 [7], camToWorld [3][4], s). H is the 28 entries of the upper triangle, row-major.
    NaloError for a system that is not finite or not positive definite. Needs no device"""
    Hh, bb = np.ascontiguousarray(H, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
    if Hh.size != 28 or bb.size != 7:
        raise NaloError("tsdf_align_step: H holds 28 entries, b 7")
    e, out, inc = tsdf_align_est(cam_to_world, s), TsdfAlignEst(), np.zeros(7, np.float64)
    rc = host_lib().nalo_tsdf_align_step(_d(Hh), _d(bb), C.c_double(lam), int(dof), C.byref(e), _d(inc), C.byref(out))
    if rc != 0:
        raise NaloError("nalo_tsdf_align_step: refused (%d)" % rc)
    return (inc,) + _align_est(out)


def tsdf_shift_for(desc, centre, margin=(0, 0, 0)):
    """nalo_tsdf_shift_for: the whole-voxel shift (int32 [3]) that puts the voxel containing `centre` at index dims / 2 of the volume `desc` describes (a
    TsdfDesc with the CURRENT origin: tsdf_geometry()["desc"]); an axis whose distance is within margin[a] voxels stays. Needs no device"""
    ce = np.ascontiguousarray(centre, np.float64).reshape(-1)
    mg = np.ascontiguousarray(margin, np.int32).reshape(-1)
    assert ce.size == 3 and mg.size == 3
    out = np.zeros(3, np.int32)
    rc = host_lib().nalo_tsdf_shift_for(C.byref(desc), _d(ce), _i(mg), _i(out))
    if rc != 0:
        raise NaloError("nalo_tsdf_shift_for: bad argument (%d)" % rc)
    return out


def tsdf_shift_boxes(dims, shift):
    """nalo_tsdf_shift_boxes -> dict(boxes=[(lo, size), ...], kept_lo, kept_size): the sub-boxes of the volume BEFORE tsdf_shift(shift) whose meshes (or surface
    points, or blocks) hold every cell the shift loses, in the header's order; kept_*: the voxels that stay, zeros when none does. Needs no device"""
    dm = np.ascontiguousarray(dims, np.int32).reshape(-1)
    sh = np.ascontiguousarray(shift, np.int32).reshape(-1)
    assert dm.size == 3 and sh.size == 3
    b = TsdfShiftBoxes()
    rc = host_lib().nalo_tsdf_shift_boxes(_i(dm), _i(sh), C.byref(b))
    if rc != 0:
        raise NaloError("nalo_tsdf_shift_boxes: bad argument (%d)" % rc)
    return dict(boxes=[(tuple(b.lo[k]), tuple(b.size[k])) for k in range(b.n_boxes)], kept_lo=tuple(b.kept_lo), kept_size=tuple(b.kept_size))


def tsdf_est_world_to_cam(cam_to_world, s=1.0):
    """nalo_tsdf_est_world_to_cam -> float32 [3][4]: R^T / s and -(R^T t) / s of an estimate; for s = 1 the integration's worldToCam bit for bit. NaloError for
    a non-finite pose, or an s that is not finite or <= 0. Needs no device"""
    e, M = tsdf_align_est(cam_to_world, s), np.zeros(12, np.float32)
    rc = host_lib().nalo_tsdf_est_world_to_cam(C.byref(e), _f(M))
    if rc != 0:
        raise NaloError("nalo_tsdf_est_world_to_cam: bad argument (%d)" % rc)
    return M.reshape(3, 4)


def tsdf_frustum_box_est(desc, w, h, K, cam_to_world, s, max_depth):
    """nalo_tsdf_frustum_box_est: the culling box (lo, hi) of a removal or an add at the estimate (cam_to_world, s), hi exclusive, all zeros when it is empty;
    for s = 1 tsdf_frustum_box's. Needs no device"""
    Kf = np.ascontiguousarray(K, np.float32).reshape(-1)
    assert Kf.size == 4
    e = tsdf_align_est(cam_to_world, s)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    rc = host_lib().nalo_tsdf_frustum_box_est(C.byref(desc), int(w), int(h), _f(Kf), C.byref(e), C.c_float(max_depth), _i(lo), _i(hi))
    if rc != 0:
        raise NaloError("nalo_tsdf_frustum_box_est: bad argument (%d)" % rc)
    return lo, hi


def tsdf_box_shift(dims, shift, lo, size):
    """nalo_tsdf_box_shift -> (lo, size) int32 [3]: where the voxels of the box [lo, lo + size) lie after tsdf_shift(shift), clipped to the grid; all zeros when
    none is left. Needs no device"""
    dm, sh = np.ascontiguousarray(dims, np.int32).reshape(-1), np.ascontiguousarray(shift, np.int32).reshape(-1)
    l, z = np.array(lo, np.int32).reshape(-1), np.array(size, np.int32).reshape(-1)
    assert dm.size == 3 and sh.size == 3 and l.size == 3 and z.size == 3
    rc = host_lib().nalo_tsdf_box_shift(_i(dm), _i(sh), _i(l), _i(z))
    if rc != 0:
        raise NaloError("nalo_tsdf_box_shift: bad argument (%d)" % rc)
    return l, z


def tsdf_side(depth, K, cam_to_world, s, min_depth, max_depth, colour=None, colour_is_rgb=False):
    """nalo_tsdf_side (a TsdfSide) for tsdf_replace_depth: depth a 2-D float32 device array (or a DevPlane) read where it lies, K = (fx, fy, cx, cy) for ITS
    size, the estimate (cam_to_world [3][4], s), the depth range; colour: a uint8 device array [h][w][3] or a DevPlane of three channels. The side keeps the
    arrays alive; `stream` is the stream of the DEPTH plane alone, as tsdf_integrate_depth works it out (a colour plane from another stream is the caller's
    to order: see tsdf_replace_depth)"""
    sd = TsdfSide()
    sd.depth = depth if isinstance(depth, DevPlane) else dev_plane(depth)
    if colour is not None:
        sd.colour = colour if isinstance(colour, DevPlane) else dev_plane(colour, "hwc")
    sd.colour_is_rgb = int(bool(colour_is_rgb))
    sd.K[:] = [float(v) for v in K]
    sd.est = tsdf_align_est(cam_to_world, s)
    sd.min_depth, sd.max_depth = float(min_depth), float(max_depth)
    sd.keep = (depth, colour)
    sd.stream = 0
    torch = sys.modules.get("torch")
    if isinstance(depth, DeviceView):
        sd.stream = depth.stream
    elif torch is not None and isinstance(depth, torch.Tensor):
        sd.stream = torch.cuda.current_stream(depth.device).cuda_stream
    return sd


def tsdf_replace_frames_args(frame_ids, cam_to_world, K, min_depth, max_depth, s=1.0, skip_unchanged=False):
    """nalo_tsdf_replace_frames_args (a TsdfReplaceFramesArgs): frame_ids a list of ints; cam_to_world a list of [3][4] poses, None in it for a frame that is
    removed only, or None for the whole list (every frame removed only); s a scale or a list of them. The struct keeps its arrays alive. n may be anything:
    the library refuses what it refuses"""
    a = TsdfReplaceFramesArgs()
    n = len(frame_ids)
    ids = np.ascontiguousarray(frame_ids, np.int32).reshape(-1)
    a.n, a.frame_id = n, _i(ids) if n else None
    a.keep = [ids]
    if cam_to_world is not None:
        assert len(cam_to_world) == n
        ss = list(s) if np.ndim(s) else [s] * n
        est = (TsdfAlignEst * max(n, 1))()
        has = np.zeros(max(n, 1), np.uint8)
        for k, m in enumerate(cam_to_world):
            if m is not None:
                est[k], has[k] = tsdf_align_est(m, ss[k]), 1
        a.est_new, a.has_est = est, has.ctypes.data_as(c_u8p)
        a.keep += [est, has]
    a.K[:] = [float(v) for v in K]
    a.min_depth, a.max_depth, a.skip_unchanged = float(min_depth), float(max_depth), int(bool(skip_unchanged))
    return a


def tsdf_log_entry(frame_id, n_records, cam_to_world, s, K, min_depth, max_depth, lo=(0, 0, 0), size=(1, 1, 1), coloured=False):
    """a nalo_tsdf_log_entry (a TsdfLogEntry) built by hand, for tsdf_replace_frames_plan"""
    e = TsdfLogEntry()
    e.frame_id, e.n_records, e.est = int(frame_id), int(n_records), tsdf_align_est(cam_to_world, s)
    e.K[:] = [float(v) for v in K]
    e.min_depth, e.max_depth, e.coloured = float(min_depth), float(max_depth), int(bool(coloured))
    e.lo[:], e.size[:] = [int(v) for v in lo], [int(v) for v in size]
    return e


def tsdf_replace_frames_plan(args, log, list_len):
    """nalo_tsdf_replace_frames_plan, host only: the list's own checks and skip_unchanged's predicate. args: tsdf_replace_frames_args(); log: a list of
    TsdfLogEntry; list_len: the length of each frame's dense list now, or None. Returns the skip flags as a list of bools; raises NaloError on a refusal"""
    arr = (TsdfLogEntry * max(len(log), 1))(*log)
    ll = None if list_len is None else np.ascontiguousarray(list_len, np.int32)
    skip = np.zeros(64, np.uint8)
    rc = host_lib().nalo_tsdf_replace_frames_plan(C.byref(args), arr, len(log), None if ll is None else _i(ll), skip.ctypes.data_as(c_u8p))
    if rc != 0:
        raise NaloError("nalo_tsdf_replace_frames_plan: bad argument (%d)" % rc)
    return [bool(v) for v in skip[:args.n]]


def write_ply_mesh(path, xyz, tri, rgba=None):
    """nalo_io_write_ply_mesh: xyz float32 [nv][3] and tri int32 [nt][3] as a binary little-endian PLY file; with rgba (uint8 [nv][4], tsdf_mesh's colours)
    nalo_io_write_ply_mesh_rgba: the same file with red, green, blue, alpha behind every vertex. Needs no device"""
    x, t = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    if rgba is None:
        rc, who = host_lib().nalo_io_write_ply_mesh(os.fsencode(path), len(x), _f(x), len(t), _i(t)), "nalo_io_write_ply_mesh"
    else:
        c = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
        if len(c) != len(x):
            raise NaloError("write_ply_mesh: rgba holds %d colours for %d vertices" % (len(c), len(x)))
        rc, who = host_lib().nalo_io_write_ply_mesh_rgba(os.fsencode(path), len(x), _f(x), _u8(c), len(t), _i(t)), "nalo_io_write_ply_mesh_rgba"
    if rc != 0:
        raise NaloError("%s: error %d (-1: an index outside the vertices, -2: the file cannot be written)" % (who, rc))


def _ground_argtypes(L):
    L.nalo_ground_tracker_init.argtypes = [C.POINTER(GroundTracker)]
    L.nalo_ground_globals_init.argtypes = [C.POINTER(GroundGlobals)]
    L.nalo_ground_frame_init.argtypes = [C.POINTER(GroundFrame)]
    for f in (L.nalo_ground_tracker_init, L.nalo_ground_globals_init, L.nalo_ground_frame_init):
        f.restype = None
    L.nalo_ground_update.argtypes = [C.POINTER(GroundPick), C.POINTER(GroundTracker), C.POINTER(GroundGlobals), C.POINTER(GroundFrame), C.c_int]
    L.nalo_ground_set_global_plane.argtypes = [C.POINTER(GroundFrame), C.c_int, C.c_int, c_dp, c_dp, c_dp, c_fp]
    L.nalo_ground_local_scale.argtypes = [C.POINTER(GroundFrame), C.c_float, c_dp]
    L.nalo_ground_reset_global_plane.argtypes = [C.POINTER(GroundFrame), C.c_int, c_dp, c_dp]


def ground_tracker():
    t = GroundTracker()
    host_lib().nalo_ground_tracker_init(C.byref(t))
    return t


def ground_globals():
    g = GroundGlobals()
    host_lib().nalo_ground_globals_init(C.byref(g))
    return g


def ground_frames(W):
    """W zeroed nalo_ground_frame, as a ctypes array (window order)"""
    fr = (GroundFrame * int(W))()
    for f in fr:
        host_lib().nalo_ground_frame_init(C.byref(f))
    return fr


def ground_update(pick, tracker, globals_, frames):
    """nalo_ground_update on the caller's structs, in place (CoarseTracker.cpp:609-616, 696-816)"""
    rc = host_lib().nalo_ground_update(C.byref(pick), C.byref(tracker), C.byref(globals_), frames, len(frames))
    if rc != 0:
        raise NaloError("nalo_ground_update: %d" % rc)


def ground_set_global_plane(frames, worldToCam_frame1, max_frames=7):
    """FullSystem::setglobalplane -> (fixed, gplane[4], backup_gplane[4], lgh); the outputs are None when it did not fix"""
    gp, bk, lgh = np.zeros(4), np.zeros(4), np.zeros(1, np.float32)
    M = np.ascontiguousarray(worldToCam_frame1, np.float64).reshape(-1)
    rc = host_lib().nalo_ground_set_global_plane(frames, len(frames), int(max_frames), _d(M), _d(gp), _d(bk), _f(lgh))
    if rc < 0:
        raise NaloError("nalo_ground_set_global_plane: %d" % rc)
    return (True, gp, bk, np.float32(lgh[0])) if rc == 1 else (False, None, None, None)


def ground_local_scale(frame, lgh):
    """PlaneOptimize.cpp:203-211 -> localscale (a Python float, the C double) or None when the frame has no ground"""
    out = np.zeros(1)
    rc = host_lib().nalo_ground_local_scale(C.byref(frame), C.c_float(lgh), _d(out))
    if rc < 0:
        raise NaloError("nalo_ground_local_scale: %d" % rc)
    return float(out[0]) if rc == 1 else None


def ground_reset_global_plane(frames, worldToCam):
    """FullSystem::resetGlobalPlane -> (index of the frame used or -1, gplane[4])"""
    gp = np.zeros(4)
    M = np.ascontiguousarray(worldToCam, np.float64).reshape(-1)
    return int(host_lib().nalo_ground_reset_global_plane(frames, len(frames), _d(M), _d(gp))), gp


def load():
    """dlopen the in-tree library; raises if it has not been built (python nalo-slam_amd/build.py)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise RuntimeError("libnalo_gpu.so is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); no CPU fallback exists")
    L = C.CDLL(p)
    vp = C.c_void_p
    L.nalo_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, c_fp, C.c_int]
    L.nalo_destroy.argtypes = [vp]
    L.nalo_destroy.restype = None
    L.nalo_last_error.argtypes = [vp]
    L.nalo_last_error.restype = C.c_char_p
    L.nalo_levels.argtypes = [vp]
    L.nalo_sync.argtypes = [vp]
    L.nalo_stream.argtypes = [vp]
    L.nalo_stream.restype = vp
    L.nalo_test_inject.argtypes = [vp, C.c_int, C.c_int]
    L.nalo_frame_upload.argtypes = [vp, C.c_int, c_fp, c_fp, c_u8p, c_fp]
    L.nalo_frame_upload_async.argtypes = [vp, C.c_int, c_fp, c_fp, c_u8p, c_fp]
    L.nalo_frame_wait.argtypes = [vp, C.c_int]
    L.nalo_frame_ingest_device.argtypes = [vp, C.c_int, C.POINTER(FrameIngestArgs)]
    L.nalo_frame_release.argtypes = [vp, C.c_int, vp]
    L.nalo_dev_plane_check.argtypes = [vp, C.POINTER(DevPlane)]
    L.nalo_frame_attach.argtypes = [vp, C.c_int, c_u8p, c_u8p]
    L.nalo_host_alloc.argtypes = [C.c_size_t]
    L.nalo_host_alloc.restype = vp
    L.nalo_host_free.argtypes = [vp]
    L.nalo_host_free.restype = None
    L.nalo_frame_rebuild.argtypes = [vp, C.c_int]
    L.nalo_frame_download.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp]
    L.nalo_frame_download_mask.argtypes = [vp, C.c_int, c_fp, c_u8p]
    L.nalo_trk_make_k.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
    L.nalo_trk_set_ref.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_fp]
    L.nalo_trk_ref_upload.argtypes = [vp, C.c_int, c_fp, c_fp, c_fp, c_fp]
    L.nalo_trk_set_ref_resident.argtypes = [vp, C.c_int]
    L.nalo_trk_set_ref_from_window.argtypes = [vp]
    L.nalo_trk_set_ref_from_depth.argtypes = [vp, C.c_int, C.POINTER(TrkDepthRefArgs)]
    L.nalo_trk_set_pc.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_fp]
    L.nalo_trk_get_pc.argtypes = [vp, C.c_int, c_ip, c_fp, c_fp, c_fp, c_fp]
    L.nalo_trk_get_depth.argtypes = [vp, C.c_int, c_fp, c_fp]
    L.nalo_trk_set_depth.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp]
    L.nalo_frame_plane.argtypes = [vp, C.c_int, C.c_int, C.POINTER(DevPlane)]
    L.nalo_trk_ref_export.argtypes = [vp, C.POINTER(TrkRefView)]
    L.nalo_trk_ref_import.argtypes = [vp, C.c_int, C.POINTER(TrkRefView)]
    L.nalo_trk_ref_release.argtypes = [vp, vp]
    L.nalo_trk_depth_image.argtypes = [vp, C.POINTER(DepthImageArgs)]
    L.nalo_trk_eval.argtypes = [vp, C.c_int, C.c_int, c_dp, c_dp, c_fp, C.c_float, C.c_float, C.c_int, c_dp, c_dp, c_dp]
    L.nalo_trk_track_tries.argtypes = [vp, C.POINTER(TrkTriesArgs)]
    L.nalo_trk_track.argtypes = [vp, C.c_int, c_dp, c_dp, c_dp, c_fp, C.c_int, c_dp, c_dp, c_dp, c_ip, c_ip]
    L.nalo_ba_set_window.argtypes = [vp, C.c_int, C.POINTER(FrameState), c_dp, c_dp]
    L.nalo_ba_set_points.argtypes = [vp, C.c_int, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip]
    L.nalo_ba_set_residuals.argtypes = [vp, c_u8p]
    L.nalo_ba_set_prior.argtypes = [vp, c_dp, c_dp]
    L.nalo_ba_get_prior.argtypes = [vp, c_dp, c_dp]
    L.nalo_ba_linearize.argtypes = [vp, C.c_int, c_dp]
    L.nalo_ba_accumulate.argtypes = [vp, C.c_int, c_dp, c_dp]
    L.nalo_ba_accumulate_sc.argtypes = [vp, C.c_int, c_dp, c_dp]
    L.nalo_ba_solve_system.argtypes = [vp, C.c_int, C.c_double, c_dp]
    L.nalo_ba_backup_state.argtypes = [vp]
    L.nalo_ba_do_step.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_ip]
    L.nalo_ba_optimize.argtypes = [vp, C.c_int, C.c_int, c_dp]
    L.nalo_ba_marginalize_points.argtypes = [vp, c_u8p, c_dp, c_dp, c_dp, c_dp]
    L.nalo_ba_marginalize_frame.argtypes = [vp, C.c_int]
    L.nalo_ba_set_point_history.argtypes = [vp, c_ip, c_i8p, c_i8p]
    L.nalo_ba_get_point_history.argtypes = [vp, c_ip, c_i8p, c_i8p]
    L.nalo_ba_flag_points.argtypes = [vp, c_u8p, c_u8p, c_fp, c_ip]
    L.nalo_ba_marginalize_flagged.argtypes = [vp, c_dp, c_dp, c_dp, c_dp]
    L.nalo_ba_get_frames.argtypes = [vp, C.POINTER(FrameState), c_dp, c_dp]
    L.nalo_ba_carry_window.argtypes = [vp, C.POINTER(FrameState), C.c_int]
    L.nalo_ba_carry_map.argtypes = [vp, c_ip]
    L.nalo_ba_carry_last.argtypes = [vp, c_ip]
    L.nalo_ba_window_from_initializer.argtypes = [vp, C.POINTER(InitWindowArgs)]
    L.nalo_ba_init_window_map.argtypes = [vp, c_ip]
    L.nalo_ba_init_window_last.argtypes = [vp, c_fp, c_ip]
    L.nalo_map_enable.argtypes = [vp, C.c_int, C.c_int]
    L.nalo_map_reset.argtypes = [vp]
    L.nalo_map_counts.argtypes = [vp, C.c_int, c_ip]
    L.nalo_map_get_frame.argtypes = [vp, C.c_int, vp, C.c_int, c_ip]
    L.nalo_map_world_points.argtypes = [vp, C.c_int, c_dp, c_dp, C.c_int, c_ip]
    L.nalo_map_world_points_host.argtypes = [C.c_int, c_fp, c_fp, c_fp, c_fp, c_dp, c_dp]
    L.nalo_map_frame_cloud.argtypes = [vp, C.POINTER(MapCloudArgs)]
    L.nalo_map_render.argtypes = [vp, C.POINTER(MapRenderArgs)]
    L.nalo_map_render_mesh.argtypes = [vp, C.POINTER(MapRenderArgs), C.POINTER(MapRenderMeshArgs)]
    L.nalo_view_look_at.argtypes = [c_dp, c_dp, c_dp, c_dp]
    L.nalo_map_graph_enable.argtypes = [vp, C.c_int]
    L.nalo_map_graph.argtypes = [vp, vp, C.c_int, c_ip]
    L.nalo_map_graph_connections.argtypes = [vp, vp, C.c_int, c_ip]
    L.nalo_map_window_plot.argtypes = [vp, C.POINTER(WindowPlotArgs)]
    L.nalo_dense_update_map.argtypes = [vp, C.c_int, C.POINTER(PlaneFitArgs), c_dp, C.c_int, vp, vp, c_ip, c_ip]
    L.nalo_map_dense_enable.argtypes = [vp, C.c_int, C.c_int]
    L.nalo_map_dense_counts.argtypes = [vp, C.c_int, c_ip, c_ip]
    L.nalo_map_dense_get.argtypes = [vp, C.c_int, vp, C.c_int, c_ip]
    L.nalo_map_dense_world_points.argtypes = [vp, C.c_int, c_dp, c_dp, C.c_int, c_ip]
    L.nalo_map_dense_cloud.argtypes = [vp, C.POINTER(MapDenseCloudArgs)]
    L.nalo_tsdf_create.argtypes = [vp, C.POINTER(TsdfDesc)]
    L.nalo_tsdf_reset.argtypes = [vp]
    L.nalo_tsdf_destroy.argtypes = [vp]
    L.nalo_tsdf_integrate_depth.argtypes = [vp, C.POINTER(TsdfIntegrateArgs)]
    L.nalo_tsdf_release.argtypes = [vp, vp]
    L.nalo_tsdf_integrate_frame.argtypes = [vp, C.c_int, c_dp, c_fp, C.c_float, C.c_float]
    L.nalo_tsdf_last.argtypes = [vp, C.POINTER(TsdfStats)]
    L.nalo_tsdf_get.argtypes = [vp, c_ip, c_ip, c_fp, c_fp]
    L.nalo_tsdf_set.argtypes = [vp, c_ip, c_ip, c_fp, c_fp]
    L.nalo_tsdf_view.argtypes = [vp, C.POINTER(TsdfVolumeView)]
    L.nalo_tsdf_surface_points.argtypes = [vp, C.POINTER(TsdfSurfaceArgs)]
    L.nalo_tsdf_mesh.argtypes = [vp, C.POINTER(TsdfMeshArgs)]
    L.nalo_tsdf_mesh_view.argtypes = [vp, C.POINTER(TsdfMeshDev)]
    L.nalo_tsdf_mesh_table.argtypes = [C.c_void_p]
    L.nalo_tsdf_color_enable.argtypes = [vp]
    L.nalo_tsdf_color_disable.argtypes = [vp]
    L.nalo_tsdf_integrate_depth_color.argtypes = [vp, C.POINTER(TsdfIntegrateArgs), C.POINTER(DevPlane), C.c_int]
    L.nalo_tsdf_color_get.argtypes = [vp, c_ip, c_ip, c_fp]
    L.nalo_tsdf_color_set.argtypes = [vp, c_ip, c_ip, c_fp]
    L.nalo_tsdf_color_view.argtypes = [vp, C.POINTER(TsdfColorVolumeView)]
    L.nalo_tsdf_mesh_color.argtypes = [vp, C.POINTER(TsdfMeshArgs), C.POINTER(TsdfMeshColorArgs)]
    L.nalo_tsdf_mesh_color_view.argtypes = [vp, C.POINTER(TsdfMeshColorDev)]
    L.nalo_tsdf_raycast.argtypes = [vp, C.POINTER(TsdfRaycastArgs)]
    L.nalo_tsdf_raycast_view.argtypes = [vp, C.POINTER(TsdfRaycastDev)]
    L.nalo_tsdf_raycast_steps.argtypes = [C.c_float, C.c_float, C.c_float, c_ip]
    L.nalo_tsdf_align_eval.argtypes = [vp, C.POINTER(TsdfAlignArgs), C.POINTER(TsdfAlignEst), C.POINTER(TsdfAlignSums)]
    L.nalo_tsdf_align_depth.argtypes = [vp, C.POINTER(TsdfAlignArgs), C.POINTER(TsdfAlignEst), C.POINTER(TsdfAlignResult)]
    L.nalo_tsdf_align_frame.argtypes = [vp, C.c_int, C.POINTER(TsdfAlignArgs), C.POINTER(TsdfAlignEst), C.POINTER(TsdfAlignResult)]
    L.nalo_tsdf_align_step.argtypes = [c_dp, c_dp, C.c_double, C.c_int, C.POINTER(TsdfAlignEst), c_dp, C.POINTER(TsdfAlignEst)]
    L.nalo_tsdf_shift.argtypes = [vp, c_ip]
    L.nalo_tsdf_geometry.argtypes = [vp, C.POINTER(TsdfGeometry)]
    L.nalo_tsdf_frustum_box.argtypes = [C.POINTER(TsdfDesc), C.c_int, C.c_int, c_fp, c_dp, C.c_float, c_ip, c_ip]
    L.nalo_tsdf_replace_depth.argtypes = [vp, C.POINTER(TsdfReplaceArgs)]
    L.nalo_tsdf_replace_last.argtypes = [vp, C.POINTER(TsdfReplaceStats)]
    L.nalo_tsdf_replace_frame.argtypes = [vp, C.c_int, C.POINTER(TsdfAlignEst), c_fp, C.c_float, C.c_float]
    L.nalo_tsdf_replace_depth_n.argtypes = [vp, C.POINTER(TsdfReplaceArgs), C.c_int]
    L.nalo_tsdf_replace_last_n.argtypes = [vp, C.POINTER(TsdfReplaceStats), C.POINTER(TsdfReplacePairStats), C.c_int, c_ip]
    L.nalo_tsdf_replace_frames.argtypes = [vp, C.POINTER(TsdfReplaceFramesArgs)]
    L.nalo_tsdf_log_enable.argtypes = [vp, C.c_int]
    L.nalo_tsdf_log_get.argtypes = [vp, C.POINTER(TsdfLogEntry), C.c_int, c_ip]
    L.nalo_tsdf_archive_enable.argtypes = [vp]
    L.nalo_tsdf_archive_disable.argtypes = [vp]
    L.nalo_tsdf_archive_reset.argtypes = [vp]
    L.nalo_tsdf_archive_mesh.argtypes = [vp, C.POINTER(TsdfMeshArgs), C.POINTER(TsdfArchiveStats)]
    L.nalo_tsdf_archive_stats.argtypes = [vp, C.POINTER(TsdfArchiveStats)]
    L.nalo_tsdf_archive_get.argtypes = [vp, C.POINTER(TsdfArchiveGetArgs)]
    L.nalo_tsdf_archive_view.argtypes = [vp, C.POINTER(TsdfArchiveDev)]
    L.nalo_tsdf_follow.argtypes = [vp, c_dp, c_ip, C.c_float, c_ip, C.POINTER(TsdfFollowStats)]
    L.nalo_ba_get_points.argtypes = [vp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]
    L.nalo_ba_get_residuals.argtypes = [vp, c_i8p, c_u8p, c_fp, c_fp, c_fp]
    L.nalo_ba_get_acc13.argtypes = [vp, c_dp]
    L.nalo_ba_counts.argtypes = [vp, c_ip, c_ip, c_ip]
    L.nalo_ba_get_launch_config.argtypes = [vp, c_ip]
    L.nalo_ba_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    L.nalo_ba_set_allreduce_mode.argtypes = [vp, C.c_int]
    L.nalo_ba_set_allreduce_side.argtypes = [vp, ALLREDUCE_FN, vp]
    L.nalo_side_stream.argtypes = [vp]
    L.nalo_side_stream.restype = vp
    L.nalo_rccl_unique_id.argtypes = [C.c_char_p]
    L.nalo_ba_rccl_init.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    L.nalo_ba_set_rccl_comm.argtypes = [vp, vp, vp]
    L.nalo_ba_rccl_ranks.argtypes = [vp, c_ip, c_ip]
    L.nalo_shard_points.argtypes = [C.c_int, C.c_int, c_ip, c_fp, c_fp, C.c_int, C.c_int, C.c_int, C.c_int, c_ip]
    L.nalo_ba_snapshot.argtypes = [vp]
    L.nalo_init_calc_res_and_gs.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_fp, c_u8p, c_fp, c_fp, c_dp, c_dp, C.c_float, C.c_float, C.c_float,
                                            c_u8p, c_fp, c_fp, c_fp, c_fp, c_dp, c_dp, c_dp, c_dp, c_dp]
    L.nalo_init_do_step.argtypes = [vp, C.c_int, c_u8p, c_fp, c_fp, c_fp, C.c_float, c_fp, c_fp]
    L.nalo_trk_append_plane_points.argtypes = [vp, c_fp, C.c_float, C.c_int, c_ip, c_ip]
    L.nalo_trk_fit_planes.argtypes = [vp, C.POINTER(PlaneFitArgs), C.c_int, vp, c_ip]
    L.nalo_dense_fit_planes.argtypes = [vp, C.c_int, C.POINTER(PlaneFitArgs), C.c_int, vp, c_ip]
    L.nalo_plane_fit_members.argtypes = [vp, C.c_int, c_ip, c_ip]
    L.nalo_trk_fit_ground.argtypes = [vp, C.POINTER(PlaneFitArgs), C.POINTER(GroundArgs), C.c_int, vp, c_ip, C.POINTER(GroundPick)]
    _ground_argtypes(L)
    L.nalo_undist_set.argtypes = [vp, C.c_int, C.c_int, c_fp, C.c_int, c_fp, C.c_int, c_fp, c_fp]
    L.nalo_frame_upload_raw.argtypes = [vp, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, c_u8p, c_u8p, c_fp]
    L.nalo_frame_upload_raw_async.argtypes = [vp, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, c_fp]
    L.nalo_ba_get_idepth_zero.argtypes = [vp, c_fp]
    L.nalo_ba_calc_l_energy.argtypes = [vp, c_dp]
    L.nalo_ba_plane_scale_fix.argtypes = [vp, C.c_double, c_dp, c_dp]
    L.nalo_ba_sw_gray_optimize.argtypes = [vp, c_dp, c_ip]
    L.nalo_ba_calc_m_energy.argtypes = [vp, c_dp]
    L.nalo_ba_optimize_stats.argtypes = [vp, c_ip, c_ip]
    L.nalo_get_settings.argtypes = [vp, C.POINTER(Settings)]
    L.nalo_set_settings.argtypes = [vp, C.POINTER(Settings)]
    L.nalo_init_set_first.argtypes = [vp, C.c_int, c_ip, c_ip]
    L.nalo_init_track_frame.argtypes = [vp, C.c_int, C.c_float, C.c_float, c_ip]
    L.nalo_init_get_state.argtypes = [vp, c_dp, c_dp, c_ip, c_ip, c_ip, c_ip]
    L.nalo_init_get_points.argtypes = [vp, C.c_int, C.c_int, c_ip, c_fp, c_fp, c_fp, c_fp, c_u8p, c_fp, c_fp, c_fp, c_fp, c_ip, c_fp, c_ip, c_fp]
    L.nalo_trk_last_evals.argtypes = [vp, c_ip, c_ip]
    L.nalo_trk_get_launch_config.argtypes = [vp, c_ip]
    L.nalo_init_set_state.argtypes = [vp, c_dp, c_dp, C.c_int, C.c_int, C.c_int]
    L.nalo_init_set_points.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_u8p, c_fp, c_fp, c_fp, c_fp, c_fp, c_u8p, c_fp]
    L.nalo_init_get_carried.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_fp, c_u8p]
    L.nalo_init_sweep.argtypes = [vp, C.c_int, C.c_int]
    L.nalo_init_depth_image.argtypes = [vp, C.POINTER(InitPlotArgs)]
    L.nalo_ba_get_pattern_projections.argtypes = [vp, c_fp, c_fp]
    L.nalo_ba_residual_plot.argtypes = [vp, C.POINTER(ResidualPlotArgs)]
    L.nalo_pixsel_make_hists.argtypes = [vp, C.c_int, c_fp, c_fp]
    L.nalo_pixsel_set_random.argtypes = [vp, c_u8p, c_ip]
    L.nalo_pixsel_select.argtypes = [vp, C.c_int, C.c_int, C.c_float, c_fp, c_ip]
    L.nalo_pixsel_make_maps.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.c_float, c_ip, c_fp, c_ip]
    L.nalo_pixsel_make_maps_lidar.argtypes = [vp, C.c_int, C.c_float, C.c_int, c_fp, c_ip]
    L.nalo_pixsel_get_selected.argtypes = [vp, C.c_int, c_ip, c_u8p, c_ip]
    L.nalo_dist_make_map.argtypes = [vp, C.c_int, c_fp, c_fp, c_fp]
    L.nalo_imm_create.argtypes = [vp, C.c_int, C.c_int, c_ip, c_ip, c_fp, c_fp, c_fp, c_fp]
    L.nalo_imm_trace.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, C.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp]
    L.nalo_imm_resident_set.argtypes = [vp, C.c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, c_fp, c_fp, c_ip, c_fp]
    L.nalo_imm_resident_trace.argtypes = [vp, C.c_int, C.c_int, c_fp, c_fp, c_fp]
    L.nalo_imm_resident_get.argtypes = [vp, c_fp, c_fp, c_ip, c_fp, c_fp, c_fp]
    L.nalo_imm_optimize.argtypes = [vp, C.c_int, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_int, c_ip, c_fp, c_u8p]
    L.nalo_imm_resident_optimize.argtypes = [vp, C.c_int, c_ip, C.c_int, c_ip, c_fp, c_u8p]
    L.nalo_imm_resident_set_type.argtypes = [vp, c_fp]
    L.nalo_imm_resident_activate.argtypes = [vp, C.c_int, c_fp, c_fp, c_ip, C.c_float, C.c_int, c_ip, c_ip, c_ip, c_ip, c_fp, c_u8p]
    L.nalo_imm_activate_last.argtypes = [vp, c_ip]
    L.nalo_imm_resident_carry.argtypes = [vp, C.POINTER(ImmCarryArgs)]
    L.nalo_imm_resident_carry_map.argtypes = [vp, c_ip]
    L.nalo_imm_resident_carry_last.argtypes = [vp, c_ip]
    L.nalo_imm_resident_get_points.argtypes = [vp, c_ip, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_ip, c_fp]
    L.nalo_ba_restore.argtypes = [vp]
    L.nalo_dense_make_map.argtypes = [vp, C.c_int, c_fp, C.c_float, c_dp, C.c_int, c_ip, c_ip, c_ip, c_fp, c_fp, c_u8p, c_ip, c_ip]
    L.nalo_profile_enable.argtypes = [vp, C.c_int]
    L.nalo_profile_reset.argtypes = [vp]
    L.nalo_profile_select.argtypes = [vp, C.c_char_p]
    L.nalo_profile_get.argtypes = [vp, C.c_char_p, c_dp, c_ip]
    L.nalo_profile_samples.argtypes = [vp, C.c_char_p, c_fp, C.c_int, c_ip]
    L.nalo_profile_sample.argtypes = [vp, C.c_int]
    L.nalo_hbm_calibrate.argtypes = [vp, C.c_size_t, C.c_int, c_dp, c_dp]
    _LIB = L
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(c_fp)


def _d(a):
    return None if a is None else a.ctypes.data_as(c_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(c_ip)


def _u8(a):
    return None if a is None else a.ctypes.data_as(c_u8p)


class NaloError(RuntimeError):
    pass


_TYPESTR_DT = {"<u1": DT_U8, "|u1": DT_U8, "<u2": DT_U16, "<i4": DT_I32, "<f4": DT_F32}


def dev_plane(obj, channels_layout=None):
    """nalo_dev_plane (a DevPlane) of a device array: any object with __cuda_array_interface__ (torch tensors on ROCm have it). Pure host code: data, shape,
    typestr and strides are read, nothing is converted or copied and no library call is made. channels_layout: None for a 2-D (h, w) plane, "hwc" for
    (h, w, 3), "chw" for (3, h, w). strides None means C-contiguous. TypeError for an object without the interface (a numpy array), NaloError for a dtype
    outside the table (u1, u2, i4, f4, little-endian), a shape that does not fit the layout, or negative strides. The plane keeps `obj` alive."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError("dev_plane: %s has no __cuda_array_interface__ (device arrays only: nothing is copied to the device here)" % type(obj).__name__)
    dt = _TYPESTR_DT.get(cai["typestr"])
    if dt is None:
        raise NaloError("dev_plane: typestr %r is outside the table (u1, u2, i4, f4, little-endian); cast on the producer's side" % (cai["typestr"],))
    item = {DT_U8: 1, DT_U16: 2, DT_I32: 4, DT_F32: 4}[dt]
    shape = tuple(int(v) for v in cai["shape"])
    if channels_layout not in (None, "hwc", "chw"):
        raise NaloError("dev_plane: channels_layout is None, 'hwc' or 'chw'")
    if len(shape) != (2 if channels_layout is None else 3):
        raise NaloError("dev_plane: shape %r does not fit channels_layout %r" % (shape, channels_layout))
    strides = cai.get("strides")
    if strides is None:
        strides = [item] * len(shape)
        for k in range(len(shape) - 2, -1, -1):
            strides[k] = strides[k + 1] * shape[k + 1]
    strides = tuple(int(v) for v in strides)
    if len(strides) != len(shape):
        raise NaloError("dev_plane: strides %r do not fit shape %r" % (strides, shape))
    if any(v < 0 for v in strides):
        raise NaloError("dev_plane: negative strides %r (flip on the producer's side)" % (strides,))
    if channels_layout is None:
        (h, w), (sy, sx), ch, sc = shape, strides, 1, 0
    elif channels_layout == "hwc":
        (h, w, ch), (sy, sx, sc) = shape, strides
    else:
        (ch, h, w), (sc, sy, sx) = shape, strides
    if ch not in (1, 3):
        raise NaloError("dev_plane: %d channels (1 or 3)" % ch)
    d = DevPlane(int(cai["data"][0]) or None, dt, w, h, ch, sy, sx, sc)
    d._keep = obj
    return d


class DeviceView:
    """Device memory somebody else owns, as an object with __cuda_array_interface__ (version 2): torch.as_tensor(view) is a zero-copy tensor, dev_plane(view)
    its descriptor. Nothing is copied and nothing is owned: the view is good as long as what it names (include/nalo_gpu.h, "Lifetime of a view"). stream: the
    hipStream_t (an int) whose queued work produces the memory - frame_ingest and trk_ref_import wait for it on the device; a torch consumer on another stream
    waits for it itself. owner: kept alive with the view (the Context)."""

    def __init__(self, ptr, shape, typestr, strides=None, stream=0, owner=None):
        self.ptr, self.shape, self.typestr, self.stream, self.owner = int(ptr or 0), tuple(int(v) for v in shape), typestr, int(stream or 0), owner
        self.strides = None if strides is None else tuple(int(v) for v in strides)
        self.__cuda_array_interface__ = dict(shape=self.shape, typestr=typestr, data=(self.ptr, False), strides=self.strides, version=2)

    @classmethod
    def of_plane(cls, d, stream=0, owner=None):
        """a DevPlane (nalo_frame_plane's) as a view: (h, w) for one channel, (h, w, 3) for interleaved colour; strides are given only where they are not C-contiguous"""
        typestr = {DT_U8: "|u1", DT_U16: "<u2", DT_I32: "<i4", DT_F32: "<f4"}[d.dtype]
        item = int(typestr[2])
        if d.channels == 1:
            shape, strides, dense = (d.h, d.w), (d.stride_y, d.stride_x), (d.w * item, item)
        else:
            shape, strides, dense = (d.h, d.w, d.channels), (d.stride_y, d.stride_x, d.stride_c), (d.w * d.channels * item, d.channels * item, item)
        return cls(d.ptr, shape, typestr, None if tuple(strides) == dense else strides, stream, owner)


def pyr_intrinsics(K, levels):
    """(fx, fy, cx, cy) per level as nalo_create derives them from K (CoarseTracker::makeK, CoarseTracker.cpp:97-141): float32 arrays of `levels` entries"""
    out = np.zeros((4, levels), np.float32)
    out[:, 0] = np.asarray(K, np.float32)
    for l in range(1, levels):
        out[0, l], out[1, l] = np.float32(float(out[0, l - 1]) * 0.5), np.float32(float(out[1, l - 1]) * 0.5)
        out[2, l], out[3, l] = np.float32((float(out[2, 0]) + 0.5) / (1 << l) - 0.5), np.float32((float(out[3, 0]) + 0.5) / (1 << l) - 0.5)
    return out


def _dense_f4(obj, what, shapes):
    """(pointer, element count, the object) of a dense little-endian float32 device array whose shape is one of `shapes`"""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError("trk_ref_view: %s: %s has no __cuda_array_interface__ (device arrays only: nothing is copied to the device here)" % (what, type(obj).__name__))
    if cai["typestr"] != "<f4":
        raise NaloError("trk_ref_view: %s: typestr %r, float32 ('<f4') is required" % (what, cai["typestr"]))
    shape = tuple(int(v) for v in cai["shape"])
    if shapes is not None and shape not in shapes:
        raise NaloError("trk_ref_view: %s: shape %r, expected one of %r" % (what, shape, shapes))
    strides = cai.get("strides")
    if strides is not None:
        dense, acc = [], 4
        for k in reversed(shape):
            dense.insert(0, acc)
            acc *= k
        if any(k > 1 and int(st) != de for k, st, de in zip(shape, strides, dense)):
            raise NaloError("trk_ref_view: %s: strides %r are not dense (the copy reads consecutive words; make it contiguous on the producer's side)" % (what, tuple(strides)))
    n = int(np.prod(shape)) if shape else 1
    return int(cai["data"][0]) or None, n, obj


def trk_ref_view(w, h, levels, per_level, intrinsics, stream=0, slot_ref=-1):
    """nalo_trk_ref_view (a TrkRefView) from device arrays: per_level is a sequence of `levels` dicts with the 1-D float32 arrays u, v, idepth, color (equal
    length; all absent or None: an empty cloud) and the maps idepth_map, weight_sums ((h>>l, w>>l) or flat; both or neither - neither: the importer zero-fills).
    Any object with __cuda_array_interface__ serves; a slice 4 bytes off a 16-byte boundary is fine. intrinsics: (fx, fy, cx, cy) per level (pyr_intrinsics).
    Pure host code; the struct keeps the arrays alive."""
    if not 1 <= levels <= MAX_LEVELS or len(per_level) != levels:
        raise NaloError("trk_ref_view: %d levels described, %d expected (at most %d)" % (len(per_level), levels, MAX_LEVELS))
    intr = np.asarray(intrinsics, np.float32)
    if intr.shape != (4, levels):
        raise NaloError("trk_ref_view: intrinsics are (fx, fy, cx, cy) x levels")
    V = TrkRefView()
    V.w, V.h, V.levels, V.slot_ref, V.stream = w, h, levels, slot_ref, stream or None
    keep = []
    for l, lv in enumerate(per_level):
        cloud = [lv.get(k) for k in ("u", "v", "idepth", "color")]
        if any(a is not None for a in cloud):
            if any(a is None for a in cloud):
                raise NaloError("trk_ref_view: level %d: u, v, idepth and color come together" % l)
            got = [_dense_f4(a, "level %d %s" % (l, k), None) for a, k in zip(cloud, ("u", "v", "idepth", "color"))]
            if any(len(a.__cuda_array_interface__["shape"]) != 1 for a in cloud) or len({g[1] for g in got}) != 1:
                raise NaloError("trk_ref_view: level %d: u, v, idepth and color are 1-D arrays of equal length" % l)
            V.n[l] = got[0][1]
            V.u[l], V.v[l], V.idepth[l], V.color[l] = (g[0] if got[0][1] else None for g in got)
            keep += cloud
        maps = [lv.get("idepth_map"), lv.get("weight_sums")]
        if (maps[0] is None) != (maps[1] is None):
            raise NaloError("trk_ref_view: level %d: idepth_map and weight_sums are given together or not at all" % l)
        if maps[0] is not None:
            wl, hl = w >> l, h >> l
            got = [_dense_f4(a, "level %d %s" % (l, k), ((hl, wl), (hl * wl,))) for a, k in zip(maps, ("idepth_map", "weight_sums"))]
            V.idepth_map[l], V.weight_sums[l] = got[0][0], got[1][0]
            keep += maps
        V.fx[l], V.fy[l], V.cx[l], V.cy[l] = (float(x) for x in intr[:, l])
    V._keep = keep
    return V


def shard_points(host, u, v, W, img_w, img_h, rank, world):
    """indices (ascending) of the active points rank `rank` of `world` keeps: nalo_shard_points, host code (no device needed)"""
    L = load()
    h = np.ascontiguousarray(host, np.int32)
    uu, vv = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    keep = np.zeros(len(h), np.int32)
    n = L.nalo_shard_points(len(h), int(W), _i(h), _f(uu), _f(vv), int(img_w), int(img_h), int(rank), int(world), _i(keep))
    if n < 0:
        raise NaloError("nalo_shard_points: bad argument (%d)" % n)
    return keep[:n].copy()


def rccl_unique_id():
    """128-byte ncclUniqueId (rank 0 draws it, the caller ships it to the other ranks)"""
    buf = C.create_string_buffer(128)
    rc = load().nalo_rccl_unique_id(buf)
    if rc != 0:
        raise NaloError("nalo_rccl_unique_id failed (%d): librccl missing?" % rc)
    return buf.raw


class Context:
    """Thin object wrapper over nalo_ctx*."""

    def __init__(self, w, h, K, n_slots, levels=0, device=0):
        self.L = load()
        self.h_ = C.c_void_p()
        Kf = np.asarray(K, np.float32)
        rc = self.L.nalo_create(C.byref(self.h_), device, w, h, levels, _f(Kf), n_slots)
        if rc != 0:
            raise NaloError("nalo_create failed (%d): needs a gfx950 device, no CPU fallback" % rc)
        self.w, self.h, self.K = w, h, tuple(float(k) for k in K)
        self.levels = self.L.nalo_levels(self.h_)
        self.W = 0
        self.P = 0
        self._hook = None
        self._pinned = []

    def close(self):
        if self.h_:
            self.L.nalo_destroy(self.h_)
            self.h_ = C.c_void_p()
            for p in self._pinned:
                self.L.nalo_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise NaloError("nalo error %d: %s" % (rc, self.L.nalo_last_error(self.h_).decode()))

    def sync(self):
        self._ck(self.L.nalo_sync(self.h_))

    def test_inject(self, what, count=1):
        """tests only: the count-th matching event from now fails once (nalo_test_inject); count 0 disarms"""
        self._ck(self.L.nalo_test_inject(self.h_, what, count))

    # ---- frames
    def frame_upload(self, slot, img, mask=None, bgr=None, gammaB=None):
        img = np.ascontiguousarray(img, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.float32)
        b = None if bgr is None else np.ascontiguousarray(bgr, np.uint8)
        g = None if gammaB is None else np.ascontiguousarray(gammaB, np.float32)
        assert g is None or g.size == 256
        self._ck(self.L.nalo_frame_upload(self.h_, slot, _f(img), _f(m), _u8(b), _f(g)))

    def frame_upload_async(self, slot, img, mask=None, bgr=None, gammaB=None):
        """img (and mask / bgr) must be contiguous arrays of the right dtype that stay alive and untouched until frame_wait(slot): no conversion, no copy
        here (pinned_array() gives page-locked arrays, the only kind the copy engine reads asynchronously)"""
        assert img.dtype == np.float32 and img.flags.c_contiguous and img.size == self.w * self.h
        assert mask is None or (mask.dtype == np.float32 and mask.flags.c_contiguous)
        assert bgr is None or (bgr.dtype == np.uint8 and bgr.flags.c_contiguous)
        assert gammaB is None or (gammaB.dtype == np.float32 and gammaB.size == 256)
        self._ck(self.L.nalo_frame_upload_async(self.h_, slot, _f(img), _f(mask), _u8(bgr), _f(gammaB)))

    def frame_wait(self, slot):
        self._ck(self.L.nalo_frame_wait(self.h_, slot))

    def dev_plane_check(self, desc):
        """nalo_dev_plane_check on a DevPlane (dev_plane()): raises NaloError when the library refuses the descriptor; launches nothing"""
        self._ck(self.L.nalo_dev_plane_check(self.h_, C.byref(desc)))

    def frame_ingest(self, slot, image=None, mask=None, colour=None, colour_layout="hwc", colour_order="bgr", exposure=1.0, factor=1.0, gammaB=None, stream=None,
                     release=True):
        """nalo_frame_ingest_device: image (u1 / u2 sensor frame or f4 rectified irradiance; None attaches mask / colour to the slot's pyramid), mask (u1 / i4 / f4)
        and colour (u1, colour_layout 'hwc' or 'chw', colour_order 'bgr' or 'rgb') are device arrays with __cuda_array_interface__, read where they lie: nothing is
        converted or copied here. stream: the hipStream_t (an int) whose queued work produces them; None takes torch.cuda.current_stream of a torch.Tensor and
        the null stream for anything else. release=True lets that stream wait (on the device) until the planes have been read, so they may be dropped or overwritten
        on it at once; with release=False call frame_wait(slot) or frame_release(slot, stream) first. Returns without waiting for the device."""
        if colour_layout not in ("hwc", "chw") or colour_order not in ("bgr", "rgb"):
            raise NaloError("frame_ingest: colour_layout is 'hwc' or 'chw', colour_order 'bgr' or 'rgb'")
        planes = [None if o is None else dev_plane(o, lay) for o, lay in ((image, None), (mask, None), (colour, colour_layout))]
        if stream is None:
            stream = 0
            torch = sys.modules.get("torch")                       # a torch.Tensor exists only where torch has been imported: never imported for other producers
            for o in (image, mask, colour):
                if isinstance(o, DeviceView):                      # a view of another context's slot: that context's main stream produced it
                    stream = o.stream
                    break
                if torch is not None and isinstance(o, torch.Tensor):
                    stream = torch.cuda.current_stream(o.device).cuda_stream
                    break
        g = None if gammaB is None else np.ascontiguousarray(gammaB, np.float32)
        assert g is None or g.size == 256
        ptr = lambda d: None if d is None else C.pointer(d)
        a = FrameIngestArgs(ptr(planes[0]), exposure, factor, ptr(planes[1]), ptr(planes[2]), int(colour_order == "rgb"), _f(g), stream or None)
        self._ck(self.L.nalo_frame_ingest_device(self.h_, slot, C.byref(a)))
        if release:
            self.frame_release(slot, stream)

    def frame_release(self, slot, stream):
        """nalo_frame_release: `stream` (a hipStream_t as an int, 0 / None the null stream) waits on the device until the slot's last ingest has read its planes"""
        self._ck(self.L.nalo_frame_release(self.h_, slot, stream or None))

    def frame_attach(self, slot, mask_org=None, bgr_org=None):
        """nalo_frame_attach: mask and / or colour (host arrays in the sensor's size) resized into a slot that holds a pyramid already; synchronous"""
        m = None if mask_org is None else np.ascontiguousarray(mask_org, np.uint8)
        b = None if bgr_org is None else np.ascontiguousarray(bgr_org, np.uint8)
        no = getattr(self, "_und_size", None)
        if no is None:
            raise NaloError("frame_attach: undist_set has not run on this context")
        if (m is not None and m.size != no) or (b is not None and b.size != 3 * no):
            raise NaloError("frame_attach: mask_org is wOrg x hOrg bytes, bgr_org wOrg x hOrg x 3")
        self._ck(self.L.nalo_frame_attach(self.h_, slot, _u8(m), _u8(b)))

    def pinned_array(self, shape, dtype=np.float32):
        """numpy array over page-locked host memory from nalo_host_alloc (freed when the context closes)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.L.nalo_host_alloc(n)
        if not p:
            raise NaloError("nalo_host_alloc(%d) failed" % n)
        self._pinned.append(p)
        buf = (C.c_char * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def frame_rebuild(self, slot):
        self._ck(self.L.nalo_frame_rebuild(self.h_, slot))

    def frame_download(self, slot, lvl):
        n = (self.w >> lvl) * (self.h >> lvl)
        dI, ab = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        self._ck(self.L.nalo_frame_download(self.h_, slot, lvl, _f(dI), _f(ab)))
        return dI, ab

    def frame_download_mask(self, slot, mask=True, bgr=True):
        """(mask [h, w] float32 or None, bgr [h, w, 3] uint8 or None) of the slot: nalo_frame_download_mask"""
        m = np.zeros((self.h, self.w), np.float32) if mask else None
        b = np.zeros((self.h, self.w, 3), np.uint8) if bgr else None
        self._ck(self.L.nalo_frame_download_mask(self.h_, slot, _f(m), _u8(b)))
        return m, b

    # ---- tracker
    def trk_set_ref(self, slot, Ku, Kv, new_idepth, HdiF):
        a = [np.ascontiguousarray(x, np.float32) for x in (Ku, Kv, new_idepth, HdiF)]
        self._ck(self.L.nalo_trk_set_ref(self.h_, slot, len(a[0]), *[_f(x) for x in a]))

    def trk_ref_upload(self, Ku, Kv, new_idepth, HdiF):
        """the inputs of setCoarseTrackingRef resident on the device (nalo_trk_ref_upload); trk_set_ref_resident(slot) then builds the reference from them"""
        a = [np.ascontiguousarray(x, np.float32) for x in (Ku, Kv, new_idepth, HdiF)]
        self._ck(self.L.nalo_trk_ref_upload(self.h_, len(a[0]), *[_f(x) for x in a]))

    def trk_set_ref_resident(self, slot):
        self._ck(self.L.nalo_trk_set_ref_resident(self.h_, slot))

    def trk_set_ref_from_window(self):
        """setCoarseTrackingRef from this context's BA window (nalo_trk_set_ref_from_window): the IN residuals to the newest frame as the last
        linearizeAll(true) left them, gathered on the device; the reference slot is the newest window frame's"""
        self._ck(self.L.nalo_trk_set_ref_from_window(self.h_))

    def trk_set_ref_from_depth(self, slot, depth, min_depth, max_depth, hdi, step=1, min_grad=0.0, stream=None):
        """setCoarseTrackingRef from a depth plane on the device (nalo_trk_set_ref_from_depth): every pixel with u % step == 0, v % step == 0, min_depth <= D <=
        max_depth and (min_grad != 0) absSquaredGrad >= min_grad becomes a point (u, v, 1 / D, hdi); the result is trk_set_ref's on that list, bit for bit.
        depth is a 2-D float32 device array of the context's size (anything with __cuda_array_interface__: a torch tensor or view, the depth DeviceView of
        tsdf_raycast_view) or a DevPlane. stream: the producing hipStream_t (None: a DeviceView's own, torch's current stream of a tensor, else the null stream).
        The plane has been read when the call returns. Returns n_seeded; self.trk_depth_ref_seeded holds it too, 0 after a refusal."""
        a = TrkDepthRefArgs()
        a.depth = depth if isinstance(depth, DevPlane) else dev_plane(depth)
        if stream is None:
            stream = 0
            torch = sys.modules.get("torch")
            if isinstance(depth, DeviceView):
                stream = depth.stream
            elif torch is not None and isinstance(depth, torch.Tensor):
                stream = torch.cuda.current_stream(depth.device).cuda_stream
        a.min_depth, a.max_depth, a.hdi, a.step, a.min_grad, a.producer_stream = float(min_depth), float(max_depth), float(hdi), int(step), float(min_grad), stream or None
        a.n_seeded = -1
        rc = self.L.nalo_trk_set_ref_from_depth(self.h_, slot, C.byref(a))
        self.trk_depth_ref_seeded = int(a.n_seeded)
        self._ck(rc)
        return int(a.n_seeded)

    def trk_set_pc(self, slot, lvl, u, v, idepth, color):
        a = [np.ascontiguousarray(x, np.float32) for x in (u, v, idepth, color)]
        self._ck(self.L.nalo_trk_set_pc(self.h_, slot, lvl, len(a[0]), *[_f(x) for x in a]))

    def trk_get_pc(self, lvl):
        n = C.c_int(0)
        self._ck(self.L.nalo_trk_get_pc(self.h_, lvl, C.byref(n), None, None, None, None))
        out = [np.zeros(n.value, np.float32) for _ in range(4)]
        self._ck(self.L.nalo_trk_get_pc(self.h_, lvl, C.byref(n), *[_f(o) for o in out]))
        return out

    def trk_get_depth(self, lvl):
        n = (self.w >> lvl) * (self.h >> lvl)
        a, b = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._ck(self.L.nalo_trk_get_depth(self.h_, lvl, _f(a), _f(b)))
        return a, b

    def trk_set_depth(self, slot, lvl, idepth=None, weight_sums=None):
        """one level's inverse-depth map / weight sums injected directly (nalo_trk_set_depth); None leaves that half untouched"""
        n = (self.w >> lvl) * (self.h >> lvl)
        a = [None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1) for x in (idepth, weight_sums)]
        assert all(x is None or x.size == n for x in a)
        self._ck(self.L.nalo_trk_set_depth(self.h_, slot, lvl, _f(a[0]), _f(a[1])))

    def frame_plane(self, slot, which):
        """nalo_frame_plane: a DeviceView of the slot's level-0 irradiance ('irradiance' / PLANE_IRRADIANCE: (h, w) float32), mask ('mask': (h, w) float32) or
        colour ('colour': (h, w, 3) uint8, B,G,R). Zero-copy: torch.as_tensor(view) aliases the slot, and another context's frame_ingest(slot, image=view, ...)
        reads it where it lies, waiting on the device for this context's stream. Launches nothing. Good until the slot is rewritten or the context closed."""
        d = DevPlane()
        self._ck(self.L.nalo_frame_plane(self.h_, slot, _PLANE_NAMES.get(which, which), C.byref(d)))
        return DeviceView.of_plane(d, self.stream, self)

    def trk_ref_export(self):
        """nalo_trk_ref_export: dict(view = the raw TrkRefView for another context's trk_ref_import, n, slot_ref, intrinsics (4, levels), stream, levels = per level a
        dict of DeviceViews u, v, idepth, color (n[l] floats) and idepth_map, weight_sums ((h>>l, w>>l), or None where the level has none)). Launches nothing."""
        V = TrkRefView()
        self._ck(self.L.nalo_trk_ref_export(self.h_, C.byref(V)))
        st = int(V.stream or 0)
        lv = []
        for l in range(V.levels):
            d = {k: DeviceView(getattr(V, k)[l], (V.n[l],), "<f4", None, st, self) for k in ("u", "v", "idepth", "color")}
            for k in ("idepth_map", "weight_sums"):
                d[k] = DeviceView(getattr(V, k)[l], (self.h >> l, self.w >> l), "<f4", None, st, self) if getattr(V, k)[l] else None
            lv.append(d)
        intr = np.array([[getattr(V, k)[l] for l in range(V.levels)] for k in ("fx", "fy", "cx", "cy")], np.float32)
        return dict(view=V, n=[V.n[l] for l in range(V.levels)], slot_ref=V.slot_ref, intrinsics=intr, stream=st, levels=lv)

    def trk_ref_import(self, slot, view, intrinsics=None, stream=None):
        """nalo_trk_ref_import: this context's tracking reference becomes a clone of `view` - a TrkRefView, what trk_ref_export returned, or a sequence of per-level
        dicts of device arrays (trk_ref_view; torch tensors serve), for which intrinsics defaults to this context's own (pyr_intrinsics) and stream to torch's
        current stream of the first tensor found (the null stream otherwise). `slot` holds the reference frame in THIS context. Returns without waiting for the
        device; trk_ref_release(stream) is the back edge before the source is rewritten."""
        if isinstance(view, dict) and "view" in view:
            view = view["view"]
        if not isinstance(view, TrkRefView):
            if stream is None:
                stream = 0
                torch = sys.modules.get("torch")
                for o in [a for lv in view for a in lv.values()]:
                    if isinstance(o, DeviceView):
                        stream = o.stream
                        break
                    if torch is not None and isinstance(o, torch.Tensor):
                        stream = torch.cuda.current_stream(o.device).cuda_stream
                        break
            view = trk_ref_view(self.w, self.h, self.levels, view, pyr_intrinsics(self.K, self.levels) if intrinsics is None else intrinsics, stream)
        self._ck(self.L.nalo_trk_ref_import(self.h_, slot, C.byref(view)))

    def trk_ref_release(self, stream):
        """nalo_trk_ref_release: `stream` (a hipStream_t as an int, 0 / None the null stream) waits on the device until this context's last import has read its source"""
        self._ck(self.L.nalo_trk_ref_release(self.h_, stream or None))

    def trk_depth_image(self, minmax=None, want_idepth=False):
        """debugPlotIDepthMap on the device (nalo_trk_depth_image). minmax: the caller's (minIdJetVisTracker, maxIdJetVisTracker) pair, None = the reference's
        NULL pointers. Returns a dict: bgr (h, w, 3) uint8, minmax (the rewritten pair as float32, or None), n_positive, min_new, max_new, min_used, max_used
        (float32) and, when asked for, idepth (w * h)"""
        a = DepthImageArgs()
        bgr = np.zeros((self.h, self.w, 3), np.uint8)
        mm = None if minmax is None else np.array(minmax, np.float32).reshape(2)
        idp = np.zeros(self.w * self.h, np.float32) if want_idepth else None
        a.minmax_io, a.bgr, a.idepth = _f(mm), _u8(bgr), _f(idp)
        self._ck(self.L.nalo_trk_depth_image(self.h_, C.byref(a)))
        out = {"bgr": bgr, "minmax": mm, "n_positive": a.n_positive}
        for k in ("min_new", "max_new", "min_used", "max_used"):
            out[k] = np.float32(getattr(a, k))
        if want_idepth:
            out["idepth"] = idp
        return out

    def trk_eval(self, slot_new, lvl, T, affLL, b0, cutoff, want_gs=True):
        T = np.ascontiguousarray(T, np.float64).reshape(3, 4)
        R = np.ascontiguousarray(T[:, :3]).reshape(-1)
        t = np.ascontiguousarray(T[:, 3])
        st, H, b = np.zeros(6), np.zeros(64), np.zeros(8)
        self._ck(self.L.nalo_trk_eval(self.h_, slot_new, lvl, _d(R), _d(t), _f(np.asarray(affLL, np.float32)), b0, cutoff,
                                      int(want_gs), _d(st), _d(H), _d(b)))
        return st, H.reshape(8, 8), b

    def trk_set_shard(self, rank, world, fn=None, stream_ordered=False):
        """sharded tracker: this context evaluates rank / world of every level's points; fn(device_ptr:int, n:int) sums n doubles in place across ranks. world = 1: off"""
        self._trk_hook = ALLREDUCE_FN(lambda user, ptr, n: fn(ptr, n)) if fn is not None else C.cast(None, ALLREDUCE_FN)
        self.L.nalo_trk_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p, C.c_int]
        self._ck(self.L.nalo_trk_set_shard(self.h_, int(rank), int(world), self._trk_hook, None, int(bool(stream_ordered))))

    def trk_track(self, slot_new, T0, aff0, ref_aff, exposures, coarsest, min_res=None):
        T = np.ascontiguousarray(T0, np.float64).reshape(-1).copy()
        aff = np.array(aff0, np.float64)
        mr = np.full(5, np.nan) if min_res is None else np.asarray(min_res, np.float64)
        lr, lf = np.zeros(5), np.zeros(3)
        ok, ne = C.c_int(0), C.c_int(0)
        self._ck(self.L.nalo_trk_track(self.h_, slot_new, _d(T), _d(aff), _d(np.asarray(ref_aff, np.float64)),
                                       _f(np.asarray(exposures, np.float32)), coarsest, _d(mr), _d(lr), _d(lf), C.byref(ok), C.byref(ne)))
        return ok.value, T.reshape(3, 4), aff, lr, lf, ne.value

    def trk_track_tries(self, slot_new, tries, aff_init, ref_aff, exposures, coarsest, last_coarse_rmse, retrack_threshold=0.0, records=True, args=None):
        """nalo_trk_track_tries: trackNewCoarse's whole hypothesis loop in one call. tries: [n, 3, 4] (or n x 12). Returns a dict: T, aff, flow, achievedRes,
        lastCoarseRMSE (what the call left in lastCoarseRMSE_io), have_one_good, try_iterations, winner, driver, records (structured array, TRY_RECORD_DTYPE,
        one entry per try that ran). args: a prepared TrkTriesArgs to pass as it is (tests of the refusals)."""
        if args is None:
            t = np.ascontiguousarray(tries, np.float64).reshape(-1, 12)
            args = TrkTriesArgs()
            args.slot_new, args.n_tries, args.coarsestLvl = int(slot_new), len(t), int(coarsest)
            args.tries = _d(t)
            args.aff_init[:] = [float(x) for x in aff_init]; args.ref_aff[:] = [float(x) for x in ref_aff]; args.exposures[:] = [float(x) for x in exposures]
            args.lastCoarseRMSE_io[:] = [float(x) for x in np.broadcast_to(np.asarray(last_coarse_rmse, np.float64), (5,))]
            args.reTrackThreshold = float(retrack_threshold)
            args._keep = t
        n = max(args.n_tries, 0)
        rec = np.zeros(min(n, TRK_MAX_TRIES) if records else 0, TRY_RECORD_DTYPE)
        if len(rec):
            args.records, args.records_cap = rec.ctypes.data_as(C.POINTER(TrkTryRecord)), len(rec)
        self._ck(self.L.nalo_trk_track_tries(self.h_, C.byref(args)))
        return dict(T=np.array(args.T).reshape(3, 4), aff=np.array(args.aff), flow=np.array(args.flow), achievedRes=np.array(args.achievedRes),
                    lastCoarseRMSE=np.array(args.lastCoarseRMSE_io), have_one_good=args.have_one_good, try_iterations=args.try_iterations, winner=args.winner,
                    driver=args.driver, records=rec[:args.try_iterations].copy())

    def trk_last_evals(self):
        """LM evaluations per pyramid level of the last trk_track and the point-cloud sizes of the levels (nalo_trk_last_evals)"""
        ev, n = np.zeros(5, np.int32), np.zeros(5, np.int32)
        self._ck(self.L.nalo_trk_last_evals(self.h_, _i(ev), _i(n)))
        return ev, n

    def trk_launch_config(self):
        """how the last trk_track ran (nalo_trk_get_launch_config): driver 1 = persistent LM kernel, 2 = host-driven loop"""
        a = (C.c_int * 9)()
        self._ck(self.L.nalo_trk_get_launch_config(self.h_, a))
        return dict(lanes=a[0], nblocks=a[1], driver=a[2], rounds=list(a[3:8]), have_repeated=a[8])

    # ---- BA
    def ba_set_window(self, slots, evalPT, aff=None, exposure=None, th=None, frame_ids=None, state6=None, calib=None, calib_zero=None,
                      states=None, states_zero=None):
        """states / states_zero ([W][10], unscaled FrameHessian::state / state_zero) give the general form a running window needs; without them the
        frames are set like FrameHessian::setEvalPT_scaled (state_zero = [0.., a/SCALE_A, b/SCALE_B, 0, 0]) plus an optional state6."""
        W = len(slots)
        arr = (FrameState * W)()
        for i in range(W):
            fs = arr[i]
            fs.slot = int(slots[i])
            fs.frame_id = int(i if frame_ids is None else frame_ids[i])
            e = np.ascontiguousarray(evalPT[i], np.float64).reshape(-1)
            for k in range(12):
                fs.worldToCam_evalPT[k] = e[k]
            if states is not None:
                for k in range(10):
                    fs.state[k] = float(states[i][k])
                    fs.state_zero[k] = float(states_zero[i][k])
            else:
                a, b = (0.0, 0.0) if aff is None else aff[i]
                # FrameHessian::setEvalPT_scaled (HessianBlocks.h:247-255): state = [0.., a/SCALE_A, b/SCALE_B, 0, 0], state_zero = state
                st = np.zeros(10)
                # (1.0f / SCALE_A) * a in double, whatever type a has (numpy >= 2 would round float32 * Python float to float32)
                st[6] = float(np.float32(1.0 / 10.0)) * float(a)
                st[7] = float(np.float32(1.0 / 1000.0)) * float(b)
                for k in range(10):
                    fs.state_zero[k] = st[k]
                if state6 is not None:
                    st[:6] = state6[i]
                for k in range(10):
                    fs.state[k] = st[k]
            fs.ab_exposure = 1.0 if exposure is None else float(exposure[i])
            fs.frameEnergyTH = 8 * 8 * 8.0 if th is None else float(th[i])
        cal = np.asarray(self.K if calib is None else calib, np.float64)
        calz = cal if calib_zero is None else np.asarray(calib_zero, np.float64)
        self._ck(self.L.nalo_ba_set_window(self.h_, W, arr, _d(cal), _d(calz)))
        self.W = W

    def ba_set_points(self, host, u, v, idepth, color, weights, has_prior=None, idepth_zero=None):
        a = [np.ascontiguousarray(host, np.int32)] + [np.ascontiguousarray(x, np.float32) for x in (u, v, idepth, color, weights)]
        hp = None if has_prior is None else np.ascontiguousarray(has_prior, np.int32)
        iz = None if idepth_zero is None else np.ascontiguousarray(idepth_zero, np.float32)
        self.P = len(a[0])
        self._ck(self.L.nalo_ba_set_points(self.h_, self.P, _i(a[0]), _f(a[1]), _f(a[2]), _f(a[3]), _f(iz), _f(a[4]), _f(a[5]), _i(hp)))

    def ba_set_prior(self, HM=None, bM=None):
        H = None if HM is None else np.ascontiguousarray(HM, np.float64)
        b = None if bM is None else np.ascontiguousarray(bM, np.float64)
        assert H is None or H.size == self.n * self.n
        self._ck(self.L.nalo_ba_set_prior(self.h_, _d(H), _d(b)))

    def ba_get_prior(self):
        n = self.n
        H, b = np.zeros(n * n), np.zeros(n)
        self._ck(self.L.nalo_ba_get_prior(self.h_, _d(H), _d(b)))
        return H.reshape(n, n), b

    def ba_marginalize_frame(self, idx):
        """EnergyFunctional::marginalizeFrame on HM/bM; the window shrinks by one frame (re-issue set_window / set_points / set_residuals next)"""
        self._ck(self.L.nalo_ba_marginalize_frame(self.h_, int(idx)))
        self.W -= 1

    def ba_set_prior_carry(self, on):
        """declare the context one continuing EnergyFunctional: every ba_set_window keeps (same frames) or extends (one frame appended) HM / bM"""
        self._ck(self.L.nalo_ba_set_prior_carry(self.h_, int(bool(on))))

    def ba_set_residuals(self, exists):
        self._ck(self.L.nalo_ba_set_residuals(self.h_, _u8(np.ascontiguousarray(exists, np.uint8))))

    @property
    def n(self):
        return 8 * self.W + 4

    def ba_linearize(self, fix=False):
        e = C.c_double(0)
        self._ck(self.L.nalo_ba_linearize(self.h_, int(fix), C.byref(e)))
        return e.value

    def ba_accumulate(self, mode):
        H, b = np.zeros(self.n * self.n), np.zeros(self.n)
        self._ck(self.L.nalo_ba_accumulate(self.h_, mode, _d(H), _d(b)))
        return H.reshape(self.n, self.n), b

    def ba_accumulate_sc(self, shift=True):
        H, b = np.zeros(self.n * self.n), np.zeros(self.n)
        self._ck(self.L.nalo_ba_accumulate_sc(self.h_, int(shift), _d(H), _d(b)))
        return H.reshape(self.n, self.n), b

    def ba_solve_system(self, iteration, lam=1e-5):
        x = np.zeros(self.n)
        self._ck(self.L.nalo_ba_solve_system(self.h_, iteration, lam, _d(x)))
        return x

    def ba_backup_state(self):
        self._ck(self.L.nalo_ba_backup_state(self.h_))

    def ba_do_step(self, f=1.0):
        cb = C.c_int(0)
        self._ck(self.L.nalo_ba_do_step(self.h_, f, f, f, f, f, C.byref(cb)))
        return cb.value

    def ba_optimize(self, its=6, never_break=False):
        r = C.c_double(0)
        self._ck(self.L.nalo_ba_optimize(self.h_, its, int(never_break), C.byref(r)))
        return r.value

    def ba_marginalize_points(self, flags):
        n = self.n
        M, Mb, Ms, Mbs = np.zeros(n * n), np.zeros(n), np.zeros(n * n), np.zeros(n)
        self._ck(self.L.nalo_ba_marginalize_points(self.h_, _u8(np.ascontiguousarray(flags, np.uint8)), _d(M), _d(Mb), _d(Ms), _d(Mbs)))
        return M.reshape(n, n), Mb, Ms.reshape(n, n), Mbs

    def ba_set_point_history(self, num_good=None, last_target=None, last_state=None):
        """PointHessian::numGoodResiduals [P] and lastResiduals[2] as (window index of .first or -1, .second) [P][2]; None = the defaults of the header"""
        ng = None if num_good is None else np.ascontiguousarray(num_good, np.int32)
        lt = None if last_target is None else np.ascontiguousarray(last_target, np.int8)
        ls = None if last_state is None else np.ascontiguousarray(last_state, np.int8)
        assert (ng is None or ng.shape == (self.P,)) and (lt is None or lt.shape == (self.P, 2)) and (ls is None or ls.shape == (self.P, 2))
        self._ck(self.L.nalo_ba_set_point_history(self.h_, _i(ng), None if lt is None else lt.ctypes.data_as(c_i8p), None if ls is None else ls.ctypes.data_as(c_i8p)))

    def ba_get_point_history(self):
        ng, lt, ls = np.zeros(self.P, np.int32), np.zeros((self.P, 2), np.int8), np.zeros((self.P, 2), np.int8)
        self._ck(self.L.nalo_ba_get_point_history(self.h_, _i(ng), lt.ctypes.data_as(c_i8p), ls.ctypes.data_as(c_i8p)))
        return ng, lt, ls

    def ba_flag_points(self, frame_flagged, outputs=True):
        """flagPointsForRemoval on the device -> (decision [P], idepth_hessian [P], counts [W][4]); outputs=False leaves the decisions resident and returns None"""
        ff = np.ascontiguousarray(frame_flagged, np.uint8)
        assert ff.shape == (self.W,)
        if not outputs:
            self._ck(self.L.nalo_ba_flag_points(self.h_, _u8(ff), None, None, None))
            return None
        dec, H, cnt = np.zeros(self.P, np.uint8), np.zeros(self.P, np.float32), np.zeros((self.W, 4), np.int32)
        self._ck(self.L.nalo_ba_flag_points(self.h_, _u8(ff), _u8(dec), _f(H), _i(cnt)))
        return dec, H, cnt

    def ba_marginalize_flagged(self):
        n = self.n
        M, Mb, Ms, Mbs = np.zeros(n * n), np.zeros(n), np.zeros(n * n), np.zeros(n)
        self._ck(self.L.nalo_ba_marginalize_flagged(self.h_, _d(M), _d(Mb), _d(Ms), _d(Mbs)))
        return M.reshape(n, n), Mb, Ms.reshape(n, n), Mbs

    def frame_state(self, slot, evalPT, frame_id=0, aff=(0.0, 0.0), exposure=1.0, th=8 * 8 * 8.0, state6=None):
        """one nalo_frame_state as ba_set_window builds it without states / states_zero (FrameHessian::setEvalPT_scaled plus an optional state6)"""
        fs = FrameState()
        fs.slot, fs.frame_id = int(slot), int(frame_id)
        e = np.ascontiguousarray(evalPT, np.float64).reshape(-1)
        st = np.zeros(10)
        st[6] = float(np.float32(1.0 / 10.0)) * float(aff[0])
        st[7] = float(np.float32(1.0 / 1000.0)) * float(aff[1])
        for k in range(12):
            fs.worldToCam_evalPT[k] = e[k]
        for k in range(10):
            fs.state_zero[k] = st[k]
        if state6 is not None:
            st[:6] = state6
        for k in range(10):
            fs.state[k] = st[k]
        fs.ab_exposure, fs.frameEnergyTH = float(exposure), float(th)
        return fs

    def ba_carry_window(self, entering=None, insert_activated=False):
        """the window re-issued from what is resident (nalo_ba_carry_window): entering = a FrameState appended as the newest frame, insert_activated = the
        pending imm_resident_activate result becomes window points -> (points carried, points inserted, P, Ppad)"""
        self._ck(self.L.nalo_ba_carry_window(self.h_, None if entering is None else C.byref(entering), int(bool(insert_activated))))
        st = np.zeros(4, np.int32)
        self._ck(self.L.nalo_ba_carry_last(self.h_, _i(st)))
        self.W += 0 if entering is None else 1
        self.P = int(st[2])
        return tuple(int(x) for x in st)

    def ba_carry_map(self):
        """old submission index of every point of the carried window, -(k + 1) for the k-th selected point of the activation"""
        m = np.zeros(self.P, np.int32)
        self._ck(self.L.nalo_ba_carry_map(self.h_, _i(m)))
        return m

    def init_window_args(self, first, entering, draws, density=2000.0, calib=None, calib_zero=None):
        """nalo_init_window_args from two FrameStates (slot, frame_id, ab_exposure, frameEnergyTH are read), the draws and setting_desiredPointDensity; the
        draws array is kept alive by the returned object"""
        a = InitWindowArgs()
        C.memmove(C.byref(a.first), C.byref(first), C.sizeof(FrameState))
        C.memmove(C.byref(a.entering), C.byref(entering), C.sizeof(FrameState))
        cal = np.asarray(self.K if calib is None else calib, np.float64)
        calz = cal if calib_zero is None else np.asarray(calib_zero, np.float64)
        for k in range(4):
            a.calib[k], a.calib_zero[k] = float(cal[k]), float(calz[k])
        a.desired_point_density = float(density)
        a._draws = None if draws is None else np.ascontiguousarray(draws, np.int32)
        a.n_draws = 0 if draws is None else len(a._draws)
        a.draws = None if draws is None else _i(a._draws)
        return a

    def ba_window_from_initializer(self, first, entering, draws, density=2000.0, calib=None, calib_zero=None):
        """the first window {first, entering} issued from the initialiser's level-0 points on the device (nalo_ba_window_from_initializer)
        -> (the two FrameStates as the call set them, (sumID, numID, rescaleFactor), (n, skipped by draw, rejected non-finite, P))"""
        a = self.init_window_args(first, entering, draws, density, calib, calib_zero)
        self._ck(self.L.nalo_ba_window_from_initializer(self.h_, C.byref(a)))
        scale, stats = self.ba_init_window_last()
        self.W, self.P = 2, int(stats[3])
        out = [FrameState(), FrameState()]
        C.memmove(C.byref(out[0]), C.byref(a.first), C.sizeof(FrameState))
        C.memmove(C.byref(out[1]), C.byref(a.entering), C.sizeof(FrameState))
        return out, scale, stats

    def ba_init_window_map(self):
        """level-0 index of every point of the window issued from the initialiser, in submission order"""
        m = np.zeros(self.P, np.int32)
        self._ck(self.L.nalo_ba_init_window_map(self.h_, _i(m)))
        return m

    def ba_init_window_last(self):
        scale, stats = np.zeros(3, np.float32), np.zeros(4, np.int32)
        self._ck(self.L.nalo_ba_init_window_last(self.h_, _f(scale), _i(stats)))
        return scale, tuple(int(x) for x in stats)

    # ---- the map: removed points archived on the device, and the clouds published from it
    def map_enable(self, on=True, chunk_points=0):
        """nalo_map_enable: from the next ba_flag_points on, ba_marginalize_flagged archives every point it removes"""
        self._ck(self.L.nalo_map_enable(self.h_, int(bool(on)), int(chunk_points)))

    def map_reset(self):
        self._ck(self.L.nalo_map_reset(self.h_))

    def map_counts(self, frame_id):
        """(pointHessiansMarginalized.size(), pointHessiansOut.size()) of the frame"""
        a = np.zeros(2, np.int32)
        self._ck(self.L.nalo_map_counts(self.h_, int(frame_id), _i(a)))
        return int(a[0]), int(a[1])

    def map_get_frame(self, frame_id):
        """the frame's archive records (MAP_RECORD_DTYPE): marginalised first, then out"""
        n = C.c_int(0)
        rc = self.L.nalo_map_get_frame(self.h_, int(frame_id), None, 0, C.byref(n))
        if n.value == 0:
            self._ck(rc)
        rec = np.zeros(n.value, MAP_RECORD_DTYPE)
        if n.value:
            self._ck(self.L.nalo_map_get_frame(self.h_, int(frame_id), rec.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return rec

    def map_world_points(self, frame_id, cam_to_world):
        """publishKeyframes(final = true): the world points [n][3] (float64) of the frame's marginalised points"""
        m = np.ascontiguousarray(cam_to_world, np.float64).reshape(-1)
        assert m.size == 12
        n = C.c_int(0)
        rc = self.L.nalo_map_world_points(self.h_, int(frame_id), _d(m), None, 0, C.byref(n))
        if n.value == 0:
            self._ck(rc)
        xyz = np.zeros((n.value, 3), np.float64)
        if n.value:
            self._ck(self.L.nalo_map_world_points(self.h_, int(frame_id), _d(m), _d(xyz), n.value, C.byref(n)))
        return xyz

    def map_frame_cloud(self, frame_id, display_mode=1, scaledTH=1e10, absTH=1e10, minRelBS=0.0, with_immature=True, draws=None, sparsity=1):
        """setFromKF + refreshPC for one frame -> dict(xyz [n][3] float32, rgb [n][3] uint8, records [4], survivors [4])"""
        a = MapCloudArgs()
        a.frame_id, a.display_mode, a.with_immature, a.sparsity = int(frame_id), int(display_mode), int(bool(with_immature)), int(sparsity)
        a.scaledTH, a.absTH, a.minRelBS = float(scaledTH), float(absTH), float(minRelBS)
        rc = self.L.nalo_map_frame_cloud(self.h_, C.byref(a))                    # cap = 0: answers n_needed (and is the whole call for a frame without records)
        if a.n_needed == 0:
            self._ck(rc)
        cap = a.n_needed
        xyz, rgb = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8)
        if cap:
            d = None if draws is None else np.ascontiguousarray(draws, np.int32)
            a.cap, a.xyz, a.rgb = cap, _f(xyz), _u8(rgb)
            a.draws, a.n_draws = (None, 0) if d is None else (_i(d), len(d))
            self._ck(self.L.nalo_map_frame_cloud(self.h_, C.byref(a)))
        return dict(xyz=xyz[:a.n], rgb=rgb[:a.n], records=np.array(list(a.records)), survivors=np.array(list(a.survivors)), n_needed=cap)

    def map_window_plot(self, mode=1, frame_mask=0, minmax=None, rainbow_scale=1.0, quality_scale=1.0):
        """FullSystem::debugPlot on the device (nalo_map_window_plot): one image per selected window frame. minmax: the caller's (minIdJetVisDebug,
        maxIdJetVisDebug) pair for mode 7, None = no smoothing. Returns a dict: bgr (n_frames, h, w, 3) uint8, frame_id [n_frames], sources [n_frames][4]
        (immature, active, marginalised, out), minmax (the rewritten pair as float32, or None), n_values, min_new, max_new, min_used, max_used (float32)"""
        a = WindowPlotArgs()
        W = max(self.W, 1)
        nf = bin(frame_mask).count("1") if frame_mask else W
        bgr = np.zeros((max(nf, 1), self.h, self.w, 3), np.uint8)
        mm = None if minmax is None else np.array(minmax, np.float32).reshape(2)
        a.mode, a.rainbow_scale, a.quality_scale, a.frame_mask = int(mode), float(rainbow_scale), float(quality_scale), int(frame_mask)
        a.minmax_io, a.bgr = _f(mm), _u8(bgr)
        self._ck(self.L.nalo_map_window_plot(self.h_, C.byref(a)))
        n = a.n_frames
        out = {"bgr": bgr[:n], "frame_id": [a.frame_id[j] for j in range(n)], "sources": np.array([list(a.sources[j]) for j in range(n)], np.int32).reshape(n, 4),
               "minmax": mm, "n_values": a.n_values}
        for k in ("min_new", "max_new", "min_used", "max_used"):
            out[k] = np.float32(getattr(a, k))
        return out

    def map_render_args(self, vw, vh, view, frames=(), fx=400.0, fy=400.0, cx=None, cy=None, znear=0.1, zfar=1000.0, display_mode=1, scaledTH=1e10, absTH=1e10,
                        minRelBS=0.0, with_immature=True, sparsity=1, with_dense=False, show_kf_cams=False, current_cam=None, show_active_constraints=False,
                        show_all_constraints=False, show_trajectory=False, all_poses=None, background=(255, 255, 255)):
        """a filled MapRenderArgs without outputs, and the arrays it points into (keep them alive). frames: [(frame_id, camToWorld 3x4)]; current_cam: a 3x4 pose
        (show_current_cam) or None; all_poses: [n][3] (show_full_trajectory) or None; cx, cy default to vw / 2, vh / 2 as in the viewer"""
        a = MapRenderArgs()
        a.vw, a.vh, a.fx, a.fy, a.znear, a.zfar = int(vw), int(vh), float(fx), float(fy), float(znear), float(zfar)
        a.cx, a.cy = float(vw / 2 if cx is None else cx), float(vh / 2 if cy is None else cy)
        a.viewFromWorld = (C.c_double * 12)(*np.asarray(view, np.float64).reshape(12))
        fr = (ViewFrame * max(len(frames), 1))()
        for i, (fid, m) in enumerate(frames):
            fr[i].frame_id = int(fid)
            fr[i].camToWorld = (C.c_double * 12)(*np.asarray(m, np.float64).reshape(12))
        a.n_frames, a.frames = len(frames), fr
        a.display_mode, a.with_immature, a.sparsity, a.with_dense = int(display_mode), int(bool(with_immature)), int(sparsity), int(bool(with_dense))
        a.scaledTH, a.absTH, a.minRelBS = float(scaledTH), float(absTH), float(minRelBS)
        a.show_kf_cams, a.show_current_cam = int(bool(show_kf_cams)), int(current_cam is not None)
        if current_cam is not None:
            a.currentCamToWorld = (C.c_double * 12)(*np.asarray(current_cam, np.float64).reshape(12))
        a.show_active_constraints, a.show_all_constraints, a.show_trajectory = int(bool(show_active_constraints)), int(bool(show_all_constraints)), int(bool(show_trajectory))
        poses = None if all_poses is None else np.ascontiguousarray(all_poses, np.float32).reshape(-1, 3)
        a.show_full_trajectory, a.n_all_poses, a.all_poses = int(poses is not None), 0 if poses is None else len(poses), _f(poses)
        a.background = (C.c_uint8 * 3)(*[int(b) for b in background])
        return a, (fr, poses)

    def map_render(self, vw, vh, view, frames=(), want_depth=True, **kw):
        """the viewer's 3-D panel on the device (nalo_map_render; keywords: map_render_args) -> dict(rgb (vh, vw, 3) uint8, depth (vh, vw) float32 or None,
        n_vertices, n_drawn_points, n_segments, n_line_samples)"""
        a, keep = self.map_render_args(vw, vh, view, frames, **kw)
        rgb = np.zeros((int(vh), int(vw), 3), np.uint8)
        depth = np.zeros((int(vh), int(vw)), np.float32) if want_depth else None
        a.rgb, a.depth = _u8(rgb), _f(depth)
        self._ck(self.L.nalo_map_render(self.h_, C.byref(a)))
        del keep
        return dict(rgb=rgb, depth=depth, n_vertices=int(a.n_vertices), n_drawn_points=int(a.n_drawn_points), n_segments=int(a.n_segments),
                    n_line_samples=int(a.n_line_samples))

    @staticmethod
    def render_mesh_src(mesh, stream=None):
        """a filled RenderMeshSrc from mesh = (xyz [nv][3] float32, tri [nt][3] int32, rgba [nv][4] uint8 or None), each anything with __cuda_array_interface__
        (dense, C-contiguous), read where it lies; stream: the hipStream_t (an int) whose queued work produces the arrays, None / 0 = the null stream. Returns
        (src, what it points into): keep the second alive"""
        xyz, tri, rgba = mesh
        src = RenderMeshSrc()

        def dense(obj, what, typestrs, cols):
            cai = getattr(obj, "__cuda_array_interface__", None)
            if cai is None:
                raise TypeError("map_render_mesh: %s: %s has no __cuda_array_interface__ (device arrays only: nothing is copied to the device here)" % (what, type(obj).__name__))
            shape = tuple(int(v) for v in cai["shape"])
            if cai["typestr"] not in typestrs or len(shape) != 2 or shape[1] != cols:
                raise NaloError("map_render_mesh: %s: typestr %r shape %r, expected %s [n][%d]" % (what, cai["typestr"], shape, typestrs[0], cols))
            item = int(typestrs[0][2])
            st = cai.get("strides")
            if st is not None and shape[0] > 0 and ((shape[0] > 1 and int(st[0]) != cols * item) or int(st[1]) != item):
                raise NaloError("map_render_mesh: %s: strides %r are not dense (make it contiguous on the producer's side)" % (what, tuple(st)))
            return (int(cai["data"][0]) or None) if shape[0] > 0 else None, shape[0]

        src.xyz, src.n_vertices = dense(xyz, "xyz", ("<f4",), 3)
        src.tri, src.n_triangles = dense(tri, "tri", ("<i4",), 3)
        if rgba is not None:
            src.rgba, n = dense(rgba, "rgba", ("|u1", "<u1"), 4)
            if n != src.n_vertices:
                raise NaloError("map_render_mesh: rgba has %d rows, xyz %d" % (n, src.n_vertices))
        src.producer_stream = int(stream) if stream else None
        return src, (xyz, tri, rgba)

    def map_render_mesh(self, vw, vh, view, frames=(), archive=False, live=False, mesh=None, colour_mode=0, max_box_pixels=0, mesh_stream=None, want_depth=True, **kw):
        """nalo_map_render_mesh: map_render with the triangles of the TSDF meshes in the same depth test (keywords: map_render_args) -> map_render's dict plus
        n_triangles, n_tri_bad_index, n_tri_near, n_tri_guard, n_tri_degenerate, n_tri_large, n_tri_pixels. archive: the welded archive (tsdf_archive_view's
        arrays); live: the device mesh the last tsdf_mesh left; mesh: a caller's (xyz, tri, rgba-or-None) device arrays in WORLD coordinates, produced by the
        work queued on mesh_stream (a hipStream_t as an int; None = the null stream). colour_mode 0: vertex colours, 1: shaded grey. One call, one wait"""
        a, keep = self.map_render_args(vw, vh, view, frames, **kw)
        rgb = np.zeros((int(vh), int(vw), 3), np.uint8)
        depth = np.zeros((int(vh), int(vw)), np.float32) if want_depth else None
        a.rgb, a.depth = _u8(rgb), _f(depth)
        m = MapRenderMeshArgs()
        m.with_archive, m.with_live_mesh, m.colour_mode, m.max_box_pixels = int(bool(archive)), int(bool(live)), int(colour_mode), int(max_box_pixels)
        src = None
        if mesh is not None:
            src, keep_mesh = self.render_mesh_src(mesh, mesh_stream)
            m.user = C.pointer(src)
        self._ck(self.L.nalo_map_render_mesh(self.h_, C.byref(a), C.byref(m)))
        del keep, src
        out = dict(rgb=rgb, depth=depth, n_vertices=int(a.n_vertices), n_drawn_points=int(a.n_drawn_points), n_segments=int(a.n_segments),
                   n_line_samples=int(a.n_line_samples))
        out.update({k: int(getattr(m, k)) for k in MESH_COUNTS})
        return out

    # ---- the keyframe graph: EnergyFunctional::connectivityMap from the device chain
    def map_graph_enable(self, on=True):
        """nalo_map_graph_enable: the pairs of the frames that share a window from now on, and the residuals marginalised between them"""
        self._ck(self.L.nalo_map_graph_enable(self.h_, int(bool(on))))

    def _graph_get(self, fn, dtype):
        cap = getattr(self, "_graph_cap", 512)                                    # one device call unless the table has outgrown the last answer
        while True:
            out, n = np.zeros(cap, dtype), C.c_int(-1)
            rc = fn(self.h_, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
            if rc != 0 and n.value > cap:
                cap = self._graph_cap = 2 * n.value
                continue
            self._ck(rc)
            return out[:n.value].copy()

    def map_graph(self):
        """connectivityMap: every entry (GRAPH_EDGE_DTYPE) in key order, act = [0], marg = [1]"""
        return self._graph_get(self.L.nalo_map_graph, GRAPH_EDGE_DTYPE)

    def map_graph_connections(self):
        """PangolinDSOViewer::publishGraph's connections (GRAPH_CONNECTION_DTYPE), frame ids for the KeyFrameDisplay pointers"""
        return self._graph_get(self.L.nalo_map_graph_connections, GRAPH_CONNECTION_DTYPE)

    # ---- the dense map: updateMap in one call, mapPoints archived on the device
    def map_dense_enable(self, on=True, chunk_points=0):
        self._ck(self.L.nalo_map_dense_enable(self.h_, int(bool(on)), int(chunk_points)))

    def dense_update_map(self, host_frame, draws, cam_to_world, threshold=0.01, min_points=10, cap=2048, null_runs=False):
        """updateMap for one window frame (nalo_dense_update_map) -> (clusters PLANE_DTYPE[C], runs DENSE_RUN_DTYPE[C], n_appended); self.plane_n_clusters holds
        the count after a refusal too; cam_to_world=None and null_runs pass NULL"""
        m = None if cam_to_world is None else np.ascontiguousarray(cam_to_world, np.float64).reshape(-1)
        assert m is None or m.size == 12
        runs = np.zeros(max(cap, 1), DENSE_RUN_DTYPE)
        napp = np.zeros(1, np.int32)
        call = lambda a, cap_, o, n: self.L.nalo_dense_update_map(self.h_, int(host_frame), a, None if m is None else _d(m), cap_, o,
                                                                  None if null_runs else runs.ctypes.data_as(C.c_void_p), n, _i(napp))
        recs, n = self._fit_planes(call, draws, threshold, min_points, 0, cap)
        return recs, runs[:n].copy(), int(napp[0])

    def map_dense_counts(self, frame_id):
        """(points, appended cluster runs) of the frame's dense list"""
        a, b = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.L.nalo_map_dense_counts(self.h_, int(frame_id), _i(a), _i(b)))
        return int(a[0]), int(b[0])

    def map_dense_get(self, frame_id):
        """the frame's dense points (DENSE_POINT_DTYPE) in append order"""
        n = C.c_int(0)
        rc = self.L.nalo_map_dense_get(self.h_, int(frame_id), None, 0, C.byref(n))
        if n.value == 0:
            self._ck(rc)
        pts = np.zeros(n.value, DENSE_POINT_DTYPE)
        if n.value:
            self._ck(self.L.nalo_map_dense_get(self.h_, int(frame_id), pts.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return pts

    def map_dense_world_points(self, frame_id, cam_to_world):
        """SampleOutputWrapper's tsdf=1 loop: the world points [n][3] (float64) of the frame's dense points"""
        m = np.ascontiguousarray(cam_to_world, np.float64).reshape(-1)
        assert m.size == 12
        n = C.c_int(0)
        rc = self.L.nalo_map_dense_world_points(self.h_, int(frame_id), _d(m), None, 0, C.byref(n))
        if n.value == 0:
            self._ck(rc)
        xyz = np.zeros((n.value, 3), np.float64)
        if n.value:
            self._ck(self.L.nalo_map_dense_world_points(self.h_, int(frame_id), _d(m), _d(xyz), n.value, C.byref(n)))
        return xyz

    # ---- the TSDF volume (nalo_tsdf_*)
    def tsdf_create(self, origin, voxel_size, dims, trunc, max_weight):
        """nalo_tsdf_create: a dense volume [nz][ny][nx] (tsdf 1.0, weight 0.0) in this context; a second call replaces it"""
        d = tsdf_desc(origin, voxel_size, dims, trunc, max_weight)
        self._ck(self.L.nalo_tsdf_create(self.h_, C.byref(d)))
        self.tsdf_dims = tuple(int(v) for v in dims)

    def tsdf_reset(self):
        self._ck(self.L.nalo_tsdf_reset(self.h_))

    def tsdf_destroy(self):
        self._ck(self.L.nalo_tsdf_destroy(self.h_))

    def tsdf_shift(self, shift):
        """nalo_tsdf_shift: voxel (i, j, k) takes the words of voxel (i + s0, j + s1, k + s2), the initial values where that lies outside the grid, and the origin
        moves by s voxels: the box follows the camera. Enqueues only once the spare arrays exist (the first non-zero shift allocates them: a shifted volume holds
        twice its memory). tsdf_view / tsdf_color_view taken before a non-zero shift are stale after it; tsdf_last needs a new integration"""
        s = np.ascontiguousarray(shift, np.int32).reshape(-1)
        if s.size != 3:
            raise NaloError("tsdf_shift: shift is three whole voxels")
        self._ck(self.L.nalo_tsdf_shift(self.h_, _i(s)))

    def tsdf_geometry(self):
        """nalo_tsdf_geometry -> dict(desc (a TsdfDesc with the CURRENT origin: what tsdf_frustum_box and a twin's tsdf_create take), origin, origin0 float32 [3],
        base int32 [3], voxel_size, dims); launches nothing"""
        g = TsdfGeometry()
        self._ck(self.L.nalo_tsdf_geometry(self.h_, C.byref(g)))
        return dict(desc=g.desc, origin=np.array(g.desc.origin[:], np.float32), origin0=np.array(g.origin0[:], np.float32), base=np.array(g.base[:], np.int32),
                    voxel_size=np.float32(g.desc.voxel_size), dims=tuple(g.desc.dims[:]))

    def tsdf_color_enable(self):
        """nalo_tsdf_color_enable: three float32 planes [3][nz][ny][nx] (B, G, R) at 0.0 next to the volume; enable before the first integration if the colour is to
        be the average of every observation"""
        self._ck(self.L.nalo_tsdf_color_enable(self.h_))

    def tsdf_color_disable(self):
        self._ck(self.L.nalo_tsdf_color_disable(self.h_))

    def tsdf_color_get(self, lo=None, size=None):
        """nalo_tsdf_color_get -> float32 [3][sz][sy][sx] (planes B, G, R) of the sub-block [lo, lo + size); the whole grid by default"""
        lo_a = np.zeros(3, np.int32) if lo is None else np.ascontiguousarray(lo, np.int32)
        size_a = np.asarray(self.tsdf_dims, np.int32) if size is None else np.ascontiguousarray(size, np.int32)
        out = np.zeros((3,) + tuple(max(int(v), 0) for v in size_a[::-1]), np.float32)
        self._ck(self.L.nalo_tsdf_color_get(self.h_, _i(lo_a), _i(size_a), _f(out)))
        return out

    def tsdf_color_set(self, lo, bgr):
        """nalo_tsdf_color_set: a float32 block [3][sz][sy][sx] written at lo, bit for bit"""
        b = np.ascontiguousarray(bgr, np.float32)
        if b.ndim != 4 or b.shape[0] != 3:
            raise NaloError("tsdf_color_set: bgr is a [3][sz][sy][sx] block")
        lo_a, size_a = np.ascontiguousarray(lo, np.int32), np.asarray(b.shape[:0:-1], np.int32)
        self._ck(self.L.nalo_tsdf_color_set(self.h_, _i(lo_a), _i(size_a), _f(b)))

    def tsdf_color_view(self):
        """nalo_tsdf_color_view -> a DeviceView of shape [3, nz, ny, nx] (planes B, G, R): torch.as_tensor(view, device="cuda") is a zero-copy tensor. Launches
        nothing."""
        v = TsdfColorVolumeView()
        self._ck(self.L.nalo_tsdf_color_view(self.h_, C.byref(v)))
        return DeviceView(v.bgr, (3, v.dims[2], v.dims[1], v.dims[0]), "<f4", None, v.stream, self)

    def tsdf_integrate_depth(self, depth, K, cam_to_world, min_depth, max_depth, stream=None, release=True, colour=None, colour_is_rgb=False):
        """nalo_tsdf_integrate_depth: depth is a 2-D float32 device array (anything with __cuda_array_interface__, or a DevPlane), read where it lies through its
        strides; K = (fx, fy, cx, cy) for ITS size. stream / release as frame_ingest: the producing hipStream_t (None: torch's current stream of a tensor, a
        DeviceView's own, else the null stream), and whether that stream waits on the device until the plane has been read. Returns without waiting.
        colour (a uint8 device array [h][w][3], or a DevPlane of three channels) routes to nalo_tsdf_integrate_depth_color; colour_is_rgb: channel 0 is R."""
        a = TsdfIntegrateArgs()
        a.depth = depth if isinstance(depth, DevPlane) else dev_plane(depth)
        if stream is None:
            stream = 0
            torch = sys.modules.get("torch")
            if isinstance(depth, DeviceView):
                stream = depth.stream
            elif torch is not None and isinstance(depth, torch.Tensor):
                stream = torch.cuda.current_stream(depth.device).cuda_stream
        a.K[:] = [float(v) for v in K]
        a.camToWorld[:] = [float(v) for v in np.asarray(cam_to_world, np.float64).reshape(-1)]
        a.min_depth, a.max_depth, a.producer_stream = float(min_depth), float(max_depth), stream or None
        if colour is None:
            self._ck(self.L.nalo_tsdf_integrate_depth(self.h_, C.byref(a)))
        else:
            cp = colour if isinstance(colour, DevPlane) else dev_plane(colour, "hwc")
            self._ck(self.L.nalo_tsdf_integrate_depth_color(self.h_, C.byref(a), C.byref(cp), int(bool(colour_is_rgb))))
        if release:
            self.tsdf_release(stream)

    def tsdf_release(self, stream):
        """nalo_tsdf_release: `stream` (a hipStream_t as an int, 0 / None the null stream) waits on the device until the last integration has read its plane"""
        self._ck(self.L.nalo_tsdf_release(self.h_, stream or None))

    def tsdf_integrate_frame(self, frame_id, cam_to_world, K, min_depth, max_depth):
        """nalo_tsdf_integrate_frame: the frame's dense list (nalo_dense_update_map) as a depth plane, integrated with the pose given here"""
        m = np.ascontiguousarray(cam_to_world, np.float64).reshape(-1)
        Kf = np.ascontiguousarray(K, np.float32).reshape(-1)
        assert m.size == 12 and Kf.size == 4
        self._ck(self.L.nalo_tsdf_integrate_frame(self.h_, int(frame_id), _d(m), _f(Kf), C.c_float(min_depth), C.c_float(max_depth)))

    def tsdf_last(self):
        """nalo_tsdf_last -> dict(lo, hi, visited, updated) of the last integration (hi exclusive); waits"""
        st = TsdfStats()
        self._ck(self.L.nalo_tsdf_last(self.h_, C.byref(st)))
        return dict(lo=tuple(st.lo), hi=tuple(st.hi), visited=int(st.visited), updated=int(st.updated))

    def tsdf_replace_depth(self, remove=None, add=None, box=None, stream=None, release=True):
        """nalo_tsdf_replace_depth: per voxel the removal of side `remove`, then the add of side `add` (tsdf_side() builds them; either may be None), in one
        launch. box = (lo, size) restricts the REMOVE side to those voxels. stream / release as tsdf_integrate_depth; None: the stream tsdf_side() found for
        the ADD side's depth plane, else the remove side's. ONE stream is waited for and released: a caller whose planes (the two sides', or a colour plane)
        come from more than one producer passes `stream` and orders the others behind it, or synchronises first. Returns without waiting."""
        a = TsdfReplaceArgs()
        if remove is not None:
            a.remove = C.pointer(remove)
        if add is not None:
            a.add = C.pointer(add)
        if box is not None:
            a.use_box = 1
            a.lo[:] = [int(v) for v in box[0]]
            a.size[:] = [int(v) for v in box[1]]
        if stream is None:
            stream = next((sd.stream for sd in (add, remove) if sd is not None and getattr(sd, "stream", 0)), 0)
        a.producer_stream = stream or None
        self._ck(self.L.nalo_tsdf_replace_depth(self.h_, C.byref(a)))
        if release:
            self.tsdf_release(stream)

    def tsdf_replace_last(self):
        """nalo_tsdf_replace_last -> dict(lo, hi, visited, removed, reset, added, written) of the last replacement (hi exclusive); waits"""
        st = TsdfReplaceStats()
        self._ck(self.L.nalo_tsdf_replace_last(self.h_, C.byref(st)))
        return dict(lo=tuple(st.lo), hi=tuple(st.hi), visited=int(st.visited), removed=int(st.removed), reset=int(st.reset), added=int(st.added), written=int(st.written))

    def tsdf_replace_frame(self, frame_id, cam_to_world, K, min_depth, max_depth, s=1.0):
        """nalo_tsdf_replace_frame: the logged contribution of the frame removed and its dense list as it is now fused at (cam_to_world, s); cam_to_world None:
        remove only. Needs tsdf_log_enable and the dense archive"""
        Kf = np.ascontiguousarray(K, np.float32).reshape(-1)
        assert Kf.size == 4
        e = None if cam_to_world is None else C.byref(tsdf_align_est(cam_to_world, s))
        self._ck(self.L.nalo_tsdf_replace_frame(self.h_, int(frame_id), e, _f(Kf), C.c_float(min_depth), C.c_float(max_depth)))

    def tsdf_replace_depth_n(self, pairs, release=True):
        """nalo_tsdf_replace_depth_n: the chain tsdf_replace_depth(pairs[0]), tsdf_replace_depth(pairs[1]), ... per voxel in ONE launch. pairs: a list (1 .. 16) of
        dict(remove=, add=, box=, stream=) with tsdf_replace_depth's meanings, or of (remove, add) / (remove, add, box) tuples. Every distinct producer stream of
        the list is waited for on the device, and released when `release`. Returns without waiting."""
        n = len(pairs)
        arr = (TsdfReplaceArgs * max(n, 1))()
        streams = []
        for k, p in enumerate(pairs):
            if not isinstance(p, dict):
                p = dict(zip(("remove", "add", "box"), p))
            remove, add, box, stream = p.get("remove"), p.get("add"), p.get("box"), p.get("stream")
            a = arr[k]
            if remove is not None:
                a.remove = C.pointer(remove)
            if add is not None:
                a.add = C.pointer(add)
            if box is not None:
                a.use_box = 1
                a.lo[:] = [int(v) for v in box[0]]
                a.size[:] = [int(v) for v in box[1]]
            if stream is None:
                stream = next((sd.stream for sd in (add, remove) if sd is not None and getattr(sd, "stream", 0)), 0)
            a.producer_stream = stream or None
            if stream not in streams:
                streams.append(stream)
        self._ck(self.L.nalo_tsdf_replace_depth_n(self.h_, arr if n else None, n))
        if release:
            for st in streams:
                self.tsdf_release(st)

    def tsdf_replace_last_n(self):
        """nalo_tsdf_replace_last_n -> (total, per_pair): total as tsdf_replace_last (written: the voxels where any pair fired, each once), per_pair a list of
        dict(removed, reset, added, written); waits"""
        st, rows, n = TsdfReplaceStats(), (TsdfReplacePairStats * 16)(), np.zeros(1, np.int32)
        self._ck(self.L.nalo_tsdf_replace_last_n(self.h_, C.byref(st), rows, 16, _i(n)))
        total = dict(lo=tuple(st.lo), hi=tuple(st.hi), visited=int(st.visited), removed=int(st.removed), reset=int(st.reset), added=int(st.added), written=int(st.written))
        return total, [dict(removed=int(r.removed), reset=int(r.reset), added=int(r.added), written=int(r.written)) for r in rows[:int(n[0])]]

    def tsdf_replace_frames(self, frame_ids, cam_to_world, K, min_depth, max_depth, s=1.0, skip_unchanged=False):
        """nalo_tsdf_replace_frames: tsdf_replace_frame for every frame of the list, in order, in ONE launch, the log updated all or nothing. Arguments as
        tsdf_replace_frames_args(). Returns n_skipped."""
        a = tsdf_replace_frames_args(frame_ids, cam_to_world, K, min_depth, max_depth, s, skip_unchanged)
        self._ck(self.L.nalo_tsdf_replace_frames(self.h_, C.byref(a)))
        return int(a.n_skipped)

    def tsdf_log_enable(self, on=True):
        """nalo_tsdf_log_enable: the fusion log, what tsdf_replace_frame removes by; off by default, and off it changes nothing. Turning it off clears it"""
        self._ck(self.L.nalo_tsdf_log_enable(self.h_, int(bool(on))))

    def tsdf_log_get(self):
        """nalo_tsdf_log_get -> a list of dict(frame_id, n_records, cam_to_world [3][4], s, K, min_depth, max_depth, lo, size, coloured) in the order the frames were
        first fused; launches nothing"""
        n = np.zeros(1, np.int32)
        self._ck(self.L.nalo_tsdf_log_get(self.h_, None, 0, _i(n)))
        out = (TsdfLogEntry * max(int(n[0]), 1))()
        self._ck(self.L.nalo_tsdf_log_get(self.h_, out, int(n[0]), _i(n)))
        return [dict(frame_id=int(e.frame_id), n_records=int(e.n_records), cam_to_world=_align_est(e.est)[0], s=float(e.est.s), K=tuple(float(k) for k in e.K),
                     min_depth=float(e.min_depth), max_depth=float(e.max_depth), lo=tuple(e.lo), size=tuple(e.size), coloured=bool(e.coloured)) for e in out[:int(n[0])]]

    def tsdf_get(self, lo=None, size=None):
        """nalo_tsdf_get -> (tsdf, weight) of the sub-block [lo, lo + size) as float32 [sz][sy][sx]; the whole grid by default"""
        lo_a = np.zeros(3, np.int32) if lo is None else np.ascontiguousarray(lo, np.int32)
        size_a = np.asarray(self.tsdf_dims, np.int32) if size is None else np.ascontiguousarray(size, np.int32)
        shape = tuple(max(int(v), 0) for v in size_a[::-1])
        t, w = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self._ck(self.L.nalo_tsdf_get(self.h_, _i(lo_a), _i(size_a), _f(t), _f(w)))
        return t, w

    def tsdf_set(self, lo, tsdf=None, weight=None):
        """nalo_tsdf_set: float32 blocks [sz][sy][sx] written at lo, bit for bit; either may be None"""
        t = None if tsdf is None else np.ascontiguousarray(tsdf, np.float32)
        w = None if weight is None else np.ascontiguousarray(weight, np.float32)
        ref = t if t is not None else w
        if ref is None or ref.ndim != 3 or (t is not None and w is not None and t.shape != w.shape):
            raise NaloError("tsdf_set: tsdf and / or weight as [sz][sy][sx] blocks of one shape")
        lo_a, size_a = np.ascontiguousarray(lo, np.int32), np.asarray(ref.shape[::-1], np.int32)
        self._ck(self.L.nalo_tsdf_set(self.h_, _i(lo_a), _i(size_a), _f(t), _f(w)))

    def tsdf_view(self):
        """nalo_tsdf_view -> (tsdf, weight) as DeviceViews of shape [nz, ny, nx]: torch.as_tensor(view, device="cuda") is a zero-copy tensor. Launches nothing."""
        v = TsdfVolumeView()
        self._ck(self.L.nalo_tsdf_view(self.h_, C.byref(v)))
        shape = (v.dims[2], v.dims[1], v.dims[0])
        return DeviceView(v.tsdf, shape, "<f4", None, v.stream, self), DeviceView(v.weight, shape, "<f4", None, v.stream, self)

    def tsdf_surface_points(self, min_weight, lo=None, size=None, cap=None):
        """nalo_tsdf_surface_points -> float32 [n][3], in (k, j, i, axis) order, over the sub-box [lo, lo + size) or the whole grid. With cap (room for that
        many points, e.g. the count of the last call plus a margin) it is ONE library call and one wait, refused with NaloError when the surface has more points;
        without it the library is called twice, first with cap = 0 for n_needed (count and scan run twice, two waits). self.tsdf_surface_needed holds n_needed
        after either, a refusal included"""
        a = TsdfSurfaceArgs()
        if lo is not None:
            a.use_box = 1
            a.lo[:] = [int(v) for v in lo]
            a.size[:] = [int(v) for v in size]
        a.min_weight = float(min_weight)
        if cap is None:
            rc = self.L.nalo_tsdf_surface_points(self.h_, C.byref(a))            # cap = 0: answers n_needed (and is the whole call without a crossing)
            self.tsdf_surface_needed = int(a.n_needed)
            if a.n_needed == 0:
                self._ck(rc)
                return np.zeros((0, 3), np.float32)
            cap = int(a.n_needed)
        xyz = np.zeros((max(int(cap), 0), 3), np.float32)
        a.cap, a.xyz = int(cap), _f(xyz)
        rc = self.L.nalo_tsdf_surface_points(self.h_, C.byref(a))
        self.tsdf_surface_needed = int(a.n_needed)
        self._ck(rc)
        return xyz[:int(a.n)].copy()

    def tsdf_mesh(self, min_weight, lo=None, size=None, download=True, colour=False):
        """nalo_tsdf_mesh -> (xyz float32 [nv][3], tri int32 [nt][3]): the marching-tetrahedra mesh of the sub-box [lo, lo + size) or of the whole grid, in the
        header's order. The mesh is always built on the device (tsdf_mesh_view); download=False returns the counts (nv, nt) only, after one library call and one
        wait. With the download the arrays are sized from that call's counts and a second call fills them. self.tsdf_mesh_counts holds the counts of the last
        call, a refusal included. colour=True: nalo_tsdf_mesh_color -> (xyz, tri, rgba uint8 [nv][4]), the colours on the device under tsdf_mesh_color_view"""
        cc = TsdfMeshColorArgs()
        call = (lambda a: self.L.nalo_tsdf_mesh_color(self.h_, C.byref(a), C.byref(cc))) if colour else (lambda a: self.L.nalo_tsdf_mesh(self.h_, C.byref(a)))
        a = TsdfMeshArgs()
        if lo is not None:
            a.use_box = 1
            a.lo[:] = [int(v) for v in lo]
            a.size[:] = [int(v) for v in size]
        a.min_weight = float(min_weight)
        rc = call(a)
        self.tsdf_mesh_counts = (int(a.n_vertices), int(a.n_triangles))
        self._ck(rc)
        if not download:
            return self.tsdf_mesh_counts
        nv, nt = self.tsdf_mesh_counts
        xyz, tri, rgba = np.zeros((nv, 3), np.float32), np.zeros((nt, 3), np.int32), np.zeros((nv, 4), np.uint8)
        if nv == 0 and nt == 0:
            return (xyz, tri, rgba) if colour else (xyz, tri)
        a.cap_vertices, a.cap_triangles, a.xyz, a.tri = nv, nt, (_f(xyz) if nv else None), (_i(tri) if nt else None)
        cc.cap, cc.rgba = nv, (_u8(rgba) if nv else None)
        rc = call(a)
        self.tsdf_mesh_counts = (int(a.n_vertices), int(a.n_triangles))
        self._ck(rc)
        return (xyz, tri, rgba) if colour else (xyz, tri)

    def tsdf_mesh_view(self):
        """nalo_tsdf_mesh_view -> (xyz, tri) as DeviceViews of shape [nv, 3] float32 and [nt, 3] int32: torch.as_tensor(view, device="cuda") is a zero-copy
        tensor of the device mesh the last tsdf_mesh built. Launches nothing; good until the next tsdf_mesh / tsdf_create / tsdf_destroy / close."""
        v = TsdfMeshDev()
        self._ck(self.L.nalo_tsdf_mesh_view(self.h_, C.byref(v)))
        return DeviceView(v.xyz, (v.n_vertices, 3), "<f4", None, v.stream, self), DeviceView(v.tri, (v.n_triangles, 3), "<i4", None, v.stream, self)

    def tsdf_mesh_color_view(self):
        """nalo_tsdf_mesh_color_view -> a DeviceView of shape [nv, 4] uint8 (R, G, B, 255): the colours of the device mesh the last tsdf_mesh(colour=True) built.
        Launches nothing; a plain tsdf_mesh afterwards invalidates it."""
        v = TsdfMeshColorDev()
        self._ck(self.L.nalo_tsdf_mesh_color_view(self.h_, C.byref(v)))
        return DeviceView(v.rgba, (v.n_vertices, 4), "|u1", None, v.stream, self)

    def tsdf_raycast(self, w, h, K, cam_to_world, min_depth, max_depth, step, min_weight, normals=False, colour=False, download=True):
        """nalo_tsdf_raycast -> dict(depth float32 [h][w], normal float32 [h][w][3] (normals), rgba uint8 [h][w][4] (colour), n_hit, n_back, n_normal, n_steps):
        the volume's first front face along every pixel's ray of a w x h view with K = (fx, fy, cx, cy), sampled at z_n = min_depth + n * step <= max_depth.
        A miss has depth 0. One library call and one wait; download=False leaves the images on the device (tsdf_raycast_view) and returns the counts only.
        self.tsdf_raycast_counts holds (n_hit, n_back, n_normal, n_steps) of the last call, a refusal included"""
        a = TsdfRaycastArgs()
        a.w, a.h = int(w), int(h)
        a.K[:] = [float(v) for v in K]
        a.camToWorld[:] = [float(v) for v in np.asarray(cam_to_world, np.float64).reshape(-1)]
        a.min_depth, a.max_depth, a.step, a.min_weight = float(min_depth), float(max_depth), float(step), float(min_weight)
        a.with_normals, a.with_colour = int(bool(normals)), int(bool(colour))
        out = {}
        if download and a.w > 0 and a.h > 0:
            out["depth"] = np.zeros((a.h, a.w), np.float32)
            a.depth = _f(out["depth"])
            if normals:
                out["normal"] = np.zeros((a.h, a.w, 3), np.float32)
                a.normal = _f(out["normal"])
            if colour:
                out["rgba"] = np.zeros((a.h, a.w, 4), np.uint8)
                a.rgba = _u8(out["rgba"])
        rc = self.L.nalo_tsdf_raycast(self.h_, C.byref(a))
        self.tsdf_raycast_counts = (int(a.n_hit), int(a.n_back), int(a.n_normal), int(a.n_steps))
        self._ck(rc)
        out.update(n_hit=int(a.n_hit), n_back=int(a.n_back), n_normal=int(a.n_normal), n_steps=int(a.n_steps))
        return out

    def tsdf_raycast_view(self):
        """nalo_tsdf_raycast_view -> dict(depth [h, w] float32, normal [h, w, 3] float32 or None, rgba [h, w, 4] uint8 or None) of DeviceViews on the images the
        last tsdf_raycast wrote: torch.as_tensor(view, device="cuda") is a zero-copy tensor, and the depth view is what tsdf_integrate_depth takes as it is.
        Launches nothing; good until the next tsdf_raycast / tsdf_create / tsdf_destroy / close"""
        v = TsdfRaycastDev()
        self._ck(self.L.nalo_tsdf_raycast_view(self.h_, C.byref(v)))
        return dict(depth=DeviceView(v.depth.ptr, (v.h, v.w), "<f4", None, v.stream, self),
                    normal=DeviceView(v.normal.ptr, (v.h, v.w, 3), "<f4", None, v.stream, self) if v.normal.ptr else None,
                    rgba=DeviceView(v.rgba.ptr, (v.h, v.w, 4), "|u1", None, v.stream, self) if v.rgba.ptr else None)

    # ---- the alignment (nalo_tsdf_align_*)
    def _align_args(self, depth, K, min_depth, max_depth, min_weight, huber, step, dof, stream, records, max_iterations=1, min_used=1, lambda0=0.0, eps=0.0):
        a = TsdfAlignArgs()
        if depth is not None:
            a.depth = depth if isinstance(depth, DevPlane) else dev_plane(depth)
        if stream is None:
            stream = 0
            torch = sys.modules.get("torch")
            if isinstance(depth, DeviceView):
                stream = depth.stream
            elif torch is not None and isinstance(depth, torch.Tensor):
                stream = torch.cuda.current_stream(depth.device).cuda_stream
        a.K[:] = [float(v) for v in K]
        a.min_depth, a.max_depth, a.min_weight, a.huber = float(min_depth), float(max_depth), float(min_weight), float(huber)
        a.step, a.dof, a.producer_stream = int(step), int(dof), stream or None
        if records is not None:
            cai = records.__cuda_array_interface__
            if cai["typestr"] != "<f4" or cai.get("strides") is not None:
                raise NaloError("tsdf_align: records is a contiguous float32 device array")
            a.records, a.records_cap = int(cai["data"][0]) or None, int(np.prod(cai["shape"]))
        a.max_iterations, a.min_used, a.lambda0, a.eps = int(max_iterations), int(min_used), float(lambda0), float(eps)
        return a, stream

    def tsdf_align_eval(self, depth, K, cam_to_world, s=1.0, min_depth=0.0, max_depth=1e30, min_weight=1.0, huber=1.0, step=1, dof=6, stream=None, release=True, records=None):
        """nalo_tsdf_align_eval -> dict(H float64 [28] (upper triangle, row-major), b [7], E, rr, count (used, no depth, no field, no gradient)): one evaluation of
        the depth plane (as tsdf_integrate_depth takes it, K for ITS size) against the volume at the estimate (camToWorld, s). records: a contiguous float32
        device array of at least h w 10 elements, written at visited pixels as [h][w][10] = r, hw, J0..J6, state. One launch, one wait.
        self.tsdf_align_counts holds the counts of the last call, a refusal included"""
        a, stream = self._align_args(depth, K, min_depth, max_depth, min_weight, huber, step, dof, stream, records)
        e, S = tsdf_align_est(cam_to_world, s), TsdfAlignSums()
        rc = self.L.nalo_tsdf_align_eval(self.h_, C.byref(a), C.byref(e), C.byref(S))
        self.tsdf_align_counts = tuple(int(v) for v in S.count)
        self._ck(rc)
        if release:
            self.tsdf_release(stream)
        return _align_sums(S)

    def _align_result(self, rc, r, trace):
        self.tsdf_align_counts = (int(r.iterations), int(r.evaluations), int(r.n_first), int(r.n_last), int(r.n_trace))
        self._ck(rc)
        T, s = _align_est(r.est)
        tr = []
        for t in trace[:r.n_trace]:
            Tt, st = _align_est(t.est)
            tr.append(dict(cam_to_world=Tt, s=st, lam=float(t.lambda_), E=float(t.E), count=tuple(int(v) for v in t.count), accepted=bool(t.accepted)))
        return dict(cam_to_world=T, s=s, status=int(r.status), iterations=int(r.iterations), evaluations=int(r.evaluations), E_first=float(r.E_first), E_last=float(r.E_last),
                    n_first=int(r.n_first), n_last=int(r.n_last), last=_align_sums(r.last), trace=tr)

    def tsdf_align_depth(self, depth, K, cam_to_world, s=1.0, min_depth=0.0, max_depth=1e30, min_weight=1.0, huber=1.0, step=1, dof=6, max_iterations=12, min_used=1,
                         lambda0=0.0, eps=1e-6, trace_cap=ALIGN_MAX_EVALUATIONS, stream=None, release=True, records=None):
        """nalo_tsdf_align_depth -> dict(cam_to_world [3][4], s, status (ALIGN_*), iterations, evaluations, E_first, E_last, n_first, n_last, last (the sums at
        the answer), trace: one dict(cam_to_world, s, lam, E, count, accepted) per evaluation, at most trace_cap): the Levenberg-Marquardt alignment of the depth
        plane against the volume from the start (cam_to_world, s). One launch and one wait per evaluation.
        self.tsdf_align_counts holds (iterations, evaluations, n_first, n_last, n_trace) of the last call, a refusal included"""
        a, stream = self._align_args(depth, K, min_depth, max_depth, min_weight, huber, step, dof, stream, records, max_iterations, min_used, lambda0, eps)
        e, r = tsdf_align_est(cam_to_world, s), TsdfAlignResult()
        trace = (TsdfAlignTrace * max(int(trace_cap), 1))()
        r.trace, r.trace_cap = trace, int(trace_cap)
        rc = self.L.nalo_tsdf_align_depth(self.h_, C.byref(a), C.byref(e), C.byref(r))
        out = self._align_result(rc, r, trace)
        if release:
            self.tsdf_release(stream)
        return out

    def tsdf_align_frame(self, frame_id, K, cam_to_world, s=1.0, min_depth=0.0, max_depth=1e30, min_weight=1.0, huber=1.0, step=1, dof=6, max_iterations=12, min_used=1,
                         lambda0=0.0, eps=1e-6, trace_cap=ALIGN_MAX_EVALUATIONS):
        """nalo_tsdf_align_frame: tsdf_align_depth on the plane tsdf_integrate_frame would integrate (the frame's dense list, K for the context's size)"""
        a, _ = self._align_args(None, K, min_depth, max_depth, min_weight, huber, step, dof, 0, None, max_iterations, min_used, lambda0, eps)
        e, r = tsdf_align_est(cam_to_world, s), TsdfAlignResult()
        trace = (TsdfAlignTrace * max(int(trace_cap), 1))()
        r.trace, r.trace_cap = trace, int(trace_cap)
        rc = self.L.nalo_tsdf_align_frame(self.h_, int(frame_id), C.byref(a), C.byref(e), C.byref(r))
        return self._align_result(rc, r, trace)

    # ---- the mesh archive (nalo_tsdf_archive_*)
    @staticmethod
    def _archive_stats(st):
        return dict(added_vertices=int(st.added_vertices), welded_vertices=int(st.welded_vertices), added_triangles=int(st.added_triangles), n_vertices=int(st.n_vertices),
                    n_triangles=int(st.n_triangles), cap_vertices=int(st.cap_vertices), cap_triangles=int(st.cap_triangles), table_slots=int(st.table_slots),
                    coloured=bool(st.coloured), have_lattice=bool(st.have_lattice), origin0=np.array(st.origin0, np.float32), voxel_size=np.float32(st.voxel_size))

    def tsdf_archive_enable(self):
        """nalo_tsdf_archive_enable: an empty welded mesh archive in this context, coloured iff the volume's colour is enabled now; it outlives volumes"""
        self._ck(self.L.nalo_tsdf_archive_enable(self.h_))

    def tsdf_archive_disable(self):
        self._ck(self.L.nalo_tsdf_archive_disable(self.h_))

    def tsdf_archive_reset(self):
        """nalo_tsdf_archive_reset: empties the archive, keeps its buffers and colour state, forgets its lattice"""
        self._ck(self.L.nalo_tsdf_archive_reset(self.h_))

    def tsdf_archive_stats(self):
        """nalo_tsdf_archive_stats -> dict(added_vertices, welded_vertices, added_triangles (the last tsdf_archive_mesh), n_vertices, n_triangles, cap_vertices,
        cap_triangles, table_slots, coloured, have_lattice, origin0, voxel_size). Launches nothing"""
        st = TsdfArchiveStats()
        self._ck(self.L.nalo_tsdf_archive_stats(self.h_, C.byref(st)))
        return self._archive_stats(st)

    def tsdf_archive_mesh(self, min_weight, box=None):
        """nalo_tsdf_archive_mesh: tsdf_mesh of box = (lo, size) (None: the whole grid), left on the device, and its append to the archive: a vertex whose key
        (global voxel, edge) the archive holds is welded to the archived one, the others and every triangle are added at the end. -> the dict of
        tsdf_archive_stats. self.tsdf_mesh_counts holds the piece's counts, a refusal included"""
        a, st = TsdfMeshArgs(), TsdfArchiveStats()
        if box is not None:
            a.use_box = 1
            a.lo[:] = [int(v) for v in box[0]]
            a.size[:] = [int(v) for v in box[1]]
        a.min_weight = float(min_weight)
        rc = self.L.nalo_tsdf_archive_mesh(self.h_, C.byref(a), C.byref(st))
        self.tsdf_mesh_counts = (int(a.n_vertices), int(a.n_triangles))
        self._ck(rc)
        return self._archive_stats(st)

    def tsdf_archive_get(self, keys=False):
        """nalo_tsdf_archive_get -> xyz float32 [nv][3], tri int32 [nt][3][, rgba uint8 [nv][4] of a coloured archive][, key int32 [nv][4] = (gx, gy, gz, m)]:
        the whole archive, sized from tsdf_archive_stats; what write_ply_mesh takes as it comes"""
        st = self.tsdf_archive_stats()
        nv, nt = st["n_vertices"], st["n_triangles"]
        xyz, tri = np.zeros((nv, 3), np.float32), np.zeros((nt, 3), np.int32)
        rgba = np.zeros((nv, 4), np.uint8) if st["coloured"] else None
        key = np.zeros((nv, 4), np.int32) if keys else None
        a = TsdfArchiveGetArgs()
        a.cap_vertices, a.xyz = nv, (_f(xyz) if nv else None)
        a.cap_triangles, a.tri = nt, (_i(tri) if nt else None)
        if rgba is not None:
            a.cap_rgba, a.rgba = nv, (_u8(rgba) if nv else None)
        if key is not None:
            a.cap_key, a.key = nv, (_i(key) if nv else None)
        self._ck(self.L.nalo_tsdf_archive_get(self.h_, C.byref(a)))
        return tuple(x for x in (xyz, tri, rgba, key) if x is not None)

    def tsdf_archive_view(self):
        """nalo_tsdf_archive_view -> dict(xyz [nv, 3] float32, tri [nt, 3] int32, rgba [nv, 4] uint8 or None, key [nv, 4] int32) of DeviceViews:
        torch.as_tensor(view, device="cuda") is a zero-copy tensor. Launches nothing; good until a tsdf_archive_mesh that grows a buffer, tsdf_archive_reset,
        tsdf_archive_disable or close"""
        v = TsdfArchiveDev()
        self._ck(self.L.nalo_tsdf_archive_view(self.h_, C.byref(v)))
        nv, nt = v.n_vertices, v.n_triangles
        return dict(xyz=DeviceView(v.xyz, (nv, 3), "<f4", None, v.stream, self), tri=DeviceView(v.tri, (nt, 3), "<i4", None, v.stream, self),
                    rgba=DeviceView(v.rgba, (nv, 4), "|u1", None, v.stream, self) if v.rgba else None, key=DeviceView(v.key, (nv, 4), "<i4", None, v.stream, self))

    def tsdf_follow(self, centre, margin, min_weight):
        """nalo_tsdf_follow: tsdf_geometry, tsdf_shift_for(centre, margin), tsdf_archive_mesh of every box of tsdf_shift_boxes in order, tsdf_shift, as one call
        -> dict(shift int32 [3], n_boxes, added_vertices, welded_vertices, added_triangles, n_vertices, n_triangles)"""
        ce = np.ascontiguousarray(centre, np.float64).reshape(-1)
        mg = np.ascontiguousarray(margin, np.int32).reshape(-1)
        if ce.size != 3 or mg.size != 3:
            raise NaloError("tsdf_follow: centre and margin hold three values each")
        shift, st = np.zeros(3, np.int32), TsdfFollowStats()
        self._ck(self.L.nalo_tsdf_follow(self.h_, _d(ce), _i(mg), C.c_float(min_weight), _i(shift), C.byref(st)))
        return dict(shift=shift, n_boxes=int(st.n_boxes), added_vertices=int(st.added_vertices), welded_vertices=int(st.welded_vertices),
                    added_triangles=int(st.added_triangles), n_vertices=int(st.n_vertices), n_triangles=int(st.n_triangles))

    def map_dense_cloud(self, frame_id, draws=None, cap=None, n_draws=None):
        """refreshPC() for one frame's dense points -> dict(xyz [n][3] float32, rgb [n][3] uint8, records, survivors, n_needed); cap / n_draws override the sizes
        the call is made with (the refusals); self.dense_cloud_needed holds n_needed after a refusal too"""
        a = MapDenseCloudArgs()
        a.frame_id = int(frame_id)
        rc = self.L.nalo_map_dense_cloud(self.h_, C.byref(a))                    # cap = 0: answers n_needed (and is the whole call for a frame without records)
        self.dense_cloud_needed = a.n_needed
        if a.n_needed == 0:
            self._ck(rc)
        need = a.n_needed
        xyz, rgb = np.zeros((need, 3), np.float32), np.zeros((need, 3), np.uint8)
        if need:
            d = None if draws is None else np.ascontiguousarray(draws, np.int32)
            a.cap, a.xyz, a.rgb = need if cap is None else int(cap), _f(xyz), _u8(rgb)
            a.draws, a.n_draws = (None, 0) if d is None else (_i(d), len(d) if n_draws is None else int(n_draws))
            rc = self.L.nalo_map_dense_cloud(self.h_, C.byref(a))
            self.dense_cloud_needed = a.n_needed
            self._ck(rc)
        return dict(xyz=xyz[:a.n], rgb=rgb[:a.n], records=int(a.records), survivors=int(a.survivors), n_needed=need)

    def ba_get_frames(self):
        arr = (FrameState * self.W)()
        w2c = np.zeros((self.W, 12))
        cal = np.zeros(4)
        self._ck(self.L.nalo_ba_get_frames(self.h_, arr, _d(w2c), _d(cal)))
        return arr, w2c.reshape(self.W, 3, 4), cal

    def ba_get_points(self):
        P = self.P
        o = {k: np.zeros(P, np.float32) for k in ("idepth", "step", "HdiF", "bdSumF", "Hdd", "bd")}
        o["Hcd"] = np.zeros((P, 4), np.float32)
        o["maxRelBaseline"] = np.zeros(P, np.float32)
        self._ck(self.L.nalo_ba_get_points(self.h_, _f(o["idepth"]), _f(o["step"]), _f(o["HdiF"]), _f(o["bdSumF"]), _f(o["Hdd"]),
                                           _f(o["bd"]), _f(o["Hcd"]), _f(o["maxRelBaseline"])))
        return o

    def ba_get_residuals(self):
        n = self.P * self.W
        st, ac = np.zeros(n, np.int8), np.zeros(n, np.uint8)
        jp, en, cp = np.zeros((n, 8), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        self._ck(self.L.nalo_ba_get_residuals(self.h_, st.ctypes.data_as(c_i8p), _u8(ac), _f(jp), _f(en), _f(cp)))
        s = (self.P, self.W)
        return st.reshape(s), ac.reshape(s), jp.reshape(s + (8,)), en.reshape(s), cp.reshape(s + (3,))

    def ba_pattern_projections(self):
        """PointFrameResidual::projectedTo and state_energy of every slot (nalo_ba_get_pattern_projections) -> (projected [P, W, 8, 2], state_energy [P, W]);
        a slot that does not exist or is OOB holds 2.0 / 0"""
        n = self.P * self.W
        pr, en = np.zeros((max(n, 1), 8, 2), np.float32), np.zeros(max(n, 1), np.float32)
        self._ck(self.L.nalo_ba_get_pattern_projections(self.h_, _f(pr), _f(en)))
        return pr[:n].reshape(self.P, self.W, 8, 2), en[:n].reshape(self.P, self.W)

    def ba_residual_plot(self, host, free_debug_param5=0.0, frame_mask=0, rainbow_scale=1.0):
        """one outer iteration of FullSystem::debugPlotTracking on the device (nalo_ba_residual_plot). Returns a dict: bgr (n_frames, h, w, 3) uint8, frame_id
        [n_frames], aff [n_frames, 2] float64, n_points, n_residuals, n_pattern_pixels"""
        a = ResidualPlotArgs()
        nf = bin(frame_mask).count("1") if frame_mask else max(self.W, 1)
        bgr = np.zeros((max(nf, 1), self.h, self.w, 3), np.uint8)
        a.host, a.free_debug_param5, a.rainbow_scale, a.frame_mask, a.bgr = int(host), float(free_debug_param5), float(rainbow_scale), int(frame_mask), _u8(bgr)
        self._ck(self.L.nalo_ba_residual_plot(self.h_, C.byref(a)))
        n = a.n_frames
        return {"bgr": bgr[:n], "frame_id": [a.frame_id[j] for j in range(n)], "aff": np.array([[a.aff[j][0], a.aff[j][1]] for j in range(n)], np.float64).reshape(n, 2),
                "n_points": a.n_points, "n_residuals": a.n_residuals, "n_pattern_pixels": a.n_pattern_pixels}

    def ba_get_acc13(self):
        a = np.zeros(self.W * self.W * 169)
        self._ck(self.L.nalo_ba_get_acc13(self.h_, _d(a)))
        return a.reshape(self.W * self.W, 13, 13)

    def ba_counts(self):
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.nalo_ba_counts(self.h_, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ba_launch_config(self):
        """the kernel variants the window setup chose (nalo_ba_get_launch_config)"""
        a = (C.c_int * 10)()
        self._ck(self.L.nalo_ba_get_launch_config(self.h_, a))
        keys = ("nblocks", "Ppad", "lin_sub", "sc_split", "sc_bpw", "T", "pull", "radix", "resub_mode", "prelaunch_eligible")
        return dict(zip(keys, list(a)))

    # ---- two-frame initialiser
    def init_calc_res_and_gs(self, slot_first, slot_new, lvl, refToNew, aff, pts, alphaW=150.0 * 150.0, alphaK=2.5 * 2.5, couplingWeight=1.0):
        f = lambda a: np.ascontiguousarray(a, np.float32)
        n = len(pts["u"])
        ig = np.ascontiguousarray(pts["isGood"], np.uint8)
        ign, en, ms = np.zeros(n, np.uint8), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        lh, jb = f(pts["lastHessian_new"]).copy(), f(pts["Jb"]).copy()
        H, b, Hs, bs, E3 = np.zeros(64), np.zeros(8), np.zeros(64), np.zeros(8), np.zeros(3)
        a = [f(pts[k]) for k in ("u", "v", "idepth_new", "iR")]
        eng, oth = f(pts["energy"]), f(pts["outlierTH"])
        T = np.ascontiguousarray(refToNew, np.float64).reshape(-1)
        af = np.ascontiguousarray(aff, np.float64)
        self._ck(self.L.nalo_init_calc_res_and_gs(self.h_, slot_first, slot_new, lvl, n, *[_f(x) for x in a], _u8(ig), _f(eng), _f(oth), _d(T), _d(af),
                                                  alphaW, alphaK, couplingWeight, _u8(ign), _f(en), _f(ms), _f(lh), _f(jb), _d(H), _d(b), _d(Hs), _d(bs), _d(E3)))
        return dict(H=H.reshape(8, 8), b=b, Hsc=Hs.reshape(8, 8), bsc=bs, E3=E3, isGood_new=ign, energy_new=en, maxstep=ms, lastHessian_new=lh, Jb=jb)

    def init_do_step(self, isGood, Jb, maxstep, idepth, lam, inc, idepth_new):
        f = lambda a: np.ascontiguousarray(a, np.float32)
        out = f(idepth_new).copy()
        self._ck(self.L.nalo_init_do_step(self.h_, len(out), _u8(np.ascontiguousarray(isGood, np.uint8)), _f(f(Jb)), _f(f(maxstep)), _f(f(idepth)), float(lam), _f(f(inc)), _f(out)))
        return out

    def dense_make_map(self, slot, plane, mask_value, camToWorld, cap=100000):
        """DenseMapping::updateMap bbox scan + makeMap -> dict(n, accept, rect, u, v, idepth, color, bgr)"""
        rect = np.zeros(4, np.int32)
        u, v = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        idp, col, bgr = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros((cap, 3), np.uint8)
        n, acc = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.L.nalo_dense_make_map(self.h_, slot, _f(np.ascontiguousarray(plane, np.float32)), C.c_float(mask_value), _d(np.ascontiguousarray(camToWorld, np.float64).reshape(-1)),
                                            cap, _i(rect), _i(u), _i(v), _f(idp), _f(col), _u8(bgr), _i(n), _i(acc)))
        k = min(int(n[0]), cap)
        return dict(n=int(n[0]), accept=int(acc[0]), rect=rect, u=u[:k], v=v[:k], idepth=idp[:k], color=col[:k], bgr=bgr[:k])

    def _fit_planes(self, call, draws, threshold, min_points, append, cap):
        """-> (records as a PLANE_DTYPE array, n_clusters); draws=None passes a NULL stream, a cap below the need raises NaloError with .n_clusters set"""
        d = None if draws is None else np.ascontiguousarray(draws, np.uint32)
        n_samples = self._plane_n_samples if d is None else len(d) // 3
        a = PlaneFitArgs(float(threshold), int(min_points), int(n_samples), None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint32)), int(append))
        out = np.zeros(max(cap, 1), PLANE_DTYPE)
        n = np.zeros(1, np.int32)
        rc = call(C.byref(a), cap, out.ctypes.data_as(C.c_void_p) if cap > 0 else None, _i(n))
        self.plane_n_clusters = int(n[0])
        self._ck(rc)
        return out[:int(n[0])].copy(), int(n[0])

    _plane_n_samples = 50

    def trk_fit_planes(self, draws, threshold=0.01, min_points=10, append=0, cap=2048):
        """makeMaskDistMap + fitPlane on the level-0 cloud (nalo_trk_fit_planes) -> (records, n_clusters); self.plane_n_clusters holds the count after a refusal too"""
        return self._fit_planes(lambda a, cap_, o, n: self.L.nalo_trk_fit_planes(self.h_, a, cap_, o, n), draws, threshold, min_points, append, cap)

    def trk_fit_ground(self, draws, threshold=0.01, min_points=20, append=0, cap=2048, mark=False, n_points=0, pick=None, want_scores=True):
        """nalo_trk_fit_planes + the ground choice of setCoarseTrackingRef (nalo_trk_fit_ground) -> (records, n_clusters, pick, scores, onground).
        min_points defaults to CoarseTracker::fitPlane's 20. mark: also mark the window's points (n_points = P of nalo_ba_set_points; onground is then a uint8
        array in submission order, else None). pick: a GroundPick to write into (a fresh zeroed one otherwise); scores: a GROUND_SCORE_DTYPE array of
        n_clusters entries (all zero when pick.ran == 0)."""
        pick = GroundPick() if pick is None else pick
        sc = np.zeros(max(cap, 1), GROUND_SCORE_DTYPE) if want_scores else None
        on = np.zeros(max(int(n_points), 1), np.uint8) if mark else None
        g = GroundArgs(int(bool(mark)), _u8(on), int(n_points) if mark else 0, None if sc is None else sc.ctypes.data_as(C.c_void_p))
        rec, n = self._fit_planes(lambda a, cap_, o, n_: self.L.nalo_trk_fit_ground(self.h_, a, C.byref(g), cap_, o, n_, C.byref(pick)), draws, threshold, min_points, append, cap)
        return rec, n, pick, (None if sc is None else sc[:n].copy()), (None if on is None else on[:int(n_points)])

    def dense_fit_planes(self, host_frame, draws, threshold=0.01, min_points=10, cap=2048):
        """the same on the window points and resident immature points of one host frame (nalo_dense_fit_planes)"""
        return self._fit_planes(lambda a, cap_, o, n: self.L.nalo_dense_fit_planes(self.h_, int(host_frame), a, cap_, o, n), draws, threshold, min_points, 0, cap)

    def plane_fit_members(self, n_input, n_members):
        """the last call's member lists (nalo_plane_fit_members) -> (cluster_of[n_input], order[n_members])"""
        cl, order = np.full(max(n_input, 1), -1, np.int32), np.zeros(max(n_input, 1), np.int32)     # the members are at most the input
        self._ck(self.L.nalo_plane_fit_members(self.h_, int(n_input), _i(cl), _i(order)))
        return cl[:n_input], order[:n_members]

    def trk_append_plane_points(self, dirv, dis, ref_color, rect):
        n = np.zeros(1, np.int32)
        self._ck(self.L.nalo_trk_append_plane_points(self.h_, _f(np.ascontiguousarray(dirv, np.float32)), C.c_float(dis), int(ref_color), _i(np.ascontiguousarray(rect, np.int32)), _i(n)))
        return int(n[0])

    def undist_set(self, wOrg, hOrg, G=None, vinv=None, photometric=0, remapX=None, remapY=None):
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        G, vinv, remapX, remapY = f(G), f(vinv), f(remapX), f(remapY)
        self._ck(self.L.nalo_undist_set(self.h_, wOrg, hOrg, None if G is None else _f(G), 0 if G is None else G.size, None if vinv is None else _f(vinv), int(photometric),
                                        None if remapX is None else _f(remapX), None if remapY is None else _f(remapY)))
        self._und_size = int(wOrg) * int(hOrg)

    def frame_upload_raw(self, slot, raw, exposure=1.0, factor=1.0, mask_org=None, bgr_org=None, gammaB=None):
        raw = np.ascontiguousarray(raw)
        assert raw.dtype in (np.uint8, np.uint16)
        m = None if mask_org is None else np.ascontiguousarray(mask_org, np.uint8)
        b = None if bgr_org is None else np.ascontiguousarray(bgr_org, np.uint8)
        g = None if gammaB is None else np.ascontiguousarray(gammaB, np.float32)
        self._ck(self.L.nalo_frame_upload_raw(self.h_, slot, raw.ctypes.data_as(C.c_void_p), raw.dtype.itemsize, C.c_float(exposure), C.c_float(factor),
                                              None if m is None else _u8(m), None if b is None else _u8(b), None if g is None else _f(g)))

    def frame_upload_raw_async(self, slot, raw, exposure=1.0, factor=1.0, gammaB=None):
        """raw: a contiguous uint8 / uint16 array that stays alive and untouched until frame_wait(slot) (pinned: pinned_array(..., dtype))"""
        assert raw.flags.c_contiguous and raw.dtype in (np.uint8, np.uint16)
        assert gammaB is None or (gammaB.dtype == np.float32 and gammaB.flags.c_contiguous and gammaB.size == 256)
        self._ck(self.L.nalo_frame_upload_raw_async(self.h_, slot, raw.ctypes.data_as(C.c_void_p), raw.dtype.itemsize, C.c_float(exposure), C.c_float(factor), _f(gammaB)))

    def get_settings(self):
        st = Settings()
        self._ck(self.L.nalo_get_settings(self.h_, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Settings._fields_}

    def set_settings(self, force_accept_step=None, affine_opt_mode_a=None, affine_opt_mode_b=None, min_opt_iterations=None):
        st = Settings()
        self._ck(self.L.nalo_get_settings(self.h_, C.byref(st)))
        if force_accept_step is not None: st.forceAcceptStep = int(force_accept_step)
        if affine_opt_mode_a is not None: st.affineOptModeA = float(affine_opt_mode_a)
        if affine_opt_mode_b is not None: st.affineOptModeB = float(affine_opt_mode_b)
        if min_opt_iterations is not None: st.minOptIterations = int(min_opt_iterations)
        self._ck(self.L.nalo_set_settings(self.h_, C.byref(st)))
        return st

    def ba_plane_scale_fix(self, localscale, camToTrackingRef, trackingRef_camToWorld):
        a = np.ascontiguousarray(camToTrackingRef, np.float64).reshape(-1); b = np.ascontiguousarray(trackingRef_camToWorld, np.float64).reshape(-1)
        self._ck(self.L.nalo_ba_plane_scale_fix(self.h_, float(localscale), _d(a), _d(b)))

    def ba_sw_gray_optimize(self):
        cost, n = np.zeros(1), np.zeros(1, np.int32)
        self._ck(self.L.nalo_ba_sw_gray_optimize(self.h_, _d(cost), _i(n)))
        return float(cost[0]), int(n[0])

    def ba_get_idepth_zero(self, P):
        o = np.zeros(P, np.float32)
        self._ck(self.L.nalo_ba_get_idepth_zero(self.h_, _f(o)))
        return o

    def ba_calc_l_energy(self):
        e = np.zeros(1)
        self._ck(self.L.nalo_ba_calc_l_energy(self.h_, _d(e)))
        return float(e[0])

    def ba_calc_m_energy(self):
        e = np.zeros(1)
        self._ck(self.L.nalo_ba_calc_m_energy(self.h_, _d(e)))
        return float(e[0])

    def ba_optimize_stats(self):
        a = np.zeros(2, np.int32)
        self._ck(self.L.nalo_ba_optimize_stats(self.h_, a[0:1].ctypes.data_as(C.POINTER(C.c_int)), a[1:2].ctypes.data_as(C.POINTER(C.c_int))))
        return int(a[0]), int(a[1])

    def init_set_first(self, slot_first, sparsityFactor=5):
        """CoarseInitializer::setFirst -> (points per level, the updated global sparsityFactor)"""
        sf, num = np.array([sparsityFactor], np.int32), np.zeros(6, np.int32)
        self._ck(self.L.nalo_init_set_first(self.h_, slot_first, _i(sf), _i(num)))
        return num[:self.levels].copy(), int(sf[0])

    def init_track_frame(self, slot_new, exposure_first=1.0, exposure_new=1.0):
        ok = np.zeros(1, np.int32)
        self._ck(self.L.nalo_init_track_frame(self.h_, slot_new, C.c_float(exposure_first), C.c_float(exposure_new), _i(ok)))
        return bool(ok[0])

    def init_state(self):
        T, aff, st = np.zeros(12), np.zeros(2), np.zeros(4, np.int32)
        p = lambda k: st[k:k + 1].ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.L.nalo_init_get_state(self.h_, _d(T), _d(aff), p(0), p(1), p(2), p(3)))
        return dict(thisToNext=T.reshape(3, 4), aff=aff, snapped=bool(st[0]), frameID=int(st[1]), snappedAt=int(st[2]), n_evals=int(st[3]))

    def init_set_carried(self, car):
        """car = orc.Initializer.carried(): the pose / affine / snap state and, per level, orc.Initializer.CARRIED"""
        s = car["state"]
        self._ck(self.L.nalo_init_set_state(self.h_, _d(np.ascontiguousarray(s["thisToNext"], np.float64).reshape(-1)), _d(np.ascontiguousarray(s["aff"], np.float64)),
                                            int(s["snapped"]), int(s["frameID"]), int(s["snappedAt"])))
        for l, p in enumerate(car["points"]):
            a = {k: np.ascontiguousarray(p[k], np.uint8 if k.startswith("isGood") else np.float32) for k in p}
            self._ck(self.L.nalo_init_set_points(self.h_, l, len(a["idepth"]), _f(a["idepth"]), _f(a["idepth_new"]), _f(a["iR"]), _u8(a["isGood"]), _f(a["lastHessian"]),
                                                 _f(a["energy"]), _f(a["maxstep"]), _f(a["lastHessian_new"]), _f(a["energy_new"]), _u8(a["isGood_new"]), _f(a["iRSumNum"])))

    SWEEPS = dict(opt_reg=0, propagate_up=1, propagate_down=2, reset_points=3)

    def init_sweep(self, which, lvl):
        """one of trackFrame's sweeps alone: optReg(lvl), propagateUp(srcLvl), propagateDown(srcLvl), resetPoints(lvl)"""
        self._ck(self.L.nalo_init_sweep(self.h_, self.SWEEPS[which], lvl))

    def init_carried(self, lvl):
        """the Pnt members nalo_init_set_points writes and init_points() does not return"""
        n = len(self.init_points(lvl)["u"]); m = max(n, 1)
        o = dict(idepth_new=np.zeros(m, np.float32), maxstep=np.zeros(m, np.float32), lastHessian_new=np.zeros(m, np.float32), energy_new=np.zeros((m, 2), np.float32),
                 isGood_new=np.zeros(m, np.uint8))
        self._ck(self.L.nalo_init_get_carried(self.h_, lvl, n, _f(o["idepth_new"]), _f(o["maxstep"]), _f(o["lastHessian_new"]), _f(o["energy_new"]), _u8(o["isGood_new"])))
        return {k: v[:n] for k, v in o.items()}

    def init_points(self, lvl):
        n = np.zeros(1, np.int32)
        self._ck(self.L.nalo_init_get_points(self.h_, lvl, 0, _i(n), *([None] * 13)))
        n = int(n[0]); m = max(n, 1)
        f = lambda k=1: np.zeros((m, k) if k > 1 else m, np.float32)
        o = dict(u=f(), v=f(), idepth=f(), iR=f(), isGood=np.zeros(m, np.uint8), lastHessian=f(), energy=f(2), my_type=f(), outlierTH=f(), parent=np.zeros(m, np.int32),
                 parentDist=f(), neighbours=np.zeros((m, 10), np.int32), neighboursDist=f(10))
        nn = np.zeros(1, np.int32)
        self._ck(self.L.nalo_init_get_points(self.h_, lvl, n, _i(nn), _f(o["u"]), _f(o["v"]), _f(o["idepth"]), _f(o["iR"]), _u8(o["isGood"]), _f(o["lastHessian"]), _f(o["energy"]),
                                             _f(o["my_type"]), _f(o["outlierTH"]), _i(o["parent"]), _f(o["parentDist"]), _i(o["neighbours"]), _f(o["neighboursDist"])))
        return {k: a[:n] for k, a in o.items()}

    def init_depth_image(self, lvl=0, rainbow_scale=1.0):
        """CoarseInitializer::debugPlot on the device (nalo_init_depth_image). Returns a dict: bgr (h, w, 3) uint8 of the level, n_points, n_good, sum_iR and fac
        (float32)"""
        a = InitPlotArgs()
        bgr = np.zeros(3 * self.w * self.h, np.uint8)
        a.lvl, a.rainbow_scale, a.bgr = int(lvl), float(rainbow_scale), _u8(bgr)
        self._ck(self.L.nalo_init_depth_image(self.h_, C.byref(a)))
        return {"bgr": bgr[:3 * a.w * a.h].reshape(a.h, a.w, 3), "n_points": a.n_points, "n_good": a.n_good, "sum_iR": np.float32(a.sum_iR), "fac": np.float32(a.fac)}

    def pixsel_make_hists(self, slot, readback=True):
        """-> (ths, thsSmoothed); readback=False passes NULL for both (the thresholds stay on the device, the last map's list stays readable) -> None"""
        if not readback:
            self._ck(self.L.nalo_pixsel_make_hists(self.h_, slot, None, None))
            return None
        nb = (self.w // 32) * (self.h // 32)
        ths, sm = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
        self._ck(self.L.nalo_pixsel_make_hists(self.h_, slot, _f(ths), _f(sm)))
        return ths, sm

    def pixsel_set_random(self, randomPattern, mask_draws=None):
        rp = np.ascontiguousarray(randomPattern, np.uint8)
        assert rp.size == self.w * self.h
        dr = None if mask_draws is None else np.ascontiguousarray(mask_draws, np.int32)
        self._ck(self.L.nalo_pixsel_set_random(self.h_, _u8(rp), None if dr is None else _i(dr)))

    def pixsel_select(self, slot, pot, thFactor=1.0):
        m, n = np.zeros((self.h, self.w), np.float32), np.zeros(3, np.int32)
        self._ck(self.L.nalo_pixsel_select(self.h_, slot, pot, float(thFactor), _f(m), _i(n)))
        return m, n

    def pixsel_make_maps(self, slot, density, potential, recursionsLeft=1, thFactor=1.0):
        """-> (map [h,w], numHaveSub, new currentPotential)"""
        m, pot, num = np.zeros((self.h, self.w), np.float32), np.array([potential], np.int32), np.zeros(1, np.int32)
        self._ck(self.L.nalo_pixsel_make_maps(self.h_, slot, float(density), recursionsLeft, float(thFactor), _i(pot), _f(m), _i(num)))
        return m, int(num[0]), int(pot[0])

    def pixsel_make_maps_lidar(self, slot, potential, thFactor=1.0):
        m, num = np.zeros((self.h, self.w), np.float32), np.zeros(1, np.int32)
        self._ck(self.L.nalo_pixsel_make_maps_lidar(self.h_, slot, float(thFactor), potential, _f(m), _i(num)))
        return m, int(num[0])

    def pixsel_get_selected(self):
        n = np.zeros(1, np.int32)
        self._ck(self.L.nalo_pixsel_get_selected(self.h_, 0, None, None, _i(n)))
        idx, st = np.zeros(max(int(n[0]), 1), np.int32), np.zeros(max(int(n[0]), 1), np.uint8)
        self._ck(self.L.nalo_pixsel_get_selected(self.h_, int(n[0]), _i(idx), _u8(st), _i(n)))
        return idx[:n[0]], st[:n[0]]

    def dist_make_map(self, frame, KRKi, Kt):
        out = np.zeros((self.h >> 1, self.w >> 1), np.float32)
        self._ck(self.L.nalo_dist_make_map(self.h_, frame, _f(np.ascontiguousarray(KRKi, np.float32)), _f(np.ascontiguousarray(Kt, np.float32)), _f(out)))
        return out

    # ---- immature points
    def imm_create(self, slot_host, u, v):
        n = len(u)
        ui, vi = np.ascontiguousarray(u, np.int32), np.ascontiguousarray(v, np.int32)
        color, weights, gradH, eth = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        self._ck(self.L.nalo_imm_create(self.h_, slot_host, n, _i(ui), _i(vi), _f(color), _f(weights), _f(gradH), _f(eth)))
        return color, weights, gradH, eth

    def imm_trace(self, slot_new, u, v, color, weights, gradH, energyTH, host_idx, KRKi, Kt, aff, idmin, idmax, status, quality):
        n = len(u)
        f = lambda a: np.ascontiguousarray(a, np.float32).copy()
        idmin, idmax, quality = f(idmin), f(idmax), f(quality)
        status = np.ascontiguousarray(status, np.int32).copy()
        uv, li = np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        hi = np.ascontiguousarray(host_idx, np.int32)
        a = [f(x) for x in (u, v, color, weights, gradH, energyTH)]
        k = [f(x) for x in (KRKi, Kt, aff)]
        self._ck(self.L.nalo_imm_trace(self.h_, slot_new, n, *[_f(x) for x in a], _i(hi), len(k[0].reshape(-1, 9)), *[_f(x) for x in k],
                                       _f(idmin), _f(idmax), _i(status), _f(quality), _f(uv), _f(li)))
        return idmin, idmax, status, quality, uv, li

    def imm_resident_set(self, u, v, color, weights, gradH, energyTH, host_idx, idmin, idmax, status, quality):
        f = lambda a: np.ascontiguousarray(a, np.float32)
        a = [f(x) for x in (u, v, color, weights, gradH, energyTH)]
        self._imm_n = len(a[0])
        self._ck(self.L.nalo_imm_resident_set(self.h_, self._imm_n, *[_f(x) for x in a], _i(np.ascontiguousarray(host_idx, np.int32)), _f(f(idmin)), _f(f(idmax)),
                                              _i(np.ascontiguousarray(status, np.int32)), _f(f(quality))))

    def imm_resident_trace(self, slot_new, KRKi, Kt, aff):
        k = [np.ascontiguousarray(x, np.float32) for x in (KRKi, Kt, aff)]
        self._ck(self.L.nalo_imm_resident_trace(self.h_, slot_new, len(k[0].reshape(-1, 9)), *[_f(x) for x in k]))

    def imm_resident_get(self):
        n = self._imm_n
        idmin, idmax, quality, li = [np.zeros(n, np.float32) for _ in range(4)]
        status, uv = np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
        self._ck(self.L.nalo_imm_resident_get(self.h_, _f(idmin), _f(idmax), _i(status), _f(quality), _f(uv), _f(li)))
        return idmin, idmax, status, quality, uv, li

    def imm_optimize(self, host, u, v, color, weights, energyTH, idmin, idmax, min_obs):
        n = len(u)
        f = lambda a: np.ascontiguousarray(a, np.float32)
        a = [f(x) for x in (u, v, color, weights, energyTH, idmin, idmax)]
        hi = np.ascontiguousarray(host, np.int32)
        res, idp, rin = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, self.W), np.uint8)
        self._ck(self.L.nalo_imm_optimize(self.h_, n, _i(hi), *[_f(x) for x in a], int(min_obs), _i(res), _f(idp), _u8(rin)))
        return res, idp, rin

    def imm_resident_optimize(self, sel, min_obs, n_all=None):
        """optimizeImmaturePoint for points of the device-resident set: sel = their indices (None: all n_all of them)"""
        if sel is None:
            n, sp = int(n_all), None
        else:
            si = np.ascontiguousarray(sel, np.int32); n, sp = len(si), _i(si)
        res, idp, rin = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, self.W), np.uint8)
        self._ck(self.L.nalo_imm_resident_optimize(self.h_, n, sp, int(min_obs), _i(res), _f(idp), _u8(rin)))
        return res, idp, rin

    def imm_resident_set_type(self, my_type):
        """ImmaturePoint::my_type of every resident point, once after imm_resident_set"""
        t = np.ascontiguousarray(my_type, np.float32)
        if len(t) != self._imm_n:
            raise ValueError("my_type needs one entry per resident point")
        self._ck(self.L.nalo_imm_resident_set_type(self.h_, _f(t)))

    def imm_resident_activate(self, frame, KRKi, Kt, host_flagged, min_act_dist, min_obs=None):
        """activatePointsMT's distance map + selection loop (+ optimizeImmaturePoint of the selected points when min_obs is given) for the resident set:
        fate [n], sel [n_sel] and, with min_obs, (result, idepth, res_in) rows for sel; see nalo_imm_resident_activate"""
        n = self._imm_n
        fate, sel, nsel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32)
        fl = np.ascontiguousarray(host_flagged, np.int32)
        k = [np.ascontiguousarray(x, np.float32) for x in (KRKi, Kt)]
        if min_obs is None:
            self._ck(self.L.nalo_imm_resident_activate(self.h_, int(frame), _f(k[0]), _f(k[1]), _i(fl), float(min_act_dist), 0, _i(fate), _i(nsel), _i(sel), None, None, None))
            return fate, sel[:nsel[0]].copy()
        res, idp, rin = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, self.W), np.uint8)
        self._ck(self.L.nalo_imm_resident_activate(self.h_, int(frame), _f(k[0]), _f(k[1]), _i(fl), float(min_act_dist), int(min_obs), _i(fate), _i(nsel), _i(sel),
                                                    _i(res), _f(idp), _u8(rin)))
        m = int(nsel[0])
        return fate, sel[:m].copy(), (res[:m].copy(), idp[:m].copy(), rin[:m].copy())

    def imm_activate_last(self):
        """(survivors of the test on the initial map, selected, rejected because of an earlier selected point, rounds) of the last imm_resident_activate"""
        st = np.zeros(4, np.int32)
        self._ck(self.L.nalo_imm_activate_last(self.h_, _i(st)))
        return tuple(int(x) for x in st)

    def imm_resident_carry(self, fate=None, sel=None, result=None, host_map=None, append_slot=-1, append_host=0, append_idx=None, append_status=None):
        """the resident set across a keyframe on the device (nalo_imm_resident_carry): (A) fate / sel / result of imm_resident_activate, (C) host_map[h_old] = h_new
        or -1, (B) append_slot / append_host with an explicit list or, with append_idx None, the selector's last map. -> the counts of imm_resident_carry_last"""
        a = ImmCarryArgs()
        a.append_slot, a.append_host = int(append_slot), int(append_host)
        keep = []

        def ints(x):
            keep.append(np.ascontiguousarray(x, np.int32))
            return _i(keep[-1])
        if fate is not None:
            a.fate = ints(fate)
            a.n_sel = 0 if sel is None else len(sel)
            if sel is not None:
                a.sel = ints(sel)
            if result is not None:
                a.result = ints(result)
        if host_map is not None:
            a.host_map, a.n_hosts_old = ints(host_map), len(host_map)
        if append_idx is not None:
            a.append_idx, a.append_n = ints(append_idx), len(append_idx)
            keep.append(np.ascontiguousarray(append_status, np.uint8))
            a.append_status = _u8(keep[-1])
        self._ck(self.L.nalo_imm_resident_carry(self.h_, C.byref(a)))
        st = self.imm_resident_carry_last()
        self._imm_n = st[0]
        return st

    def imm_resident_carry_last(self):
        """(n_new, deleted by (A), dropped with their host by (C), appended, points per new host [16])"""
        st = np.zeros(4 + 16, np.int32)
        self._ck(self.L.nalo_imm_resident_carry_last(self.h_, _i(st)))
        return int(st[0]), int(st[1]), int(st[2]), int(st[3]), st[4:].copy()

    def imm_resident_carry_map(self):
        src = np.zeros(max(self._imm_n, 1), np.int32)
        self._ck(self.L.nalo_imm_resident_carry_map(self.h_, _i(src)))
        return src[:self._imm_n]

    def imm_resident_get_points(self, with_type=True):
        """dict(u, v, color [n,8], weights [n,8], gradH [n,3], energyTH, host_idx, my_type) of the resident set"""
        n = np.zeros(1, np.int32)
        self._ck(self.L.nalo_imm_resident_get_points(self.h_, _i(n), None, None, None, None, None, None, None, None))
        n = int(n[0])
        m = max(n, 1)
        o = dict(u=np.zeros(m, np.float32), v=np.zeros(m, np.float32), color=np.zeros((m, 8), np.float32), weights=np.zeros((m, 8), np.float32),
                 gradH=np.zeros((m, 3), np.float32), energyTH=np.zeros(m, np.float32), host_idx=np.zeros(m, np.int32), my_type=np.zeros(m, np.float32))
        self._ck(self.L.nalo_imm_resident_get_points(self.h_, None, _f(o["u"]), _f(o["v"]), _f(o["color"]), _f(o["weights"]), _f(o["gradH"]), _f(o["energyTH"]),
                                                     _i(o["host_idx"]), _f(o["my_type"]) if with_type else None))
        return {k: a[:n] for k, a in o.items()}

    def ba_snapshot(self):
        self._ck(self.L.nalo_ba_snapshot(self.h_))

    def ba_restore(self):
        self._ck(self.L.nalo_ba_restore(self.h_))

    @property
    def stream(self):
        """hipStream_t (as int) every kernel of this context is launched on"""
        return int(self.L.nalo_stream(self.h_) or 0)

    @property
    def side_stream(self):
        """hipStream_t (as int) of the context's second stream (the threshold's histogram sums of a sharded window run there)"""
        return int(self.L.nalo_side_stream(self.h_) or 0)

    def ba_set_allreduce(self, fn, stream_ordered=False, fn_side=None):
        """fn(device_ptr:int, n:int) sums n doubles in place across ranks. stream_ordered: fn enqueues on self.stream and does not wait;
        fn_side (optional, stream-ordered only) does the same on self.side_stream."""
        self._ck(self.L.nalo_ba_set_allreduce_mode(self.h_, int(bool(stream_ordered) and fn is not None)))
        if fn is None:
            self._hook = self._hook_side = None
            self._ck(self.L.nalo_ba_set_allreduce(self.h_, C.cast(None, ALLREDUCE_FN), None))
            self._ck(self.L.nalo_ba_set_allreduce_side(self.h_, C.cast(None, ALLREDUCE_FN), None))
            return
        self._hook = ALLREDUCE_FN(lambda user, ptr, n: fn(ptr, n))
        self._ck(self.L.nalo_ba_set_allreduce(self.h_, self._hook, None))
        if fn_side is not None and stream_ordered:
            self._hook_side = ALLREDUCE_FN(lambda user, ptr, n: fn_side(ptr, n))
            self._ck(self.L.nalo_ba_set_allreduce_side(self.h_, self._hook_side, None))
        else:
            self._hook_side = None
            self._ck(self.L.nalo_ba_set_allreduce_side(self.h_, C.cast(None, ALLREDUCE_FN), None))

    def ba_exchange_failed(self, what="test"):
        """what a caller's all-reduce hook calls when its collective failed (the hook has no return value)"""
        self.L.nalo_ba_exchange_failed.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self.L.nalo_ba_exchange_failed(self.h_, what.encode()))

    def ba_rccl_ranks(self):
        """(ranks of the main communicator, ranks of the side communicator) as RCCL reports them (ncclCommCount); 0 = none installed"""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self.L.nalo_ba_rccl_ranks(self.h_, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ba_rccl_init(self, nranks, rank, id_main, id_side=None):
        """native RCCL exchange (ncclCommInitRank on this context's device, collective over the ranks); ids from rccl_unique_id()"""
        self._ck(self.L.nalo_ba_rccl_init(self.h_, int(nranks), int(rank), id_main, id_side))

    # ---- profiling
    def hbm_calibrate(self, nbytes=1 << 30, iters=10):
        """measured streaming bandwidth of this device (GB/s): (copy, triad) - the roofline's denominator next to the nominal 8 TB/s"""
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self.L.nalo_hbm_calibrate(self.h_, C.c_size_t(nbytes), iters, C.byref(a), C.byref(b)))
        return a.value, b.value

    def profile_enable(self, on=True):
        self._ck(self.L.nalo_profile_enable(self.h_, int(on)))

    def profile_select(self, name=None):
        """bracket only the scope `name` (None = all scopes)"""
        self._ck(self.L.nalo_profile_select(self.h_, None if name is None else name.encode()))

    def profile_sample(self, every=1):
        self._ck(self.L.nalo_profile_sample(self.h_, int(every)))

    def profile_reset(self):
        self._ck(self.L.nalo_profile_reset(self.h_))

    def profile_get(self, name):
        ms, n = C.c_double(0), C.c_int(0)
        self._ck(self.L.nalo_profile_get(self.h_, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_samples(self, name):
        """every bracketed launch of the scope since the last reset, in launch order (microseconds)"""
        n = C.c_int(0)
        self._ck(self.L.nalo_profile_samples(self.h_, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._ck(self.L.nalo_profile_samples(self.h_, name.encode(), _f(out), n.value, C.byref(n)))
        return out[:n.value].astype(np.float64) * 1e3
