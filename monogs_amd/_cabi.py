"""ctypes binding of the C ABI in include/monogs_raster.h.

The shared library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950) at
monogs_amd/lib/libmonogs_raster.so.  There is NO fallback: if the library is missing
or an entry point is absent, importing `lib()` raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MGS_LIB_PATH: load another build of the SAME library (kernel experiments, the -DMGS_STAMP build)
LIB_PATH = os.environ.get("MGS_LIB_PATH") or os.path.join(_HERE, "lib", "libmonogs_raster.so")

ABI_VERSION = 10

EXPORTS = (
    "mgs_abi_version", "mgs_struct_size", "mgs_status_string", "mgs_raster_workspace_query",
    "mgs_raster_forward_project", "mgs_raster_forward_blend", "mgs_raster_backward",
    "mgs_knn_scratch_bytes", "mgs_knn_dist2", "mgs_profile_enable", "mgs_profile_read",
    "mgs_pose_adam_step", "mgs_tracking_loss_partial_count", "mgs_tracking_loss_forward",
    "mgs_tracking_loss_backward", "mgs_tracking_loss_onepass", "mgs_lm_solve_step", "mgs_mapping_loss_forward",
    "mgs_mapping_loss_backward", "mgs_camera_from_pose", "mgs_tracking_iteration",
    "mgs_adam_step_multi", "mgs_map_plan_blocks", "mgs_map_plan_count", "mgs_map_plan_emit",
    "mgs_map_gather", "mgs_pack_mapping_grads", "mgs_sketch_assign", "mgs_sketch_residual",
    "mgs_tracking_iteration_second_order", "mgs_map_activate", "mgs_mapping_loss_partial_count",
    "mgs_mapping_loss_fused", "mgs_mapping_view_iteration", "mgs_map_finish_iteration", "mgs_map_append",
    "mgs_ssim_loss_partial_count", "mgs_ssim_loss", "mgs_refine_view_iteration",
    "mgs_tracking_iteration_rgbd", "mgs_tracking_iteration_second_order_rgbd", "mgs_tracking_loss_rgbd_fused",
    "mgs_sketch_residual_rgbd", "mgs_tracking_sample_scratch_bytes", "mgs_tracking_iteration_sampled",
    "mgs_keyframe_scratch_bytes", "mgs_keyframe_decide", "mgs_keyframe_seed_scratch_bytes", "mgs_keyframe_seed",
    "mgs_frame_prepare_args_size", "mgs_frame_prepare_scratch_bytes", "mgs_frame_prepare",
    "mgs_remap_build_args_size", "mgs_frame_remap_args_size", "mgs_remap_build", "mgs_frame_prepare_remapped",
    "mgs_stereo_depth_args_size", "mgs_stereo_scratch_bytes", "mgs_stereo_depth",
    "mgs_tracking_gn_args_size", "mgs_gauss_newton_scratch_bytes", "mgs_tracking_iteration_gauss_newton",
    "mgs_tracking_iteration_gauss_newton_rgbd", "mgs_normal_equations",
    "mgs_eval_score", "mgs_eval_score_partial_count", "mgs_eval_score_args_size", "mgs_eval_view_args_size",
    "mgs_eval_view",
    "mgs_view_compose_args_size", "mgs_view_compose_scratch_bytes", "mgs_view_compose",
    "mgs_view_ellipsoid_args_size", "mgs_view_ellipsoid",
    "mgs_view_time_colors_args_size", "mgs_view_time_colors_scratch_bytes", "mgs_view_time_colors",
    "mgs_view_overlay_args_size", "mgs_view_overlay_scratch_bytes", "mgs_view_overlay",
    "mgs_surface_args_size", "mgs_surface_forward", "mgs_depth_normal_args_size", "mgs_depth_normal",
    "mgs_tsdf_integrate_args_size", "mgs_tsdf_integrate", "mgs_tsdf_mesh_args_size", "mgs_tsdf_mesh_scratch_bytes",
    "mgs_tsdf_mesh_count", "mgs_tsdf_mesh_emit",
    "mgs_sparse_tsdf_volume_size", "mgs_sparse_tsdf_view_args_size", "mgs_sparse_tsdf_mesh_args_size",
    "mgs_sparse_tsdf_table_size", "mgs_sparse_tsdf_allocate_scratch_bytes", "mgs_sparse_tsdf_allocate",
    "mgs_sparse_tsdf_integrate", "mgs_sparse_tsdf_register", "mgs_sparse_tsdf_mesh_scratch_bytes",
    "mgs_sparse_tsdf_mesh_count", "mgs_sparse_tsdf_mesh_emit",
    "mgs_tsdf_raycast_args_size", "mgs_sparse_tsdf_raycast_args_size", "mgs_raycast_shade_args_size",
    "mgs_sparse_tsdf_raycast_scratch_bytes", "mgs_tsdf_raycast", "mgs_sparse_tsdf_raycast", "mgs_raycast_shade",
    "mgs_icp_args_size", "mgs_icp_scratch_bytes", "mgs_icp_align",
    "mgs_icp_intensity_args_size", "mgs_icp_rgbd_args_size", "mgs_icp_rgbd_scratch_bytes", "mgs_icp_intensity",
    "mgs_icp_align_rgbd",
    "mgs_mesh_clean_args_size", "mgs_mesh_clean_scratch_bytes", "mgs_mesh_clean_count", "mgs_mesh_clean_emit",
    "mgs_mesh_components",
    "mgs_surface_sample_args_size", "mgs_surface_sample_scratch_bytes", "mgs_surface_sample",
    "mgs_nearest_args_size", "mgs_nearest_scratch_bytes", "mgs_nearest_distance",
    "mgs_mesh_eval_args_size", "mgs_mesh_eval_scratch_bytes", "mgs_mesh_eval_stats", "mgs_mesh_eval_finish",
    "mgs_mesh_render_args_size", "mgs_mesh_render_scratch_bytes", "mgs_mesh_render",
    "mgs_vertex_visibility_args_size", "mgs_vertex_visibility",
    "mgs_mesh_cull_args_size", "mgs_mesh_cull_scratch_bytes", "mgs_mesh_cull_count", "mgs_mesh_cull_emit",
    "mgs_mesh_normals_args_size", "mgs_vertex_normals_scratch_bytes", "mgs_face_normals", "mgs_vertex_normals",
    "mgs_mesh_eval_normal_args_size", "mgs_mesh_eval_normal_scratch_bytes", "mgs_mesh_eval_normal_stats",
    "mgs_mesh_eval_normal_finish", "mgs_mesh_shade_args_size", "mgs_mesh_shade",
    "mgs_mesh_simplify_args_size", "mgs_mesh_simplify_scratch_bytes", "mgs_mesh_simplify_count", "mgs_mesh_simplify_emit",
    "mgs_mesh_edges_args_size", "mgs_mesh_edges_scratch_bytes", "mgs_mesh_edges_count", "mgs_mesh_edges_emit",
    "mgs_mesh_smooth_args_size", "mgs_mesh_smooth_scratch_bytes", "mgs_mesh_smooth",
)

_fp = C.c_void_p  # device pointers travel as plain addresses


class RasterShape(C.Structure):
    _fields_ = [("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
                ("pair_capacity", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float)]


class WorkspaceSizes(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "geom_bytes", "bins_bytes", "bwd_bytes", "sketch_bytes", "off_records",
        "off_pair_count", "off_tile_offset", "off_final_T", "off_n_contrib", "off_counters",
        "off_keys", "off_payload")]


class ForwardArgs(C.Structure):
    _fields_ = [("shape", RasterShape)] + [(n, _fp) for n in (
        "means3D", "scales", "rotations", "cov3D_precomp", "opacities", "shs", "colors_precomp",
        "viewmatrix", "projmatrix", "projmatrix_raw", "campos", "bg", "geom", "bins",
        "out_color", "out_depth", "out_opacity", "radii", "n_touched", "pair_count_out",
        "pair_count_max")] + [("big_tile_pass", C.c_int32), ("reserved0", C.c_int32)]


class MapAccumArgs(C.Structure):
    _fields_ = ([("scale_dims", C.c_int32), ("accumulate", C.c_int32), ("add_regulariser", C.c_int32),
                 ("regulariser_weight", C.c_float)]
                + [(n, _fp) for n in ("raw_rotations", "grad_xyz", "grad_features_dc", "grad_features_rest",
                                      "grad_opacity", "grad_scaling", "grad_rotation", "gradnorm_inc",
                                      "denom_inc", "radii_max", "visibility")])


class BackwardArgs(C.Structure):
    _fields_ = ([("fwd", ForwardArgs)] + [(n, _fp) for n in (
        "grad_color", "grad_depth", "bwd", "grad_means3D", "grad_means2D", "grad_colors",
        "grad_opacities", "grad_scales", "grad_rotations", "grad_cov3D", "grad_tau")]
        + [("sketch_mode", C.c_int32), ("sketch_dim", C.c_int32), ("stack_dim", C.c_int32),
           ("sketch_indices", _fp), ("grad_sketch_dtau", _fp), ("sketch_ws", _fp),
           ("sketch_bucket_flat", _fp), ("map_accum", C.POINTER(MapAccumArgs)),
           ("clamp_gradient_mode", C.c_int32), ("pair_count_bound", C.c_int32)])


class PoseAdamArgs(C.Structure):
    _fields_ = ([(n, _fp) for n in (
        "cam_rot_delta", "cam_trans_delta", "exposure_a", "exposure_b", "grad_rot", "grad_trans",
        "grad_a", "grad_b", "exp_avg", "exp_avg_sq", "T", "converged")]
        + [("step", C.c_int32)] + [(n, C.c_float) for n in (
            "lr_rot", "lr_trans", "lr_a", "lr_b", "beta1", "beta2", "eps", "converged_threshold")]
        + [("tau_partials", _fp), ("num_tau_partials", C.c_int32), ("exposure_partials", _fp),
           ("num_exposure_partials", C.c_int32), ("projection", _fp), ("viewmatrix_out", _fp),
           ("projmatrix_out", _fp), ("no_pose_update", C.c_int32), ("loss_partials", _fp),
           ("num_loss_partials", C.c_int32), ("loss_w_rgb", C.c_float), ("loss_w_depth", C.c_float),
           ("loss_view", _fp), ("loss_accum", _fp), ("loss_grad_out", _fp),
           ("loss_norm_mode", C.c_int32), ("sticky_converged", C.c_int32), ("l1_partials", _fp),
           ("best", _fp), ("num_l1_partials", C.c_int32), ("loss_pnorm", C.c_float)])


TRACK_BEST_FLOATS = 24     # MGS_TRACK_BEST_FLOATS: {best L1, T[16], a, b, index of the best iteration, counter,
                           #  L1 of the last iteration's render, |step| of the last iteration, spare}


class MappingLossArgs(C.Structure):
    _fields_ = ([(n, _fp) for n in ("image", "gt", "mask", "depth", "gt_depth", "exposure_a", "exposure_b")]
                + [("exposure_eps", C.c_float), ("w_rgb", C.c_float), ("w_depth", C.c_float),
                   ("depth_mask_threshold", C.c_float), ("apply_exposure", C.c_int32),
                   ("num_pixels", C.c_int64)]
                + [(n, _fp) for n in ("partial", "loss", "grad_out", "grad_image", "grad_depth",
                                      "grad_a", "grad_b")]
                + [("partial_ticket_ready", C.c_int32), ("reserved0", C.c_int32)])


class LMStepArgs(C.Structure):
    _fields_ = [("SJ", _fp), ("Sf", _fp), ("rows", C.c_int32), ("lam", C.c_float), ("T", _fp),
                ("exposure_a", _fp), ("exposure_b", _fp), ("x_out", _fp),
                ("sj_tau", _fp), ("sj_exposure", _fp), ("lm_state", _fp), ("loss", _fp),
                ("increase_factor", C.c_float), ("decrease_factor", C.c_float),
                ("min_lambda", C.c_float), ("max_lambda", C.c_float), ("converged_threshold", C.c_float),
                ("reserved0", C.c_int32), ("best", _fp), ("projection", _fp), ("viewmatrix_out", _fp),
                ("projmatrix_out", _fp), ("zero_after", _fp), ("zero_count", C.c_int32), ("reserved1", C.c_int32)]


class TrackingLossArgs(C.Structure):
    _fields_ = ([(n, _fp) for n in ("image", "opacity", "gt", "mask", "exposure_a", "exposure_b")]
                + [("exposure_eps", C.c_float), ("huber_delta", C.c_float), ("num_pixels", C.c_int64)]
                + [(n, _fp) for n in ("partial", "scalars", "grad_out", "grad_image", "grad_a", "grad_b")]
                + [("pnorm", C.c_float), ("reserved0", C.c_int32)])


class TrackingIterArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("bwd", _fp), ("grad_image", _fp), ("grad_tau", _fp),
                ("grad_exposure", _fp), ("one", _fp), ("loss", TrackingLossArgs),
                ("adam", PoseAdamArgs), ("camera_matrices_valid", C.c_int32), ("reserved0", C.c_int32),
                ("best", _fp)]


class SketchResidualArgs(C.Structure):
    _fields_ = ([(n, _fp) for n in ("image", "opacity", "gt", "mask", "exposure_a", "exposure_b")]
                + [("exposure_eps", C.c_float), ("huber_delta", C.c_float), ("num_pixels", C.c_int64),
                   ("stack_dim", C.c_int32), ("sketch_dim", C.c_int32)]
                + [(n, _fp) for n in ("bucket", "weights", "grad_image", "Sf", "sj_exposure", "l1")]
                + [("assign", C.c_int32), ("reserved0", C.c_int32), ("assign_key", C.c_uint64)])


class TrackingSOArgs(C.Structure):
    _fields_ = [("base", TrackingIterArgs), ("stack_dim", C.c_int32), ("sketch_dim", C.c_int32),
                ("key", C.c_uint64), ("bucket", _fp), ("weights", _fp), ("accum", _fp),
                ("sketch_ws", _fp), ("lm", LMStepArgs), ("scratch_kept_zero", C.c_int32), ("repeat_dim", C.c_int32)]


class TrackingGNArgs(C.Structure):
    _fields_ = [("base", TrackingIterArgs), ("stack_dim", C.c_int32), ("sketch_dim", C.c_int32),
                ("sketch_ws", _fp), ("scratch", _fp), ("lm", LMStepArgs), ("normal_out", _fp)]


NORMAL_SUMS = 44           # upper triangle of H (36, row-major, i <= j) then g (8)


ADAM_MAX_GROUPS = 8
GATHER_MAX_TENSORS = 24
GATHER_COPY, GATHER_ZERO_NEW, GATHER_SPLIT_SCALING, GATHER_SPLIT_XYZ = 0, 1, 2, 3


class AdamGroup(C.Structure):
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp),
                ("numel", C.c_int64), ("lr", C.c_float), ("step", C.c_int32)]


class MapPlanArgs(C.Structure):
    _fields_ = ([("n", C.c_int32)] + [(n, _fp) for n in ("grad_accum", "denom", "log_scales", "opacity_logit")]
                + [(n, C.c_float) for n in ("grad_threshold", "dense_extent", "min_opacity", "big_extent")]
                + [(n, _fp) for n in ("prune_mask", "flags", "block_counts", "totals", "src_index", "noise_row")])


class GatherTensor(C.Structure):
    _fields_ = [("src", _fp), ("dst", _fp), ("width", C.c_int32), ("mode", C.c_int32)]


class MapGatherArgs(C.Structure):
    _fields_ = [("tensors", GatherTensor * GATHER_MAX_TENSORS), ("num_tensors", C.c_int32),
                ("rows", C.c_int64), ("num_children", C.c_int32), ("src_index", _fp),
                ("rotations", _fp), ("log_scales", _fp), ("noise", _fp), ("noise_row", _fp)]


class MapActivateArgs(C.Structure):
    _fields_ = ([("num_gaussians", C.c_int32), ("scale_dims", C.c_int32), ("sh_coeffs", C.c_int32)]
                + [(n, _fp) for n in ("log_scales", "raw_rotations", "opacity_logits", "features_dc",
                                      "features_rest", "scales", "rotations", "opacities", "shs")])


class MappingViewArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("bwd", _fp), ("grad_image", _fp), ("grad_depth", _fp), ("grad_tau", _fp),
                ("loss", MappingLossArgs), ("adam", PoseAdamArgs), ("accum", MapAccumArgs),
                ("loss_view", _fp), ("loss_accum", _fp), ("camera_matrices_valid", C.c_int32),
                ("forward_only", C.c_int32)]


class MapFinishArgs(C.Structure):
    _fields_ = ([("num_gaussians", C.c_int32)]
                + [(n, _fp) for n in ("gradnorm_inc", "denom_inc", "radii_max", "xyz_gradient_accum", "denom",
                                      "max_radii2D")]
                + [("reset_mode", C.c_int32), ("reset_value", C.c_float)]
                + [(n, _fp) for n in ("opacity_logits", "opacity_exp_avg", "opacity_exp_avg_sq")])


class MapAppendArgs(C.Structure):
    _fields_ = [("tensors", GatherTensor * GATHER_MAX_TENSORS), ("new_rows", _fp * GATHER_MAX_TENSORS),
                ("num_tensors", C.c_int32), ("rows_old", C.c_int64), ("rows_new", C.c_int64)]


class SsimLossArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("channels", "height", "width")]
                + [("w_l1", C.c_float), ("w_ssim", C.c_float), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("image", "gt", "grad_out", "grad_image", "partial", "l1", "ssim", "loss")])


class RefineViewArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("bwd", _fp), ("grad_image", _fp), ("grad_tau", _fp), ("T", _fp),
                ("loss", SsimLossArgs), ("accum", MapAccumArgs), ("max_radii2D", _fp),
                ("camera_matrices_valid", C.c_int32), ("reserved0", C.c_int32)]


class TrackingDepthArgs(C.Structure):
    _fields_ = ([(n, _fp) for n in ("depth", "gt_depth", "grad_depth")]
                + [(n, C.c_float) for n in ("w_rgb", "w_depth", "depth_threshold", "opacity_threshold")])


class TrackingSampleArgs(C.Structure):
    _fields_ = [("num_samples", C.c_int32), ("reserved0", C.c_int32), ("key", C.c_uint64), ("indices", _fp),
                ("scratch", _fp), ("replay_indices", _fp), ("grad_out", _fp)]


TRACK_SAMPLE_MAX = 65536

KF_MAX_WINDOW = 16


class KeyframeArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_gaussians", "num_pixels", "window_len", "window_size", "check_time",
                                          "initialized", "monocular", "single_thread")]
                + [(n, C.c_float) for n in ("kf_translation", "kf_min_translation", "kf_overlap", "kf_cutoff")]
                + [(n, _fp) for n in ("n_touched", "depth", "opacity", "T_cur")]
                + [("T_window", _fp * KF_MAX_WINDOW), ("visibility", _fp * KF_MAX_WINDOW),
                   ("visibility_len", C.c_int64 * KF_MAX_WINDOW), ("scratch", _fp), ("result", _fp)])


class KeyframeResult(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("create_kf", "removed", "reset", "n_valid", "removed_cutoff",
                                          "removed_evict", "n_cur", "flags")]
                + [("median_depth", C.c_float), ("dist", C.c_float), ("overlap", C.c_float), ("window_len", C.c_int32),
                   ("ss_ratio", C.c_float * KF_MAX_WINDOW), ("n_row", C.c_int32 * KF_MAX_WINDOW),
                   ("n_inter", C.c_int32 * KF_MAX_WINDOW), ("score", C.c_double * KF_MAX_WINDOW)])

class KeyframeSeedResult(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_points", "n_valid", "n_outliers", "n_depth")]
                + [(n, C.c_float) for n in ("median_depth", "std_depth", "median_all", "point_size")])


class KeyframeSeedArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "row_capacity", "mode", "adaptive_pointsize", "isotropic")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "rgb_boundary_threshold", "downsample",
                                            "depth_trunc", "exposure_eps")]
                + [("point_size", C.c_double), ("seed", C.c_uint64)]
                + [(n, _fp) for n in ("image", "depth", "opacity", "T", "exposure_a", "exposure_b", "noise", "keys",
                                      "xyz", "features_dc", "log_scales", "rots", "opacity_logit", "pixel_index",
                                      "depth_out", "scratch", "result")]
                + [("result_host", C.POINTER(KeyframeSeedResult))])


FRAME_IMAGE_F32_CHW, FRAME_IMAGE_U8_HWC = 0, 1
FRAME_DEPTH_NONE, FRAME_DEPTH_F32, FRAME_DEPTH_U16 = 0, 1, 2
FRAME_MODE_GLOBAL, FRAME_MODE_PATCH = 0, 1
FRAME_PATCH_SIZE = 32


class FramePrepareArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "mode", "image_format", "depth_format")]
                + [("edge_threshold", C.c_float), ("rgb_boundary_threshold", C.c_float), ("reserved0", C.c_int32),
                   ("depth_scale", C.c_double)]
                + [(n, _fp) for n in ("image_in", "depth_in", "image", "gt_depth", "grad_mask", "rgb_pixel_mask",
                                      "rgb_pixel_mask_mapping", "median_out", "intensity_out", "scratch")])


FRAME_REMAP_DEPTH_NONE, FRAME_REMAP_DEPTH_NEAREST = 0, 1


class RemapBuildArgs(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ir", C.c_double * 9), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 5), ("map_q5", _fp)]


class FrameRemapArgs(C.Structure):
    _fields_ = [("map_q5", _fp), ("depth_mode", C.c_int32), ("reserved0", C.c_int32)]


STEREO_IMAGE_U8_GREY, STEREO_IMAGE_U8_HWC, STEREO_IMAGE_F32_CHW = 0, 1, 2
STEREO_DISPARITIES = 64


class StereoDepthArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "image_format", "num_disparities", "block_size",
                                          "uniqueness_ratio")]
                + [("bf", C.c_double)]
                + [(n, _fp) for n in ("left_in", "right_in", "map_left", "map_right", "depth", "disp16", "image",
                                      "scratch")])


EVAL_RECORD_DOUBLES = 8    # MGS_EVAL_RECORD_DOUBLES; the indices below are MGS_EVAL_*
(EVAL_SSE, EVAL_SSE_ALL, EVAL_ABS, EVAL_SSIM, EVAL_DEPTH_ABS, EVAL_N_MASK, EVAL_N_DEPTH, EVAL_PAIRS) = range(8)
EVAL_GT_F32_CHW, EVAL_GT_U8_HWC = 0, 1


class EvalScoreArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("height", "width", "gt_format", "row", "num_rows", "apply_exposure")]
                + [("exposure_eps", C.c_float), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("image", "gt", "depth", "gt_depth", "exposure_a", "exposure_b", "pair_count",
                                      "partial", "table")])


class EvalViewArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("T", _fp), ("score", EvalScoreArgs), ("camera_matrices_valid", C.c_int32),
                ("reserved0", C.c_int32)]


VIEW_RGB, VIEW_DEPTH, VIEW_OPACITY, VIEW_FLAT_BALL, VIEW_GAUSSIAN_BALL = 0, 1, 2, 3, 4     # MGS_VIEW_*


class ViewComposeArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "mode", "reserved0")]
                + [(n, _fp) for n in ("src", "lut", "out", "scratch")])


class ViewEllipsoidArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("mode", C.c_int32), ("reserved0", C.c_int32), ("hit_color", _fp),
                ("hit_depth", _fp)]


class ViewTimeColorsArgs(C.Structure):
    _fields_ = ([("num_gaussians", C.c_int32), ("sh_coeffs", C.c_int32)]
                + [(n, _fp) for n in ("features", "kf_ids", "lut", "out", "scratch")])


class ViewOverlayArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "num_poses", "num_free")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "frustum_size", "near_z")]
                + [(n, _fp) for n in ("T_view", "poses", "free_segments", "pose_colors", "free_colors", "endpoints",
                                      "frame", "scratch")])


class SurfaceArgs(C.Structure):
    _fields_ = [("fwd", ForwardArgs), ("median_depth", _fp), ("median_index", _fp)]


class DepthNormalArgs(C.Structure):
    _fields_ = ([("width", C.c_int32), ("height", C.c_int32)]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "pixel_center", "max_jump")]
                + [("depth", _fp), ("normal", _fp)])


TSDF_MAX_POINTS = (2 ** 31 - 1) // 7     # 7 nx ny nz < 2^31: the edge keys of the extraction are 32-bit


class TsdfIntegrateArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("nx", "ny", "nz", "width", "height", "normalize")]
                + [("origin", C.c_float * 3)]
                + [(n, C.c_float) for n in ("voxel_size", "trunc", "fx", "fy", "cx", "cy", "z_near", "depth_min",
                                            "depth_max", "min_opacity", "weight", "max_weight")]
                + [("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("T", "depth", "opacity", "image", "tsdf", "wsum", "color")])


class TsdfMeshArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("nx", "ny", "nz", "reserved0")] + [("origin", C.c_float * 3)]
                + [("voxel_size", C.c_float), ("min_weight", C.c_float), ("reserved1", C.c_int32)]
                + [(n, _fp) for n in ("tsdf", "weight", "color", "scratch", "counts", "verts", "faces", "colors")]
                + [("num_verts", C.c_int32), ("num_faces", C.c_int32)])


SPARSE_TSDF_BRICK = 8                                    # points along a brick's edge
SPARSE_TSDF_MAX_BRICKS = (2 ** 31 - 1) // (7 * 512)      # 7 * 512 * max_bricks < 2^31: 599186
SPARSE_TSDF_COORD_RANGE = 2 ** 20                        # brick coordinates lie in [-2^20, 2^20)


class SparseTsdfVolume(C.Structure):
    _fields_ = ([("max_bricks", C.c_int32), ("reserved0", C.c_int32), ("origin", C.c_float * 3),
                 ("voxel_size", C.c_float)]
                + [(n, _fp) for n in ("tsdf", "weight", "color", "brick_coords", "map_keys", "map_vals", "state")])


class SparseTsdfViewArgs(C.Structure):
    _fields_ = ([("vol", SparseTsdfVolume)]
                + [(n, C.c_int32) for n in ("width", "height", "normalize", "samples")]
                + [(n, C.c_float) for n in ("trunc", "fx", "fy", "cx", "cy", "z_near", "depth_min", "depth_max",
                                            "min_opacity", "view_weight", "max_weight")]
                + [("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("T", "depth", "opacity", "image", "scratch")])


class SparseTsdfMeshArgs(C.Structure):
    _fields_ = ([("vol", SparseTsdfVolume), ("num_bricks", C.c_int32), ("min_weight", C.c_float)]
                + [(n, _fp) for n in ("scratch", "counts", "verts", "faces", "colors")]
                + [("num_verts", C.c_int32), ("num_faces", C.c_int32)])


RAYCAST_FRAME_CAMERA, RAYCAST_FRAME_WORLD = 0, 1          # MGS_RAYCAST_FRAME_*
RAYCAST_MAX_STEPS = 1 << 20                              # MGS_RAYCAST_MAX_STEPS
RAYCAST_SHADE_SHADED, RAYCAST_SHADE_NORMAL, RAYCAST_SHADE_COLOR, RAYCAST_SHADE_DEPTH = 0, 1, 2, 3     # MGS_RAYCAST_SHADE_*


class RaycastView(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "num_steps", "frame", "skip", "reserved0")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "z_near", "dz", "min_weight")]
                + [("reserved1", C.c_int32)]
                + [(n, _fp) for n in ("T", "depth", "normal", "color", "hit_step", "evaluated")])


class TsdfRaycastArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("nx", "ny", "nz", "reserved0")] + [("origin", C.c_float * 3)]
                + [("voxel_size", C.c_float)] + [(n, _fp) for n in ("tsdf", "weight", "color")] + [("view", RaycastView)])


class SparseTsdfRaycastArgs(C.Structure):
    _fields_ = [("vol", SparseTsdfVolume), ("view", RaycastView), ("scratch", _fp), ("build_table", C.c_int32),
                ("reserved0", C.c_int32)]


class RaycastShadeArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "mode")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "depth_lo", "depth_hi")] + [("background", C.c_uint8 * 4)]
                + [(n, _fp) for n in ("depth", "normal", "color", "hit_step", "lut", "out")])


# MGS_ICP_*: the statuses, then the sizes
ICP_ITERATING, ICP_CONVERGED, ICP_MAX_ITERATIONS, ICP_TOO_FEW, ICP_DEGENERATE, ICP_STEP_TOO_LARGE = range(6)
ICP_MAX_LEVELS, ICP_MAX_ITERATIONS_TOTAL, ICP_SUMS, ICP_RECORD_WORDS, ICP_HISTORY_WORDS = 8, 1024, 35, 56, 8
ICP_ROWS_BLOCKS, ICP_EXP_TERMS, ICP_MAX_PIXELS = 256, 7, 1 << 22


class IcpArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "model_width", "model_height", "model_normal_chw", "num_levels",
                                          "min_pixels", "reserved0")]
                + [("stride", C.c_int32 * ICP_MAX_LEVELS), ("iterations", C.c_int32 * ICP_MAX_LEVELS)]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mfx", "mfy", "mcx", "mcy", "dist", "cos_min", "depth_max",
                                            "reserved1")]
                + [(n, C.c_double) for n in ("min_pivot_ratio", "damping", "converged")]
                + [(n, _fp) for n in ("depth", "normal", "model_depth", "model_normal", "T_model", "T_init", "scratch", "T_w2c",
                                      "D", "record")])


ICP_RGBD_SUMS, ICP_PHOTO_WEIGHT_MAX = 39, 1024.0      # MGS_ICP_RGBD_SUMS, MGS_ICP_PHOTO_WEIGHT_MAX


class IcpIntensityArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "chw", "reserved0")]
                + [(n, _fp) for n in ("rgb", "valid", "out")])


class IcpRgbdArgs(C.Structure):
    _fields_ = [("icp", IcpArgs), ("photo_weight", C.c_float), ("image_chw", C.c_int32), ("model_color_chw", C.c_int32),
                ("reserved0", C.c_int32)] + [(n, _fp) for n in ("image", "model_color", "intensity", "model_intensity")]


MESH_CLEAN_MAX_ITEMS = (2 ** 31 - 1) // 3     # 3 V, 3 F < 2^31: 32-bit element indices of the [n,3] arrays
MESH_CLEAN_COUNTS = 5                         # V', F', clusters, kept clusters, bad faces


class MeshCleanArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "keep_largest", "min_faces")]
                + [(n, _fp) for n in ("verts", "faces", "colors", "scratch", "counts", "labels", "out_verts",
                                      "out_faces", "out_colors")]
                + [("out_num_verts", C.c_int32), ("out_num_faces", C.c_int32)])


MESH_EVAL_MAX_ITEMS = (2 ** 31 - 1) // 3      # 3 n < 2^31 for vertices, faces, samples, queries and reference points
SAMPLE_RECORD_INTS = 4                        # MGS_SAMPLE_RECORD_INTS: T == 0, bad faces, low and high word of T
NEAREST_MAX_CELLS, NEAREST_MAX_DIM = 1 << 21, 1024
MESH_EVAL_RECORD_DOUBLES = 12                 # {n finite, n below, max d, sum d} x 2, then {T == 0, bad faces} x 2


class SurfaceSampleArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "num_samples", "reserved0")]
                + [("seed", C.c_uint64)]
                + [(n, _fp) for n in ("verts", "faces", "randoms", "scratch", "points", "face_index", "record")])


class NearestArgs(C.Structure):
    _fields_ = ([("num_query", C.c_int32), ("num_ref", C.c_int32), ("cell_size", C.c_float), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("query", "ref", "scratch", "d2", "index")])


class MeshEvalArgs(C.Structure):
    _fields_ = ([("num", C.c_int32), ("direction", C.c_int32), ("threshold", C.c_float), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("d2", "scratch", "record")] + [("sample_record", _fp * 2)])


MESH_RENDER_RECORD_INTS = 4                   # MGS_MESH_RENDER_RECORD_INTS: bad faces, skipped faces, large faces, spare
MESH_RENDER_LARGE_BOX = 1024                  # MGS_MESH_RENDER_LARGE_BOX: box pixels above which a face takes the large path
MESH_RENDER_LARGE_GRID = 256                  # MGS_MESH_RENDER_LARGE_GRID: workgroups that stride the large-face list
MESH_RENDER_MAX_PIXELS = 2 ** 31 - 1
MESH_CULL_COUNTS = 4                          # V', F', bad faces, spare


class MeshRenderArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "width", "height", "large_threshold", "large_grid")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "z_near")] + [("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("verts", "faces", "T", "scratch", "depth", "face_id", "record")])


class VertexVisibilityArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "width", "height", "empty_visible")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "z_near", "eps")]
                + [(n, _fp) for n in ("verts", "T", "depth", "seen_count")])


class MeshCullArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "min_views", "rule")]
                + [(n, _fp) for n in ("verts", "faces", "colors", "seen_count", "scratch", "counts", "out_verts",
                                      "out_faces", "out_colors")]
                + [("out_num_verts", C.c_int32), ("out_num_faces", C.c_int32)])


MESH_NORMAL_RECORD_INTS = 2                   # MGS_MESH_NORMAL_RECORD_INTS: bad faces, degenerate faces
MESH_EVAL_NORMAL_DOUBLES = 8                  # MGS_MESH_EVAL_NORMAL_DOUBLES: {pairs, sum |t|, t < 0, skipped} x 2
MESH_SHADE_SHADED, MESH_SHADE_NORMAL, MESH_SHADE_COLOR, MESH_SHADE_MASK = 0, 1, 2, 3     # MGS_MESH_SHADE_*


class MeshNormalsArgs(C.Structure):
    _fields_ = ([("num_verts", C.c_int32), ("num_faces", C.c_int32)]
                + [(n, _fp) for n in ("verts", "faces", "scratch", "normals", "record")])


class MeshEvalNormalArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num", "num_ref", "num_faces", "num_ref_faces", "direction", "reserved0")]
                + [(n, _fp) for n in ("d2", "index", "face", "ref_face", "normals", "ref_normals", "scratch", "record")])


class MeshShadeArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "width", "height", "mode", "colors_u8")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "z_near")] + [("background", C.c_uint8 * 4)]
                + [(n, _fp) for n in ("verts", "faces", "T", "face_id", "face_normal", "colors", "out")])


MESH_SIMPLIFY_COUNTS = 8                      # MGS_MESH_SIMPLIFY_COUNTS: V', F', clusters, collapsed, duplicates, bad vertices, bad faces, spare


class MeshSimplifyArgs(C.Structure):
    _fields_ = ([("num_verts", C.c_int32), ("num_faces", C.c_int32), ("cell", C.c_float), ("origin_from_verts", C.c_int32),
                 ("origin", C.c_float * 3), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("verts", "faces", "colors", "scratch", "counts", "out_verts", "out_faces", "out_colors")]
                + [("out_num_verts", C.c_int32), ("out_num_faces", C.c_int32)])


MESH_EDGES_RECORD_INTS = 16                   # MGS_MESH_EDGES_RECORD_INTS: edges, degree sum, referenced, boundary vertices,
                                              # boundary / manifold / non-manifold / inconsistent edges, degenerate faces,
                                              # bad faces, bad vertices, spare
MESH_SMOOTH_MAX_ITERATIONS = 1000             # MGS_MESH_SMOOTH_MAX_ITERATIONS
MESH_EDGES_MAX_FACES = (1 << 30) // 3         # 3 F <= 2^30: the hash table of the half-edges holds at most 2^31 words


class MeshEdgesArgs(C.Structure):
    _fields_ = ([("num_verts", C.c_int32), ("num_faces", C.c_int32)]
                + [(n, _fp) for n in ("faces", "scratch", "record", "vertex_degree", "vertex_flags", "edges", "edge_faces")]
                + [("out_num_edges", C.c_int32), ("reserved0", C.c_int32)])


class MeshSmoothArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("num_verts", "num_faces", "iterations", "taubin", "boundary_free")]
                + [("lam", C.c_float), ("mu", C.c_float), ("reserved0", C.c_int32)]
                + [(n, _fp) for n in ("verts", "faces", "scratch", "record", "out_verts")])


_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the native library; raise loudly if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.")
    # PyTorch first: its wheel carries its own copy of the HIP runtime.  If this library were loaded before
    # torch, its DT_NEEDED libamdhip64 would bind to the system copy, torch would bring in (and initialise)
    # a second runtime instance, and launches through this library fail with "no ROCm-capable device is
    # detected" (seen with `python __graft_entry__.py smoke`, which builds - and used to load - before
    # importing torch).  With torch's runtime already in the process the loader resolves ours to it.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}")
    L.mgs_camera_from_pose.restype = C.c_int32
    L.mgs_camera_from_pose.argtypes = [C.c_void_p] * 5
    L.mgs_tracking_iteration.restype = C.c_int32
    L.mgs_tracking_iteration.argtypes = [C.POINTER(TrackingIterArgs), C.c_void_p]
    L.mgs_adam_step_multi.restype = C.c_int32
    L.mgs_adam_step_multi.argtypes = [C.POINTER(AdamGroup), C.c_int32, C.c_double, C.c_double, C.c_double,
                                      C.c_void_p]
    L.mgs_tracking_loss_onepass.restype = C.c_int32
    L.mgs_tracking_loss_onepass.argtypes = [C.POINTER(TrackingLossArgs), C.POINTER(C.c_int32), C.c_void_p]
    L.mgs_sketch_assign.restype = C.c_int32
    L.mgs_sketch_assign.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    L.mgs_sketch_residual.restype = C.c_int32
    L.mgs_sketch_residual.argtypes = [C.POINTER(SketchResidualArgs), C.c_void_p]
    L.mgs_tracking_iteration_second_order.restype = C.c_int32
    L.mgs_tracking_iteration_second_order.argtypes = [C.POINTER(TrackingSOArgs), C.c_void_p]
    L.mgs_pack_mapping_grads.restype = C.c_int32
    L.mgs_pack_mapping_grads.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mgs_map_plan_blocks.restype = C.c_int32
    L.mgs_map_plan_blocks.argtypes = [C.c_int32]
    for fn in (L.mgs_map_plan_count, L.mgs_map_plan_emit):
        fn.restype = C.c_int32
        fn.argtypes = [C.POINTER(MapPlanArgs), C.c_void_p]
    L.mgs_map_gather.restype = C.c_int32
    L.mgs_map_gather.argtypes = [C.POINTER(MapGatherArgs), C.c_void_p]
    L.mgs_abi_version.restype = C.c_int32
    L.mgs_status_string.restype = C.c_char_p
    L.mgs_status_string.argtypes = [C.c_int32]
    L.mgs_raster_workspace_query.restype = C.c_int32
    L.mgs_raster_workspace_query.argtypes = [C.POINTER(RasterShape), C.POINTER(WorkspaceSizes)]
    for fn in (L.mgs_raster_forward_project, L.mgs_raster_forward_blend):
        fn.restype = C.c_int32
        fn.argtypes = [C.POINTER(ForwardArgs), C.c_void_p]
    L.mgs_raster_backward.restype = C.c_int32
    L.mgs_raster_backward.argtypes = [C.POINTER(BackwardArgs), C.c_void_p]
    L.mgs_knn_scratch_bytes.restype = C.c_uint64
    L.mgs_knn_scratch_bytes.argtypes = [C.c_int32]
    L.mgs_knn_dist2.restype = C.c_int32
    L.mgs_knn_dist2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mgs_profile_enable.restype = C.c_int32
    L.mgs_profile_enable.argtypes = [C.c_int32]
    L.mgs_profile_read.restype = C.c_int32
    L.mgs_profile_read.argtypes = [C.c_int32, C.c_char_p, C.POINTER(C.c_float),
                                   C.POINTER(C.c_int32)]
    L.mgs_pose_adam_step.restype = C.c_int32
    L.mgs_pose_adam_step.argtypes = [C.POINTER(PoseAdamArgs), C.c_void_p]
    for fn in (L.mgs_mapping_loss_forward, L.mgs_mapping_loss_backward):
        fn.restype = C.c_int32
        fn.argtypes = [C.POINTER(MappingLossArgs), C.c_void_p]
    L.mgs_lm_solve_step.restype = C.c_int32
    L.mgs_lm_solve_step.argtypes = [C.POINTER(LMStepArgs), C.c_void_p]
    L.mgs_tracking_loss_partial_count.restype = C.c_int32
    L.mgs_tracking_loss_partial_count.argtypes = [C.c_int64]
    for fn in (L.mgs_tracking_loss_forward, L.mgs_tracking_loss_backward):
        fn.restype = C.c_int32
        fn.argtypes = [C.POINTER(TrackingLossArgs), C.c_void_p]
    L.mgs_struct_size.restype = C.c_int32
    L.mgs_struct_size.argtypes = [C.c_int32]
    L.mgs_map_activate.restype = C.c_int32
    L.mgs_map_activate.argtypes = [C.POINTER(MapActivateArgs), C.c_void_p]
    L.mgs_mapping_loss_partial_count.restype = C.c_int32
    L.mgs_mapping_loss_partial_count.argtypes = [C.c_int64]
    L.mgs_mapping_loss_fused.restype = C.c_int32
    L.mgs_mapping_loss_fused.argtypes = [C.POINTER(MappingLossArgs), C.c_void_p, C.c_void_p]
    L.mgs_mapping_view_iteration.restype = C.c_int32
    L.mgs_mapping_view_iteration.argtypes = [C.POINTER(MappingViewArgs), C.c_void_p]
    L.mgs_map_finish_iteration.restype = C.c_int32
    L.mgs_map_finish_iteration.argtypes = [C.POINTER(MapFinishArgs), C.c_void_p]
    L.mgs_map_append.restype = C.c_int32
    L.mgs_map_append.argtypes = [C.POINTER(MapAppendArgs), C.c_void_p]
    L.mgs_ssim_loss_partial_count.restype = C.c_int32
    L.mgs_ssim_loss_partial_count.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mgs_ssim_loss.restype = C.c_int32
    L.mgs_ssim_loss.argtypes = [C.POINTER(SsimLossArgs), C.c_void_p]
    L.mgs_refine_view_iteration.restype = C.c_int32
    L.mgs_refine_view_iteration.argtypes = [C.POINTER(RefineViewArgs), C.c_void_p]
    _dp = C.POINTER(TrackingDepthArgs)
    L.mgs_tracking_iteration_rgbd.restype = C.c_int32
    L.mgs_tracking_iteration_rgbd.argtypes = [C.POINTER(TrackingIterArgs), _dp, C.c_void_p]
    L.mgs_tracking_iteration_second_order_rgbd.restype = C.c_int32
    L.mgs_tracking_iteration_second_order_rgbd.argtypes = [C.POINTER(TrackingSOArgs), _dp, C.c_void_p]
    L.mgs_tracking_loss_rgbd_fused.restype = C.c_int32
    L.mgs_tracking_loss_rgbd_fused.argtypes = [C.POINTER(TrackingLossArgs), _dp, C.POINTER(C.c_int32), C.c_void_p]
    L.mgs_sketch_residual_rgbd.restype = C.c_int32
    L.mgs_sketch_residual_rgbd.argtypes = [C.POINTER(SketchResidualArgs), _dp, C.c_void_p]
    L.mgs_tracking_sample_scratch_bytes.restype = C.c_uint64
    L.mgs_tracking_sample_scratch_bytes.argtypes = [C.POINTER(RasterShape), C.c_int32]
    L.mgs_tracking_iteration_sampled.restype = C.c_int32
    L.mgs_tracking_iteration_sampled.argtypes = [C.POINTER(TrackingIterArgs), _dp, C.POINTER(TrackingSampleArgs),
                                                 C.c_void_p]
    L.mgs_keyframe_scratch_bytes.restype = C.c_uint64
    L.mgs_keyframe_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mgs_keyframe_decide.restype = C.c_int32
    L.mgs_keyframe_decide.argtypes = [C.POINTER(KeyframeArgs), C.c_void_p]
    L.mgs_keyframe_seed_scratch_bytes.restype = C.c_uint64
    L.mgs_keyframe_seed_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    L.mgs_keyframe_seed.restype = C.c_int32
    L.mgs_keyframe_seed.argtypes = [C.POINTER(KeyframeSeedArgs), C.c_void_p]
    L.mgs_frame_prepare_args_size.restype = C.c_int32
    L.mgs_frame_prepare_args_size.argtypes = []
    if L.mgs_frame_prepare_args_size() != C.sizeof(FramePrepareArgs):     # not in mgs_struct_size()'s list: checked here
        raise NativeLibraryError("FramePrepareArgs does not have the size of mgs_frame_prepare_args")
    L.mgs_frame_prepare_scratch_bytes.restype = C.c_uint64
    L.mgs_frame_prepare_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    L.mgs_frame_prepare.restype = C.c_int32
    L.mgs_frame_prepare.argtypes = [C.POINTER(FramePrepareArgs), C.c_void_p]
    for fn, cls in ((L.mgs_remap_build_args_size, RemapBuildArgs), (L.mgs_frame_remap_args_size, FrameRemapArgs)):
        fn.restype, fn.argtypes = C.c_int32, []
        if fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    L.mgs_remap_build.restype = C.c_int32
    L.mgs_remap_build.argtypes = [C.POINTER(RemapBuildArgs), C.c_void_p]
    L.mgs_frame_prepare_remapped.restype = C.c_int32
    L.mgs_frame_prepare_remapped.argtypes = [C.POINTER(FramePrepareArgs), C.POINTER(FrameRemapArgs), C.c_void_p]
    L.mgs_stereo_depth_args_size.restype, L.mgs_stereo_depth_args_size.argtypes = C.c_int32, []
    if L.mgs_stereo_depth_args_size() != C.sizeof(StereoDepthArgs):
        raise NativeLibraryError("StereoDepthArgs does not have the size of mgs_stereo_depth_args")
    L.mgs_stereo_scratch_bytes.restype = C.c_uint64
    L.mgs_stereo_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    L.mgs_stereo_depth.restype = C.c_int32
    L.mgs_stereo_depth.argtypes = [C.POINTER(StereoDepthArgs), C.c_void_p]
    L.mgs_tracking_gn_args_size.restype, L.mgs_tracking_gn_args_size.argtypes = C.c_int32, []
    if L.mgs_tracking_gn_args_size() != C.sizeof(TrackingGNArgs):
        raise NativeLibraryError("TrackingGNArgs does not have the size of mgs_tracking_gn_args")
    L.mgs_gauss_newton_scratch_bytes.restype = C.c_uint64
    L.mgs_gauss_newton_scratch_bytes.argtypes = [C.POINTER(RasterShape)]
    L.mgs_tracking_iteration_gauss_newton.restype = C.c_int32
    L.mgs_tracking_iteration_gauss_newton.argtypes = [C.POINTER(TrackingGNArgs), C.c_void_p]
    L.mgs_tracking_iteration_gauss_newton_rgbd.restype = C.c_int32
    L.mgs_tracking_iteration_gauss_newton_rgbd.argtypes = [C.POINTER(TrackingGNArgs), _dp, C.c_void_p]
    L.mgs_normal_equations.restype = C.c_int32
    L.mgs_normal_equations.argtypes = [C.POINTER(TrackingGNArgs), _dp, C.c_void_p]
    for fn, cls in ((L.mgs_eval_score_args_size, EvalScoreArgs), (L.mgs_eval_view_args_size, EvalViewArgs)):
        fn.restype, fn.argtypes = C.c_int32, []
        if fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    L.mgs_eval_score_partial_count.restype = C.c_int32
    L.mgs_eval_score_partial_count.argtypes = [C.c_int32, C.c_int32]
    L.mgs_eval_score.restype = C.c_int32
    L.mgs_eval_score.argtypes = [C.POINTER(EvalScoreArgs), C.c_void_p]
    L.mgs_eval_view.restype = C.c_int32
    L.mgs_eval_view.argtypes = [C.POINTER(EvalViewArgs), C.c_void_p]
    for fn, cls in ((L.mgs_view_compose_args_size, ViewComposeArgs), (L.mgs_view_ellipsoid_args_size, ViewEllipsoidArgs),
                    (L.mgs_view_time_colors_args_size, ViewTimeColorsArgs),
                    (L.mgs_view_overlay_args_size, ViewOverlayArgs)):
        fn.restype, fn.argtypes = C.c_int32, []
        if fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    for fn in (L.mgs_view_compose_scratch_bytes, L.mgs_view_time_colors_scratch_bytes):
        fn.restype, fn.argtypes = C.c_uint64, []
    L.mgs_view_overlay_scratch_bytes.restype = C.c_uint64
    L.mgs_view_overlay_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    for fn, cls in ((L.mgs_view_compose, ViewComposeArgs), (L.mgs_view_ellipsoid, ViewEllipsoidArgs),
                    (L.mgs_view_time_colors, ViewTimeColorsArgs), (L.mgs_view_overlay, ViewOverlayArgs)):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    for size_fn, fn, cls in ((L.mgs_surface_args_size, L.mgs_surface_forward, SurfaceArgs),
                             (L.mgs_depth_normal_args_size, L.mgs_depth_normal, DepthNormalArgs)):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    for fn, cls in ((L.mgs_tsdf_integrate_args_size, TsdfIntegrateArgs), (L.mgs_tsdf_mesh_args_size, TsdfMeshArgs)):
        fn.restype, fn.argtypes = C.c_int32, []
        if fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    L.mgs_tsdf_mesh_scratch_bytes.restype = C.c_uint64
    L.mgs_tsdf_mesh_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mgs_tsdf_integrate.restype, L.mgs_tsdf_integrate.argtypes = C.c_int32, [C.POINTER(TsdfIntegrateArgs), C.c_void_p]
    for fn in (L.mgs_tsdf_mesh_count, L.mgs_tsdf_mesh_emit):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(TsdfMeshArgs), C.c_void_p]
    for fn, cls in ((L.mgs_sparse_tsdf_volume_size, SparseTsdfVolume), (L.mgs_sparse_tsdf_view_args_size, SparseTsdfViewArgs),
                    (L.mgs_sparse_tsdf_mesh_args_size, SparseTsdfMeshArgs)):
        fn.restype, fn.argtypes = C.c_int32, []
        if fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    for fn in (L.mgs_sparse_tsdf_table_size, L.mgs_sparse_tsdf_mesh_scratch_bytes):
        fn.restype, fn.argtypes = C.c_uint64, [C.c_int32]
    L.mgs_sparse_tsdf_allocate_scratch_bytes.restype = C.c_uint64
    L.mgs_sparse_tsdf_allocate_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    for fn in (L.mgs_sparse_tsdf_allocate, L.mgs_sparse_tsdf_integrate):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(SparseTsdfViewArgs), C.c_void_p]
    L.mgs_sparse_tsdf_register.restype = C.c_int32
    L.mgs_sparse_tsdf_register.argtypes = [C.POINTER(SparseTsdfVolume), C.c_int32, C.c_int32, C.c_void_p]
    for fn in (L.mgs_sparse_tsdf_mesh_count, L.mgs_sparse_tsdf_mesh_emit):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(SparseTsdfMeshArgs), C.c_void_p]
    for size_fn, cls, fn in ((L.mgs_tsdf_raycast_args_size, TsdfRaycastArgs, L.mgs_tsdf_raycast),
                             (L.mgs_sparse_tsdf_raycast_args_size, SparseTsdfRaycastArgs, L.mgs_sparse_tsdf_raycast),
                             (L.mgs_raycast_shade_args_size, RaycastShadeArgs, L.mgs_raycast_shade)):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} layout mismatch: library {size_fn()} bytes, ctypes {C.sizeof(cls)}")
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    L.mgs_sparse_tsdf_raycast_scratch_bytes.restype = C.c_uint64
    L.mgs_sparse_tsdf_raycast_scratch_bytes.argtypes = [C.c_int32]
    L.mgs_icp_args_size.restype, L.mgs_icp_args_size.argtypes = C.c_int32, []
    if L.mgs_icp_args_size() != C.sizeof(IcpArgs):
        raise NativeLibraryError("IcpArgs does not have the size of mgs_icp_args")
    L.mgs_icp_scratch_bytes.restype, L.mgs_icp_scratch_bytes.argtypes = C.c_uint64, [C.c_int32]
    L.mgs_icp_align.restype, L.mgs_icp_align.argtypes = C.c_int32, [C.POINTER(IcpArgs), C.c_void_p]
    for size, cls, fn in ((L.mgs_icp_intensity_args_size, IcpIntensityArgs, L.mgs_icp_intensity),
                          (L.mgs_icp_rgbd_args_size, IcpRgbdArgs, L.mgs_icp_align_rgbd)):
        size.restype, size.argtypes = C.c_int32, []
        if size() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    L.mgs_icp_rgbd_scratch_bytes.restype, L.mgs_icp_rgbd_scratch_bytes.argtypes = C.c_uint64, [C.c_int32]
    L.mgs_mesh_clean_args_size.restype, L.mgs_mesh_clean_args_size.argtypes = C.c_int32, []
    if L.mgs_mesh_clean_args_size() != C.sizeof(MeshCleanArgs):
        raise NativeLibraryError("MeshCleanArgs does not have the size of mgs_mesh_clean_args")
    L.mgs_mesh_clean_scratch_bytes.restype = C.c_uint64
    L.mgs_mesh_clean_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    for fn in (L.mgs_mesh_clean_count, L.mgs_mesh_clean_emit, L.mgs_mesh_components):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(MeshCleanArgs), C.c_void_p]
    for size_fn, cls in ((L.mgs_surface_sample_args_size, SurfaceSampleArgs), (L.mgs_nearest_args_size, NearestArgs),
                         (L.mgs_mesh_eval_args_size, MeshEvalArgs)):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    for fn in (L.mgs_surface_sample_scratch_bytes, L.mgs_nearest_scratch_bytes):
        fn.restype, fn.argtypes = C.c_uint64, [C.c_int32]
    L.mgs_mesh_eval_scratch_bytes.restype, L.mgs_mesh_eval_scratch_bytes.argtypes = C.c_uint64, []
    L.mgs_surface_sample.restype, L.mgs_surface_sample.argtypes = C.c_int32, [C.POINTER(SurfaceSampleArgs), C.c_void_p]
    L.mgs_nearest_distance.restype, L.mgs_nearest_distance.argtypes = C.c_int32, [C.POINTER(NearestArgs), C.c_void_p]
    for fn in (L.mgs_mesh_eval_stats, L.mgs_mesh_eval_finish):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(MeshEvalArgs), C.c_void_p]
    for size_fn, cls in ((L.mgs_mesh_render_args_size, MeshRenderArgs),
                         (L.mgs_vertex_visibility_args_size, VertexVisibilityArgs),
                         (L.mgs_mesh_cull_args_size, MeshCullArgs)):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
    L.mgs_mesh_render_scratch_bytes.restype = C.c_uint64
    L.mgs_mesh_render_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mgs_mesh_cull_scratch_bytes.restype, L.mgs_mesh_cull_scratch_bytes.argtypes = C.c_uint64, [C.c_int32, C.c_int32]
    L.mgs_mesh_render.restype, L.mgs_mesh_render.argtypes = C.c_int32, [C.POINTER(MeshRenderArgs), C.c_void_p]
    L.mgs_vertex_visibility.restype = C.c_int32
    L.mgs_vertex_visibility.argtypes = [C.POINTER(VertexVisibilityArgs), C.c_void_p]
    for fn in (L.mgs_mesh_cull_count, L.mgs_mesh_cull_emit):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(MeshCullArgs), C.c_void_p]
    for size_fn, cls, fns in ((L.mgs_mesh_normals_args_size, MeshNormalsArgs, (L.mgs_face_normals, L.mgs_vertex_normals)),
                              (L.mgs_mesh_eval_normal_args_size, MeshEvalNormalArgs,
                               (L.mgs_mesh_eval_normal_stats, L.mgs_mesh_eval_normal_finish)),
                              (L.mgs_mesh_shade_args_size, MeshShadeArgs, (L.mgs_mesh_shade,))):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
        for fn in fns:
            fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    L.mgs_vertex_normals_scratch_bytes.restype, L.mgs_vertex_normals_scratch_bytes.argtypes = C.c_uint64, [C.c_int32]
    L.mgs_mesh_eval_normal_scratch_bytes.restype, L.mgs_mesh_eval_normal_scratch_bytes.argtypes = C.c_uint64, []
    L.mgs_mesh_simplify_args_size.restype, L.mgs_mesh_simplify_args_size.argtypes = C.c_int32, []
    if L.mgs_mesh_simplify_args_size() != C.sizeof(MeshSimplifyArgs):
        raise NativeLibraryError("MeshSimplifyArgs does not have the size of mgs_mesh_simplify_args")
    L.mgs_mesh_simplify_scratch_bytes.restype = C.c_uint64
    L.mgs_mesh_simplify_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
    for fn in (L.mgs_mesh_simplify_count, L.mgs_mesh_simplify_emit):
        fn.restype, fn.argtypes = C.c_int32, [C.POINTER(MeshSimplifyArgs), C.c_void_p]
    for size_fn, cls, bytes_fn, fns in (
            (L.mgs_mesh_edges_args_size, MeshEdgesArgs, L.mgs_mesh_edges_scratch_bytes,
             (L.mgs_mesh_edges_count, L.mgs_mesh_edges_emit)),
            (L.mgs_mesh_smooth_args_size, MeshSmoothArgs, L.mgs_mesh_smooth_scratch_bytes, (L.mgs_mesh_smooth,))):
        size_fn.restype, size_fn.argtypes = C.c_int32, []
        if size_fn() != C.sizeof(cls):
            raise NativeLibraryError(f"{cls.__name__} does not have the size of its C struct")
        bytes_fn.restype, bytes_fn.argtypes = C.c_uint64, [C.c_int32, C.c_int32]
        for fn in fns:
            fn.restype, fn.argtypes = C.c_int32, [C.POINTER(cls), C.c_void_p]
    if L.mgs_abi_version() != ABI_VERSION:
        raise NativeLibraryError(
            f"ABI mismatch: library {L.mgs_abi_version()} vs binding {ABI_VERSION}")
    _lib = L
    return L


def struct_mirrors():
    """ctypes mirror of every argument struct, in mgs_struct_size() order."""
    return [RasterShape, WorkspaceSizes, ForwardArgs, BackwardArgs, PoseAdamArgs, MappingLossArgs,
            LMStepArgs, TrackingLossArgs, TrackingIterArgs, SketchResidualArgs, TrackingSOArgs,
            AdamGroup, MapPlanArgs, GatherTensor, MapGatherArgs, MapAccumArgs, MapActivateArgs,
            MappingViewArgs, MapFinishArgs, MapAppendArgs, SsimLossArgs, RefineViewArgs, TrackingDepthArgs,
            TrackingSampleArgs, KeyframeArgs, KeyframeSeedArgs]


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().mgs_status_string(status).decode()
        raise RuntimeError(f"{what} failed: {msg} (status {status})")


def workspace_sizes(shape: RasterShape) -> WorkspaceSizes:
    out = WorkspaceSizes()
    check(lib().mgs_raster_workspace_query(C.byref(shape), C.byref(out)),
          "mgs_raster_workspace_query")
    return out


def profile_enable(on: bool) -> None:
    check(lib().mgs_profile_enable(1 if on else 0), "mgs_profile_enable")


def profile_read(max_entries: int = 64) -> dict:
    """{kernel name: (total_ms, launches)} since the last read (synchronises)."""
    names = C.create_string_buffer(32 * max_entries)
    ms = (C.c_float * max_entries)()
    cnt = (C.c_int32 * max_entries)()
    n = lib().mgs_profile_read(max_entries, names, ms, cnt)
    if n < 0:
        check(n, "mgs_profile_read")
    out = {}
    for k in range(n):
        nm = names.raw[32 * k:32 * k + 32].split(b"\0", 1)[0].decode()
        out[nm] = (float(ms[k]), int(cnt[k]))
    return out
