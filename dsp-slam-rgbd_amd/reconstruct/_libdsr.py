"""ctypes binding of libdsr (include/dsr.h).

The library is the product path: there is no Python/PyTorch fallback.  If
``libdsr.so`` is missing or no gfx950 device is visible, every entry point
raises ``DsrError`` ("Use ctypes.CDLL, which releases the GIL
during a foreign call").
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
DEFAULT_LIB = os.path.join(_PKG, "csrc", "libdsr.so")

MAX_LAYERS = 16
CODE_LEN = 64
FAIL_REASONS = {0: "ok", 1: "sdf loss is NaN", 2: "fewer than 10 ray samples in the unit ball",
                3: "render loss is NaN (no render points)"}


class DsrError(RuntimeError):
    pass


FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)


class DecoderDesc(C.Structure):
    _fields_ = [("code_len", C.c_int), ("n_layers", C.c_int),
                ("out_dim", C.c_int * MAX_LAYERS), ("in_dim", C.c_int * MAX_LAYERS),
                ("latent_in", C.c_int), ("use_tanh", C.c_int), ("xyz_in_all", C.c_int),
                ("norm_mask", C.c_int)]


class OptimParams(C.Structure):
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("k4", C.c_float),
                ("b1", C.c_float), ("b2", C.c_float), ("lr", C.c_float), ("s_damp", C.c_float),
                ("num_iterations", C.c_int), ("code_len", C.c_int),
                ("num_depth_samples", C.c_int), ("cut_off", C.c_float),
                ("pose_only_iterations", C.c_int)]


class ObjectIn(C.Structure):
    _fields_ = [("t_cam_obj", C.c_float * 16), ("pts", FP), ("n_pts", C.c_int),
                ("rays", FP), ("n_rays", C.c_int), ("depth", FP), ("n_depth", C.c_int),
                ("code", FP), ("pose_is_obj_cam", C.c_int)]


class ViewIn(C.Structure):
    """dsr_view_in: one camera's observations of an object (dsr_reconstruct_views)."""
    _fields_ = [("t_view_ref", C.c_float * 16), ("pts", FP), ("n_pts", C.c_int),
                ("rays", FP), ("n_rays", C.c_int), ("depth", FP), ("n_depth", C.c_int)]


class ViewsObjectIn(C.Structure):
    """dsr_views_object_in: one object seen from n_views cameras, views[0] the reference view."""
    _fields_ = [("t_cam_obj", C.c_float * 16), ("code", FP), ("pose_is_obj_cam", C.c_int),
                ("n_views", C.c_int), ("views", C.POINTER(ViewIn))]


class ObjectOut(C.Structure):
    _fields_ = [("t_cam_obj", C.c_float * 16), ("code", C.c_float * CODE_LEN),
                ("loss", C.c_float), ("is_good", C.c_int), ("fail_reason", C.c_int),
                ("iters_done", C.c_int), ("n_valid_last", C.c_int), ("k_last", C.c_int)]


class PoseIn(C.Structure):
    _fields_ = [("t_co_se3", C.c_float * 16), ("scale", C.c_float), ("pts", FP), ("n_pts", C.c_int),
                ("code", FP)]


class Trace(C.Structure):
    _fields_ = [("H", FP), ("b", FP), ("dx", FP), ("loss", FP), ("sdf_loss", FP),
                ("render_loss", FP), ("n_valid", IP), ("k", IP), ("t_obj_cam", FP), ("z", FP),
                ("n_decoded", IP), ("n_refined", IP)]


ABI_VERSION = 12         # include/dsr.h DSR_ABI_VERSION
BATCH_GRAPH = 1          # include/dsr.h DSR_BATCH_GRAPH
GATHER_HOST, GATHER_RCCL = 0, 1   # include/dsr.h DSR_GATHER_* (dsr_reconstruct_multi_ex)


class Stats(C.Structure):
    _fields_ = [("fwd_ms", C.c_double), ("jac_ms", C.c_double), ("total_ms", C.c_double),
                ("fwd_points", C.c_int64), ("jac_points", C.c_int64),
                ("fwd_launches", C.c_int), ("jac_launches", C.c_int), ("inball_points", C.c_int64),
                ("lite", C.c_int), ("refine_launches", C.c_int), ("refine_ms", C.c_double),
                ("refine_points", C.c_int64), ("lite_max_err", C.c_double),
                ("lite_min_margin", C.c_double), ("jac_surface_points", C.c_int64),
                ("jac_render_points", C.c_int64), ("keep_masks", C.c_int),
                ("lite_audit_violations", C.c_int), ("lite_redo_objects", C.c_int),
                ("surface_in_exact", C.c_int), ("audit_points", C.c_int64),
                ("lite_broken_blocks", C.c_int), ("test_hooks", C.c_int),
                ("lite_eligible", C.c_int), ("audit", C.c_int), ("audit_shell", C.c_float),
                ("audit_log2", C.c_int), ("lite_margin0", C.c_float), ("lite_floor", C.c_float),
                ("lite_safety", C.c_float), ("graph_captures", C.c_int), ("graph_replays", C.c_int),
                ("n_groups", C.c_int), ("graph_mode", C.c_int), ("fwd_variant", C.c_int),
                ("jac_variant", C.c_int), ("lite_variant", C.c_int), ("split_ring", C.c_int),
                ("prescan", C.c_int)]


class DecoderInfo(C.Structure):
    """dsr_decoder_info: the decoder's load-time lite qualification (include/dsr.h)."""
    _fields_ = [("code_len", C.c_int), ("lite_eligible", C.c_int), ("lite_probe_ratio", C.c_double),
                ("lite_probe_max_err", C.c_double), ("lite_probe_max_err_all", C.c_double),
                ("probe_points", C.c_int), ("probe_codes", C.c_int), ("probe_ms", C.c_double)]

class MesherStats(C.Structure):
    """dsr_mesher_stats: the last dsr_mesher_run_batch call of a mesher (include/dsr.h)."""
    _fields_ = [("n_codes", C.c_int), ("n_passes", C.c_int), ("slots", C.c_int), ("sign_pass", C.c_int),
                ("margin", C.c_float), ("lite_tiles", C.c_int), ("all_tiles", C.c_int),
                ("exact_tiles", C.c_int), ("audit_tiles", C.c_int), ("redo_tiles", C.c_int),
                ("violations", C.c_int), ("redone_codes", C.c_int), ("lite_broken_blocks", C.c_int),
                ("test_hooks", C.c_int), ("max_lite_err", C.c_double), ("lite_ms", C.c_double),
                ("exact_ms", C.c_double), ("mc_ms", C.c_double)]


class Camera(C.Structure):
    """dsr_camera: a zero-skew pinhole; pixel (u, v) has the ray ((u-cx)/fx, (v-cy)/fy, 1)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float)]


class RenderParams(C.Structure):
    """dsr_render_params: zeros = defaults (hit_eps 1e-4, max_steps 48, damp 1, near 0.01)."""
    _fields_ = [("hit_eps", C.c_float), ("max_steps", C.c_int), ("damp", C.c_float), ("near", C.c_float),
                ("normals", C.c_int)]


class RenderObject(C.Structure):
    _fields_ = [("t_cam_obj", C.c_float * 16), ("code", FP)]


class RenderObjectOut(C.Structure):
    _fields_ = [("status", C.c_int), ("rect", C.c_int * 4), ("n_rays", C.c_int), ("n_ball", C.c_int),
                ("n_hit", C.c_int), ("n_unconverged", C.c_int), ("n_visible", C.c_int)]


class RenderStats(C.Structure):
    """dsr_render_stats: the last dsr_renderer_render call of a renderer (include/dsr.h)."""
    _fields_ = [("n_obj", C.c_int), ("n_passes", C.c_int), ("steps_run", C.c_int), ("decoded", C.c_longlong),
                ("max_live_last", C.c_int), ("setup_ms", C.c_double), ("march_ms", C.c_double),
                ("resolve_ms", C.c_double)]


RENDER_OK, RENDER_OFFSCREEN, RENDER_SKIP_NEAR = 0, 1, 2   # include/dsr.h DSR_RENDER_*


class SceneObject(C.Structure):
    """dsr_scene_object: the object->world Sim(3) (row-major) and the code of one map object."""
    _fields_ = [("t_world_obj", C.c_float * 16), ("code", FP)]


class SceneObjectOut(C.Structure):
    """dsr_scene_object_out: one object's record of a dsr_scene_query call (include/dsr.h)."""
    _fields_ = [("n_in", C.c_int), ("n_win", C.c_int), ("n_neg", C.c_int), ("n_nan", C.c_int),
                ("sum_sdf", C.c_double), ("sum_abs", C.c_double)]


class SceneStats(C.Structure):
    """dsr_scene_stats: the last dsr_scene_query call of a scene (include/dsr.h)."""
    _fields_ = [("n_obj", C.c_int), ("n_pts", C.c_int), ("n_passes", C.c_int), ("pairs", C.c_longlong),
                ("decoded", C.c_longlong), ("winners", C.c_longlong), ("bin_ms", C.c_double),
                ("decode_ms", C.c_double), ("resolve_ms", C.c_double), ("grad_ms", C.c_double)]


class FrameParams(C.Structure):
    """dsr_frame_params: every value is taken literally (dsr_frame_params_default fills the defaults)."""
    _fields_ = [("max_pts", C.c_int), ("max_bg", C.c_int), ("downsample", C.c_int), ("expand", C.c_int),
                ("min_mask_area", C.c_int), ("near", C.c_float), ("far", C.c_float)]


class FrameDet(C.Structure):
    """dsr_frame_det: a label of the instance image, an optional box (bbox[2] < bbox[0]: the mask's
    tight box) and the pose / code / pose_is_obj_cam of dsr_object_in."""
    _fields_ = [("label", C.c_int), ("bbox", C.c_int * 4), ("t_cam_obj", C.c_float * 16), ("code", FP),
                ("pose_is_obj_cam", C.c_int)]


class FrameDetOut(C.Structure):
    """dsr_frame_det_out: the ingest record of one detection."""
    _fields_ = [("status", C.c_int), ("n_mask", C.c_int), ("n_valid", C.c_int), ("n_pts", C.c_int),
                ("n_bg", C.c_int), ("box", C.c_int * 4), ("grid_h", C.c_int), ("grid_w", C.c_int)]


FRAME_OK, FRAME_NO_MASK, FRAME_SMALL_MASK, FRAME_NO_DEPTH = 0, 1, 2, 3   # include/dsr.h DSR_FRAME_*
FRAME_STATUS = {0: "ok", 1: "no pixel carries the label", 2: "mask of at most min_mask_area pixels",
                3: "no valid depth in the mask"}


class AssocParams(C.Structure):
    """dsr_assoc_params: every value is taken literally (dsr_assoc_params_default fills the defaults)."""
    _fields_ = [("inlier_tol", C.c_float), ("min_hits", C.c_int), ("min_pct", C.c_int)]


class AssocOut(C.Structure):
    """dsr_assoc_out: one detection's record of a dsr_scene_associate_* call (include/dsr.h)."""
    _fields_ = [("status", C.c_int), ("n_pts", C.c_int), ("obj", C.c_int), ("n_hit", C.c_int), ("n_in", C.c_int),
                ("n_neg", C.c_int), ("second", C.c_int), ("second_hit", C.c_int), ("ingest_status", C.c_int),
                ("n_mask", C.c_int), ("n_valid", C.c_int)]


ASSOC_MATCHED, ASSOC_NEW, ASSOC_NO_POINTS = 0, 1, 2   # include/dsr.h DSR_ASSOC_*


class FramePoseParams(C.Structure):
    """dsr_frame_pose_params: every value is taken literally (dsr_frame_pose_params_default fills the
    reference's constants)."""
    _fields_ = [("outlier_radius", C.c_float), ("lo_pct", C.c_int), ("hi_pct", C.c_int), ("box_margin", C.c_float),
                ("scale_factor", C.c_float), ("min_points", C.c_int), ("up", C.c_float * 3)]


class FramePoseOut(C.Structure):
    """dsr_frame_pose_out: the start-pose record of one detection."""
    _fields_ = [("status", C.c_int), ("n_in", C.c_int), ("n_near", C.c_int), ("n_kept", C.c_int),
                ("dims", C.c_double * 3), ("eig", C.c_double * 3), ("t_cam_obj", C.c_float * 16)]


FRAME_POSE_GIVEN, FRAME_POSE_CUBOID, FRAME_POSE_CUBOID_FLIPPED = 0, 1, 2   # include/dsr.h, the modes
# include/dsr.h DSR_FRAME_POSE_* statuses
FRAME_POSE_OK, FRAME_POSE_NOT_ASKED, FRAME_POSE_NO_INPUT, FRAME_POSE_FEW_POINTS, FRAME_POSE_DEGENERATE = 0, 1, 2, 3, 4
FRAME_POSE_STATUS = {0: "ok", 1: "not asked (the detection brought its pose)", 2: "no input (the ingest is not ok)",
                     3: "fewer than min_points points", 4: "degenerate cuboid (l == 0 or a non-finite value)"}


class LidarParams(C.Structure):
    """dsr_lidar_params: every value is taken literally (dsr_lidar_params_default fills the defaults)."""
    _fields_ = [("max_pts", C.c_int), ("max_bg", C.c_int), ("downsample", C.c_int), ("expand", C.c_int),
                ("min_mask_area", C.c_int), ("radius", C.c_float), ("box_margin", C.c_float)]


class LidarMask(C.Structure):
    """dsr_lidar_mask: a label of the instance image and an optional box (bbox[2] < bbox[0]: the
    mask's tight box)."""
    _fields_ = [("label", C.c_int), ("bbox", C.c_int * 4)]


class LidarDet(C.Structure):
    """dsr_lidar_det: a 3-D detector row (trans, size = (w, l, h), theta) and the code of dsr_object_in."""
    _fields_ = [("trans", C.c_float * 3), ("size", C.c_float * 3), ("theta", C.c_float), ("code", FP)]


class LidarDetOut(C.Structure):
    """dsr_lidar_det_out: the ingest record of one detection."""
    _fields_ = [("status", C.c_int), ("n_near", C.c_int), ("n_crop", C.c_int), ("n_pts", C.c_int),
                ("n_proj", C.c_int), ("mask", C.c_int), ("n_hits", C.c_int), ("n_mask_px", C.c_int),
                ("n_bg", C.c_int), ("box", C.c_int * 4), ("grid_h", C.c_int), ("grid_w", C.c_int),
                ("t_cam_obj", C.c_float * 16)]


LIDAR_MAX_MASKS = 256    # include/dsr.h DSR_LIDAR_MAX_MASKS
LIDAR_OK, LIDAR_BEHIND, LIDAR_NO_POINTS, LIDAR_NO_MATCH, LIDAR_SMALL_MASK = 0, 1, 2, 3, 4   # include/dsr.h DSR_LIDAR_*
LIDAR_STATUS = {0: "ok", 1: "behind the camera", 2: "no sweep point in the box",
                3: "no mask holds more than half of the projected points", 4: "mask of at most min_mask_area pixels"}


class TrackOut(C.Structure):
    """dsr_track_out: the record of one tracked object."""
    _fields_ = [("status", C.c_int), ("n_pts", C.c_int), ("n_inliers", C.c_int), ("n_near", C.c_int),
                ("n_crop", C.c_int)]


class TrackDet(C.Structure):
    """dsr_track_det: the map object's scale and, with ``pose_given``, the start pose of a detection
    tracked from a sweep or a depth image (a frame call needs the pose)."""
    _fields_ = [("scale", C.c_float), ("pose_given", C.c_int), ("t_co_se3", C.c_float * 16)]


TRACK_OK, TRACK_NO_POINTS, TRACK_NO_INLIERS = 0, 1, 2   # include/dsr.h DSR_TRACK_*
TRACK_STATUS = {0: "ok", 1: "no points", 2: "the inlier filter kept no point"}


#: dsr_batch_lite_diag record layout (csrc/dsr_dev.hpp: STD_*)
LITE_DIAG_FIELDS = ("broken_blocks", "recorded", "block", "wave", "counter", "target", "observed", "tile_iter",
                    "hw_id", "xcc_id", "polls", "real_ticks")
#: the counter index (``counter``) names the LiteStShared event counter that was waited on
LITE_DIAG_COUNTERS = ("ovf0", "ovf1", "cH0", "cH1", "cRlo", "cRhi", "cP", "cT0", "cT1", "cE", "broken")
LITE_DIAG_INTS = len(LITE_DIAG_FIELDS)


#: every function declared in include/dsr.h, with its ctypes signature
SIGNATURES = {
    "dsr_abi_version": (C.c_int, []),
    "dsr_device_count": (C.c_int, [IP]),
    "dsr_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "dsr_ctx_destroy": (C.c_int, [C.c_void_p]),
    "dsr_last_error": (C.c_char_p, [C.c_void_p]),
    "dsr_decoder_load": (C.c_int, [C.c_void_p, C.POINTER(DecoderDesc), FP, C.c_size_t,
                                   C.POINTER(C.c_void_p)]),
    "dsr_decoder_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dsr_decoder_info_get": (C.c_int, [C.c_void_p, C.POINTER(DecoderInfo)]),
    "dsr_reconstruct_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int,
                                        C.POINTER(ObjectIn), C.POINTER(ObjectOut),
                                        C.POINTER(Trace)]),
    "dsr_reconstruct_views": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int,
                                        C.POINTER(ViewsObjectIn), C.POINTER(ObjectOut),
                                        C.POINTER(Trace), IP, C.POINTER(Stats)]),
    "dsr_batch_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int,
                                   C.POINTER(ObjectIn), C.POINTER(C.c_void_p)]),
    "dsr_batch_run": (C.c_int, [C.c_void_p]),
    "dsr_batch_graph": (C.c_int, [C.c_void_p]),
    "dsr_batch_sync": (C.c_int, [C.c_void_p]),
    "dsr_batch_query": (C.c_int, [C.c_void_p]),
    "dsr_batch_download": (C.c_int, [C.c_void_p, C.POINTER(ObjectOut)]),
    "dsr_batch_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "dsr_batch_lite_diag": (C.c_int, [C.c_void_p, IP, C.c_int]),
    "dsr_batch_windows": (C.c_int, [C.c_void_p, IP, IP, IP]),
    "dsr_batch_destroy": (C.c_int, [C.c_void_p]),
    "dsr_batch_create_capacity": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "dsr_batch_refill": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ObjectIn)]),
    "dsr_sdf_eval": (C.c_int, [C.c_void_p, C.c_void_p, FP, FP, C.c_int, FP, FP]),
    "dsr_pose_only": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), FP, C.c_float,
                                FP, C.c_int, FP, FP]),
    "dsr_pose_only_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int,
                                      C.POINTER(PoseIn), FP]),
    "dsr_reconstruct_multi": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                        C.POINTER(OptimParams), C.c_int, C.POINTER(ObjectIn),
                                        C.POINTER(ObjectOut)]),
    "dsr_reconstruct_multi_ex": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                           C.POINTER(OptimParams), C.c_int, C.POINTER(ObjectIn),
                                           C.POINTER(ObjectOut), IP]),
    "dsr_gather_layout": (C.c_int, [C.c_int, C.POINTER(ObjectIn), C.c_int, C.c_int, IP, IP, IP]),
    "dsr_mesher_create": (C.c_int, [C.c_void_p, C.c_void_p, FP, C.c_int, C.POINTER(C.c_void_p)]),
    "dsr_mesher_run": (C.c_int, [C.c_void_p, FP, C.c_float, FP, C.c_int, IP, C.c_int, IP, IP]),
    "dsr_mesher_destroy": (C.c_int, [C.c_void_p]),
    "dsr_mesher_run_batch": (C.c_int, [C.c_void_p, C.c_int, FP, C.c_float, FP, C.c_int, IP, C.c_int, IP, IP]),
    "dsr_mesher_stats_get": (C.c_int, [C.c_void_p, C.POINTER(MesherStats)]),
    "dsr_mesher_peek": (C.c_int, [C.c_void_p, C.c_int, FP, FP, C.POINTER(C.c_ubyte)]),
    "dsr_mc_volume": (C.c_int, [C.c_void_p, FP, C.c_int, C.c_float, FP, C.c_int, IP, C.c_int, IP, IP]),
    "dsr_renderer_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Camera), C.POINTER(C.c_void_p)]),
    "dsr_renderer_render": (C.c_int, [C.c_void_p, C.POINTER(RenderParams), C.c_int, C.POINTER(RenderObject),
                                      FP, IP, FP, C.POINTER(RenderObjectOut)]),
    "dsr_renderer_stats_get": (C.c_int, [C.c_void_p, C.POINTER(RenderStats)]),
    "dsr_renderer_destroy": (C.c_int, [C.c_void_p]),
    "dsr_render_layout": (C.c_int, [C.POINTER(Camera), C.c_float, C.c_int, C.POINTER(RenderObject), IP, IP]),
    "dsr_scene_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "dsr_scene_set_objects": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SceneObject)]),
    "dsr_scene_query": (C.c_int, [C.c_void_p, C.c_int, FP, FP, IP, FP, C.POINTER(SceneObjectOut)]),
    "dsr_scene_peek": (C.c_int, [C.c_void_p, C.c_int, C.c_int, IP, FP, FP, IP]),
    "dsr_scene_stats_get": (C.c_int, [C.c_void_p, C.POINTER(SceneStats)]),
    "dsr_scene_destroy": (C.c_int, [C.c_void_p]),
    "dsr_scene_bin_host": (C.c_int, [C.c_int, C.POINTER(SceneObject), C.c_int, FP, C.c_int, C.c_int, IP, FP, IP,
                                     FP]),
    "dsr_frame_params_default": (C.c_int, [C.POINTER(FrameParams)]),
    "dsr_frame_inputs_host": (C.c_int, [C.POINTER(Camera), C.POINTER(FrameParams), FP, IP, C.c_int,
                                        C.POINTER(FrameDet), FP, FP, FP, C.POINTER(FrameDetOut)]),
    "dsr_frame_inputs": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams), FP, IP, C.c_int,
                                   C.POINTER(FrameDet), FP, FP, FP, C.POINTER(FrameDetOut)]),
    "dsr_batch_refill_frame": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams), FP, IP, C.c_int,
                                         C.POINTER(FrameDet)]),
    "dsr_batch_frame_info": (C.c_int, [C.c_void_p, C.POINTER(FrameDetOut)]),
    "dsr_frame_pose_params_default": (C.c_int, [C.POINTER(FramePoseParams)]),
    "dsr_frame_poses_host": (C.c_int, [C.POINTER(Camera), C.POINTER(FrameParams), C.POINTER(FramePoseParams), FP, IP,
                                       C.c_int, C.POINTER(FrameDet), IP, FP, FP, FP, C.POINTER(FrameDetOut),
                                       C.POINTER(FramePoseOut)]),
    "dsr_frame_poses": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams), C.POINTER(FramePoseParams),
                                  FP, IP, C.c_int, C.POINTER(FrameDet), IP, FP, FP, FP, C.POINTER(FrameDetOut),
                                  C.POINTER(FramePoseOut)]),
    "dsr_batch_refill_frame_poses": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams),
                                               C.POINTER(FramePoseParams), FP, IP, C.c_int, C.POINTER(FrameDet), IP]),
    "dsr_batch_frame_pose_info": (C.c_int, [C.c_void_p, C.POINTER(FramePoseOut)]),
    "dsr_lidar_params_default": (C.c_int, [C.POINTER(LidarParams)]),
    "dsr_lidar_inputs_host": (C.c_int, [C.POINTER(Camera), C.POINTER(LidarParams), FP, FP, C.c_int, C.c_int, IP,
                                        C.c_int, C.POINTER(LidarMask), C.c_int, C.POINTER(LidarDet), FP, FP, FP,
                                        C.POINTER(LidarDetOut)]),
    "dsr_lidar_inputs": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(LidarParams), FP, FP, C.c_int, C.c_int,
                                   IP, C.c_int, C.POINTER(LidarMask), C.c_int, C.POINTER(LidarDet), FP, FP, FP,
                                   C.POINTER(LidarDetOut)]),
    "dsr_batch_refill_lidar": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(LidarParams), FP, FP, C.c_int,
                                         C.c_int, IP, C.c_int, C.POINTER(LidarMask), C.c_int, C.POINTER(LidarDet)]),
    "dsr_batch_lidar_info": (C.c_int, [C.c_void_p, C.POINTER(LidarDetOut)]),
    "dsr_tracker_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimParams), C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p)]),
    "dsr_tracker_destroy": (C.c_int, [C.c_void_p]),
    "dsr_tracker_track": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(PoseIn)]),
    "dsr_tracker_track_lidar": (C.c_int, [C.c_void_p, C.POINTER(LidarParams), FP, FP, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(LidarDet), C.POINTER(TrackDet)]),
    "dsr_tracker_track_frame": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams), FP, IP, C.c_int,
                                          C.POINTER(FrameDet), C.POINTER(TrackDet)]),
    "dsr_tracker_query": (C.c_int, [C.c_void_p]),
    "dsr_tracker_download": (C.c_int, [C.c_void_p, FP, C.POINTER(TrackOut)]),
    "dsr_lidar_track_prep_host": (C.c_int, [C.POINTER(LidarParams), FP, C.c_int, C.POINTER(LidarDet), FP, FP]),
    "dsr_assoc_params_default": (C.c_int, [C.POINTER(AssocParams)]),
    "dsr_scene_associate_frame": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(FrameParams),
                                            C.POINTER(AssocParams), FP, FP, IP, C.c_int, IP, C.POINTER(AssocOut), IP]),
    "dsr_scene_associate_points": (C.c_int, [C.c_void_p, C.POINTER(AssocParams), FP, C.c_int, C.c_int, IP, FP,
                                             C.POINTER(AssocOut), IP]),
    "dsr_assoc_points_host": (C.c_int, [C.POINTER(Camera), C.POINTER(FrameParams), FP, FP, IP, C.c_int, IP, FP, IP,
                                        C.POINTER(FrameDetOut)]),
    "dsr_assoc_pick_host": (C.c_int, [C.POINTER(AssocParams), C.c_int, C.c_int, IP, IP, C.POINTER(AssocOut)]),
}

#: entry points added without an ABI number change: callers detect them by the symbol, so a
#: library of the same ABI number built before them still loads (A/B runs under DSR_LIB)
BY_SYMBOL = ("dsr_reconstruct_views", "dsr_renderer_create", "dsr_renderer_render", "dsr_renderer_stats_get",
             "dsr_renderer_destroy", "dsr_render_layout", "dsr_frame_params_default", "dsr_frame_inputs_host",
             "dsr_frame_inputs", "dsr_batch_refill_frame", "dsr_batch_frame_info", "dsr_scene_create",
             "dsr_scene_set_objects", "dsr_scene_query", "dsr_scene_peek", "dsr_scene_stats_get", "dsr_scene_destroy",
             "dsr_scene_bin_host", "dsr_frame_pose_params_default", "dsr_frame_poses_host", "dsr_frame_poses",
             "dsr_batch_refill_frame_poses", "dsr_batch_frame_pose_info", "dsr_lidar_params_default",
             "dsr_lidar_inputs_host", "dsr_lidar_inputs", "dsr_batch_refill_lidar", "dsr_batch_lidar_info",
             "dsr_tracker_create", "dsr_tracker_destroy", "dsr_tracker_track", "dsr_tracker_track_lidar",
             "dsr_tracker_query", "dsr_tracker_download", "dsr_lidar_track_prep_host", "dsr_tracker_track_frame",
             "dsr_assoc_params_default", "dsr_scene_associate_frame", "dsr_scene_associate_points",
             "dsr_assoc_points_host", "dsr_assoc_pick_host")

_lib = None
_lock = threading.RLock()       # re-entrant: Context.get holds it while load_library takes it


def lib_path() -> str:
    return os.environ.get("DSR_LIB", DEFAULT_LIB)


def load_library(path: str | None = None):
    """Load libdsr.so (once) and attach the ctypes signatures."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or lib_path()
        if not os.path.isfile(p):
            raise DsrError(f"libdsr not built: {p} is missing (run `make -C dsp-slam-rgbd_amd/csrc` "
                           "or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            if name in BY_SYMBOL and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.dsr_abi_version() != ABI_VERSION:
            raise DsrError("libdsr ABI version mismatch")
        if path is None:
            _lib = lib
        return lib


def fptr(a: np.ndarray | None):
    if a is None:
        return None
    return a.ctypes.data_as(FP)


def iptr(a: np.ndarray | None):
    if a is None:
        return None
    return a.ctypes.data_as(IP)


class Context:
    """One libdsr context per HIP device (dsr_ctx_create)."""

    _cache: dict[int, "Context"] = {}

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.dsr_ctx_create(int(device), C.byref(h))
        if rc != 0:
            msgs = {-3: "no HIP device visible", -4: "device is not gfx950 (MI355X)",
                    -2: "bad device index", -1: "HIP runtime error"}
            raise DsrError(f"dsr_ctx_create(device={device}) failed: {msgs.get(rc, rc)}")
        self.handle = h
        self.device = device

    @classmethod
    def get(cls, device: int | None = None) -> "Context":
        if device is None:
            device = int(os.environ.get("DSR_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        with _lock:            # one context per device even when threads race to create it
            if device not in cls._cache:
                cls._cache[device] = Context(device)
            return cls._cache[device]

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.dsr_last_error(self.handle)
            raise DsrError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def lite_diag(lib, handle):
    """The last run's staggered-lite-pass record (dsr_batch_lite_diag) as a dict."""
    rec = (C.c_int * LITE_DIAG_INTS)()
    rc = lib.dsr_batch_lite_diag(handle, rec, LITE_DIAG_INTS)
    if rc != 0:
        raise DsrError(f"dsr_batch_lite_diag failed ({rc})")
    v = list(rec)
    d = dict(zip(LITE_DIAG_FIELDS, v))
    if d["recorded"] and 0 <= d["counter"] < len(LITE_DIAG_COUNTERS):
        d["counter"] = LITE_DIAG_COUNTERS[d["counter"]]
    d["real_us"] = (d.pop("real_ticks") & 0xffffffff) / 100.0      # 100 MHz counter
    return d


def optim_params(cfg) -> OptimParams:
    """configs.optimizer block (optimizer.py:27-43) -> OptimParams."""
    jo = cfg["joint_optim"]
    po = cfg.get("pose_only_optim", {"num_iterations": 5}) if hasattr(cfg, "get") else \
        {"num_iterations": 5}
    return OptimParams(float(jo["k1"]), float(jo["k2"]), float(jo["k3"]), float(jo["k4"]),
                       float(jo["b1"]), float(jo["b2"]), float(jo["learning_rate"]),
                       float(jo["scale_damping"]), int(jo["num_iterations"]), int(cfg["code_len"]),
                       int(cfg["num_depth_samples"]), float(cfg["cut_off_threshold"]),
                       int(po["num_iterations"]))
