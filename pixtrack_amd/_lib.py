"""ctypes binding of libpixtrack_hip.so (include/pixtrack_hip.h).

This is the whole Python<->native seam: plain pointers, sizes and a stream handle.
torch only supplies device memory (``tensor.data_ptr()``) and the current HIP stream.
There is NO fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

import torch

_HERE = Path(__file__).resolve().parent
# PIXTRACK_HIP_LIB points at another build of the same ABI (A/B experiments, packaging)
LIB_PATH = Path(os.environ["PIXTRACK_HIP_LIB"]) if os.environ.get("PIXTRACK_HIP_LIB") else _HERE / "libpixtrack_hip.so"

PXT_MAX_LEVELS = 8
PXT_LM_LOG_STRIDE = 20
PXT_E_TIMEOUT = -3
PXT_E_GUARD = -5
ABI_VERSION = 13
PXT_LM_MAX_BATCH = 16
PXT_UNET_MAX_BATCH = 16
PXT_NGP_MAX_BATCH = 16
PXT_LM_INFO_RECORD = 48
PXT_LM_INFO_MAX_PROBLEMS = 64
PXT_LM_POINT_RECORD = 8
PXT_LM_REPORT_SUMMARY = 16
PXT_LM_REPORT_MAX_PROBLEMS = 64
PXT_POSE_ERR_RECORD = 8
PXT_DEPTH_AGREE_MAX_TAUS = 16
PXT_DEPTH_AGREE_RECORD = 24
PXT_SYM_ERR_RECORD = 8
PXT_SYM_ERR_FRAME = 40
PXT_SYM_ERR_MAX_SYMS = 1024
PXT_SENSOR_VSD_MAX_TAUS = 16
PXT_SENSOR_VSD_RECORD = 32
PXT_DEPTH_MAX_POINTS = 4096
PXT_DEPTH_MAX_ITERS = 32
PXT_DEPTH_MAX_PROBLEMS = 16
PXT_DEPTH_RECORD = 32
PXT_DEPTH_LOG_STRIDE = 20
PXT_OCCLUSION_RECORD = 16
PXT_OCCLUSION_MAX_RADIUS = 16
PXT_OCCLUSION_MAX_VIEWS = 16
PXT_ISO_CASE_TABLE_WORDS = 6 * 16 * 7
PXT_MESH_VIEW = 20
PXT_MESH_RASTER_RECORD = 16
PXT_MESH_FRAME_MAX_VIEWS = 8
PXT_MESH_BATCH_MAX_MESHES = 16
PXT_MESH_BATCH_MAX_VIEWS = 32
PXT_MESH_SCENE_MAX_GROW = 8
PXT_MESH_VIEW_OUT = 24
PXT_POINTS_MAX_VIEWS = 16


class PxtError(RuntimeError):
    """Infrastructure failure of the native path (never a tracking failure)."""


class LmLevel(C.Structure):
    _fields_ = [
        ("fmap", C.c_void_p),
        ("fref", C.c_void_p),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("C", C.c_int32),
        ("cstride", C.c_int32),
        ("cam", C.c_float * 10),
        ("ndist", C.c_int32),
        ("lambda_", C.c_float * 6),
    ]


class LmTileGuard(C.Structure):
    _fields_ = [("level", C.c_int32), ("tile_flags", C.c_void_p), ("tile_rows", C.c_int32), ("tiles_per_row", C.c_int32),
                ("tile_x0", C.c_int32), ("tile_y0", C.c_int32)]


class LmConf(C.Structure):
    _fields_ = [
        ("num_iters", C.c_int32),
        ("pad", C.c_int32),
        ("loss", C.c_int32),
        ("loss_alpha", C.c_float),
        ("loss_scale", C.c_float),
        ("grad_stop", C.c_float),
        ("dt_stop", C.c_float),
        ("dR_stop", C.c_float),
        ("min_valid", C.c_int32),
        ("n_workgroups", C.c_int32),
        ("spin_limit", C.c_int32),
        ("path", C.c_int32),
    ]


class SampleLevel(C.Structure):
    _fields_ = [
        ("fmap", C.c_void_p),
        ("out", C.c_void_p),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("C", C.c_int32),
        ("cstride", C.c_int32),
        ("cam", C.c_float * 10),
        ("ndist", C.c_int32),
        ("x0", C.c_int32),
        ("y0", C.c_int32),
        ("full_w", C.c_int32),
        ("full_h", C.c_int32),
    ]


class UnetLayerView(C.Structure):
    _fields_ = [
        ("offset", C.c_int64),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("c", C.c_int32),
        ("in_memory", C.c_int32),
        ("cfg", C.c_int32),
        ("splits", C.c_int32),
        ("pool_fused", C.c_int32),
        ("decoder", C.c_int32),
        ("deep_ring", C.c_int32),
        ("reserved", C.c_int32),
    ]


class UnetSamplePoints(C.Structure):
    _fields_ = [
        ("p3d", C.c_void_p),
        ("n_points", C.c_int32),
        ("T", C.c_float * 12),
        ("cam", C.c_float * 10),
        ("ndist", C.c_int32),
        ("pad", C.c_int32),
        ("x0", C.c_int32),
        ("y0", C.c_int32),
        ("full_w", C.c_int32),
        ("full_h", C.c_int32),
    ]


class UnetQueryPoints(C.Structure):
    _fields_ = [("points", UnetSamplePoints), ("margin", C.c_int32)]


class NgpModel(C.Structure):
    _fields_ = [
        ("n_levels", C.c_int32),
        ("n_features", C.c_int32),
        ("log2_hashmap", C.c_int32),
        ("base_res", C.c_int32),
        ("per_level_scale", C.c_float),
        ("grid_cascades", C.c_int32),
        ("aabb_scale", C.c_float),
        ("cone_angle", C.c_float),
        ("depth_scale", C.c_float),
        ("linear_colors", C.c_int32),
    ]


class MeshDesc(C.Structure):
    """pxt_mesh_desc: one mesh of pxt_mesh_render_frame_batch (device pointers; colors, or uvs + triangle_uvs +
    texture)."""
    _fields_ = [
        ("vertices", C.c_void_p),
        ("triangles", C.c_void_p),
        ("colors", C.c_void_p),
        ("uvs", C.c_void_p),
        ("triangle_uvs", C.c_void_p),
        ("texture", C.c_void_p),
        ("n_vertices", C.c_int32),
        ("n_triangles", C.c_int32),
        ("n_uvs", C.c_int32),
        ("tex_width", C.c_int32),
        ("tex_height", C.c_int32),
        ("reserved", C.c_int32),
    ]


class MeshViewPose(C.Structure):
    """pxt_mesh_view_pose: where a view of pxt_mesh_render_frame_batch_posed takes its pose from (NULL: its host
    floats)."""
    _fields_ = [("pose_record", C.c_void_p), ("radius", C.c_double)]


class NgpView(C.Structure):
    _fields_ = [
        ("cam", C.c_float * 12),
        ("focal", C.c_float),
        ("k1", C.c_float),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
        ("background", C.c_float * 4),
        ("min_transmittance", C.c_float),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("spp", C.c_int32),
        ("mode", C.c_int32),
    ]


class NgpOutputs(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("depth_rgba", C.c_void_p), ("rgb_u8", C.c_void_p), ("depth_nz", C.c_void_p)]


class LmCamera(C.Structure):
    _fields_ = [("conv27", C.c_double * 27), ("cam_slot", C.c_void_p * 2), ("cam_out13", C.c_void_p)]


class LmProblem(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("point_mask", C.c_void_p), ("n_points", C.c_int32),
                ("levels_host", C.POINTER(LmLevel)), ("n_levels", C.c_int32), ("T_init_host", C.POINTER(C.c_float)),
                ("out", C.c_void_p), ("log", C.c_void_p), ("workspace", C.c_void_p), ("cam_host", C.POINTER(LmCamera))]


class LmInfoProblem(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("point_mask", C.c_void_p), ("n_points", C.c_int32), ("level", LmLevel),
                ("pose", C.c_void_p), ("pose_is_lm_record", C.c_int32), ("out", C.c_void_p)]


class LmReportProblem(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("point_mask", C.c_void_p), ("n_points", C.c_int32), ("level", LmLevel),
                ("pose", C.c_void_p), ("pose_is_lm_record", C.c_int32), ("inlier_weight", C.c_float),
                ("points", C.c_void_p), ("summary", C.c_void_p)]


class DepthConf(C.Structure):
    _fields_ = [("num_iters", C.c_int32), ("pad", C.c_int32), ("loss", C.c_int32), ("loss_alpha", C.c_float),
                ("loss_scale", C.c_float), ("lambda_", C.c_float * 6), ("max_residual", C.c_float),
                ("max_edge", C.c_float), ("grad_stop", C.c_float), ("dt_stop", C.c_float), ("dR_stop", C.c_float),
                ("min_valid", C.c_int32)]


class DepthProblem(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("point_mask", C.c_void_p), ("n_points", C.c_int32), ("sensor", C.c_void_p),
                ("width", C.c_int32), ("height", C.c_int32), ("sensor_scale", C.c_float), ("cam", C.c_float * 10),
                ("ndist", C.c_int32), ("pose", C.c_void_p), ("pose_is_lm_record", C.c_int32), ("prior", C.c_float * 21),
                ("out", C.c_void_p), ("log", C.c_void_p), ("codes", C.c_void_p)]


class OcclusionView(C.Structure):
    """pxt_occlusion_view: one image pair of pxt_occlusion_mask_views (device pointers)."""
    _fields_ = [("depth", C.c_void_p), ("sensor", C.c_void_p), ("mask_in", C.c_void_p), ("mask_out", C.c_void_p),
                ("occluder", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("shift_x", C.c_int32),
                ("shift_y", C.c_int32), ("sensor_q", C.c_float), ("delta_q", C.c_float)]


class IsoGrid(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("iso", C.c_float), ("origin", C.c_float * 3),
                ("spacing", C.c_float * 3)]


class RelocMap(C.Structure):
    _fields_ = [
        ("fmap", C.c_void_p),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("C", C.c_int32),
        ("cstride", C.c_int32),
        ("cam", C.c_float * 10),
        ("ndist", C.c_int32),
    ]


class RelocBank(C.Structure):
    _fields_ = [("p3d", C.c_void_p), ("fref", C.c_void_p), ("valid", C.c_void_p), ("n_points", C.c_int32)]


_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); every symbol include/pixtrack_hip.h declares.
_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
PROTOTYPES = {
    "pxt_version": (C.c_int, []),
    "pxt_last_error": (C.c_char_p, []),
    "pxt_device_cus": (C.c_int, [C.POINTER(C.c_int)]),
    "pxt_lm_refine": (
        C.c_int,
        [_VP, _VP, _I32, C.POINTER(LmLevel), _I32, _VP, C.POINTER(LmConf), _VP, _VP, _VP, _VP],
    ),
    "pxt_lm_refine_cam": (
        C.c_int,
        [_VP, _VP, _I32, C.POINTER(LmLevel), _I32, _VP, C.POINTER(LmConf), _VP, _VP, _VP, C.POINTER(LmCamera), _VP],
    ),
    "pxt_lm_refine_guarded": (
        C.c_int,
        [_VP, _VP, _I32, C.POINTER(LmLevel), _I32, _VP, C.POINTER(LmConf), _VP, _VP, _VP, C.POINTER(LmCamera),
         C.POINTER(LmTileGuard), _VP],
    ),
    "pxt_lm_workspace_bytes": (_I64, []),
    "pxt_lm_batch_workspace_bytes": (_I64, [_I32]),
    "pxt_lm_refine_batch": (C.c_int, [C.POINTER(LmProblem), _I32, C.POINTER(LmConf), _VP, _VP]),
    "pxt_lm_information_workspace_bytes": (_I64, [_I32]),
    "pxt_lm_information": (C.c_int, [C.POINTER(LmInfoProblem), _I32, C.POINTER(LmConf), _VP, _VP]),
    "pxt_lm_point_report_workspace_bytes": (_I64, [_I32]),
    "pxt_lm_point_report": (C.c_int, [C.POINTER(LmReportProblem), _I32, C.POINTER(LmConf), _VP, _VP]),
    "pxt_sample_sparse": (C.c_int, [_VP, _I32, _VP, C.POINTER(SampleLevel), _I32, _I32, _I32, _VP, _VP]),
    "pxt_score_pose_hypotheses": (
        C.c_int, [C.POINTER(RelocMap), C.POINTER(RelocBank), _VP, _VP, _I32, C.POINTER(LmConf), _VP, _VP]),
    "pxt_score_pose_hypotheses_depth": (
        C.c_int, [C.POINTER(RelocBank), _VP, _VP, _I32, _VP, _I32, _I32, C.c_float, C.c_float, C.POINTER(C.c_float),
                  _I32, _VP, _VP]),
    "pxt_unet_create": (C.c_int, [_VP, _I64, C.POINTER(_VP)]),
    "pxt_unet_create_f32": (C.c_int, [_VP, _I64, C.POINTER(_VP)]),
    "pxt_unet_precision": (C.c_int, [_VP]),
    "pxt_unet_destroy": (C.c_int, [_VP]),
    "pxt_unet_workspace_bytes": (_I64, [_VP, _I32, _I32]),
    "pxt_unet_forward": (
        C.c_int,
        [_VP, _VP, _I32, _VP, _I32, _I32, C.POINTER(_VP), C.POINTER(_I32), _I32, _VP, _VP],
    ),
    "pxt_unet_forward_sampled": (
        C.c_int,
        [_VP, _VP, _I32, _VP, _I32, _I32, C.POINTER(_VP), C.POINTER(_I32), _I32, _VP, _VP, C.POINTER(UnetSamplePoints)],
    ),
    "pxt_unet_forward_pair_sampled": (
        C.c_int,
        [_VP, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_VP),
         C.POINTER(_I32), C.POINTER(_I32), _VP, _VP, C.POINTER(C.POINTER(UnetSamplePoints))],
    ),
    "pxt_unet_set_reference_tiles": (C.c_int, [_VP, _I32]),
    "pxt_unet_reference_tiles_host": (C.c_int, [C.POINTER(UnetSamplePoints), _I32, _I32, _I32, _I32, _VP, _VP]),
    "pxt_unet_set_query_tiles": (C.c_int, [_VP, _I32]),
    "pxt_unet_query_tiles": (C.c_int, [_VP, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I64)]),
    "pxt_unet_query_tiles_host": (C.c_int, [C.POINTER(UnetQueryPoints), _I32, _I32, _I32, _I32, _VP, _VP]),
    "pxt_unet_forward_pair_tiles": (
        C.c_int,
        [_VP, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_VP),
         C.POINTER(_I32), C.POINTER(_I32), _VP, _VP, C.POINTER(UnetSamplePoints), C.POINTER(UnetQueryPoints)],
    ),
    "pxt_unet_forward_pair_second": (
        C.c_int,
        [_VP, _VP, _I32, _VP, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_VP), C.POINTER(_I32), _I32, _VP, _VP],
    ),
    "pxt_unet_set_defer_join": (C.c_int, [_VP, _I32]),
    "pxt_unet_set_batch_plan": (C.c_int, [_VP, _I32]),
    "pxt_unet_set_tile_skip": (C.c_int, [_VP, _I32]),
    "pxt_unet_pair_join": (C.c_int, [_VP, _VP]),
    "pxt_unet_activation_stats": (C.c_int, [_VP, _I32, _I32, _VP, _VP, _VP]),
    "pxt_unet_layer_views": (C.c_int, [_VP, _I32, _I32, _I32, _I32, C.POINTER(UnetLayerView)]),
    "pxt_unet_layer_views_f32": (C.c_int, [_VP, _I32, _I32, _I32, C.POINTER(UnetLayerView)]),
    "pxt_unet_workspace_bytes_batch": (_I64, [_VP, _I32, _I32, _I32]),
    "pxt_unet_forward_batch": (
        C.c_int,
        [_VP, _I32, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_VP), _I32, _I32, C.POINTER(_VP), C.POINTER(_I32),
         C.POINTER(_I32), _VP, _VP],
    ),
    "pxt_unet_workspace_bytes_pair": (_I64, [_VP, C.POINTER(_I32), C.POINTER(_I32)]),
    "pxt_unet_forward_pair": (
        C.c_int,
        [_VP, C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_VP), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_VP),
         C.POINTER(_I32), C.POINTER(_I32), _VP, _VP],
    ),
    "pxt_conv3x3_nhwc_f16": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _VP]),
    "pxt_conv3x3_nhwc_f32": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _VP]),
    "pxt_conv3x3_f32_cfg": (C.c_int, [_I32, _I32, _I32]),
    "pxt_conv3x3_nhwc_f32_cfg": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _I32, _VP]),
    "pxt_conv3x3_packed_bytes": (_I64, [_I32, _I32]),
    "pxt_conv3x3_pack_weights": (C.c_int, [_VP, _I32, _I32, _VP, _VP]),
    "pxt_conv3x3_packed": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _I64, _VP]),
    "pxt_conv3x3_upcat_packed": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _I32, _I32,
                                           _VP, _I64, _VP]),
    "pxt_ngp_create": (C.c_int, [C.POINTER(NgpModel), _VP, _I64, _VP, _I64, _VP, _I64, C.POINTER(_VP)]),
    "pxt_ngp_destroy": (C.c_int, [_VP]),
    "pxt_ngp_render": (C.c_int, [_VP, C.POINTER(NgpView), _VP, _VP, _VP]),
    "pxt_ngp_render_both": (C.c_int, [_VP, C.POINTER(NgpView), _VP, _VP, _VP, _VP]),
    "pxt_ngp_render_both_from_pose": (C.c_int, [_VP, C.POINTER(NgpView), _VP, C.POINTER(C.c_double), _VP, _VP, _VP, _VP, _VP]),
    "pxt_ngp_render_frame": (C.c_int, [_VP, C.POINTER(NgpView), _I32, _I32, C.POINTER(NgpOutputs), _VP, _VP]),
    "pxt_ngp_camera_slot": (_VP, [_VP]),
    "pxt_ngp_batch_workspace_bytes": (_I64, [_I32]),
    "pxt_ngp_render_frame_batch": (C.c_int, [C.POINTER(_VP), C.POINTER(NgpView), _I32, C.POINTER(_I32), _I32,
                                              C.POINTER(NgpOutputs), C.POINTER(_VP), _VP, _VP]),
    "pxt_ngp_create_shared": (C.c_int, [_VP, C.POINTER(_VP)]),
    "pxt_ngp_timing_enable": (C.c_int, [_VP, _I32]),
    "pxt_ngp_timing_read": (C.c_int, [_VP, C.POINTER(C.c_float), C.POINTER(_I32)]),
    "pxt_ngp_query": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP]),
    "pxt_depth_mask": (C.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "pxt_depth_mask_plane": (C.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "pxt_rgba_to_u8": (C.c_int, [_VP, _I32, _I32, C.c_float, _VP, _VP]),
    "pxt_resize_linear": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _I32, _VP]),
    "pxt_resize_activity": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _VP, _VP]),
    "pxt_points_from_depth_workspace_bytes": (_I64, [_I32, _I32]),
    "pxt_points_from_depth": (C.c_int, [_VP, _I32, _I32, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, _I32, _I32,
                                        _VP, _VP, _VP, _VP, _VP]),
    "pxt_points_from_depth_views_workspace_bytes": (_I64, [_I32, C.POINTER(_I32)]),
    "pxt_points_from_depth_views": (C.c_int, [C.POINTER(_VP), C.POINTER(_I32), C.POINTER(C.c_float), _I32, C.c_float, _I32,
                                              _I32, _VP, _VP, _VP, _VP, _VP]),
    "pxt_pose_errors_workspace_bytes": (_I64, [_I32, _I32]),
    "pxt_pose_errors": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _VP, _VP, _VP]),
    "pxt_depth_agreement_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "pxt_depth_agreement": (C.c_int, [_VP, _VP, _I32, _I32, _I32, C.c_float, C.POINTER(C.c_float), _I32, _VP, _VP, _VP]),
    "pxt_symmetric_pose_errors_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "pxt_symmetric_pose_errors": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _VP, _VP, _VP]),
    "pxt_sensor_vsd_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "pxt_sensor_vsd": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, C.c_float, C.c_float, C.c_float,
                                 C.POINTER(C.c_float), _I32, _VP, _VP, _VP]),
    "pxt_depth_refine_workspace_bytes": (_I64, [_I32]),
    "pxt_depth_refine": (C.c_int, [C.POINTER(DepthProblem), _I32, C.POINTER(DepthConf), _VP, _VP]),
    "pxt_occlusion_mask_workspace_bytes": (_I64, [_I32, _I32]),
    "pxt_occlusion_mask": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, C.c_float, C.c_float, C.c_float, _I32, _I32,
                                     _VP, _VP, _VP, _VP, _VP]),
    "pxt_occlusion_mask_views_workspace_bytes": (_I64, [_I32, C.POINTER(_I32)]),
    "pxt_occlusion_mask_views": (C.c_int, [C.POINTER(OcclusionView), _I32, C.c_float, _I32, _I32, _VP, _VP, _VP]),
    "pxt_points_visible": (C.c_int, [_VP, _VP, _I32, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32, _VP, _I32, _I32,
                                     _VP, _VP, _VP]),
    "pxt_mask_exclude": (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP, _VP]),
    "pxt_iso_case_table": (C.c_int, [C.POINTER(_I32)]),
    "pxt_iso_surface_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "pxt_iso_surface_count": (C.c_int, [_VP, C.POINTER(IsoGrid), _VP, _VP, _VP]),
    "pxt_iso_surface_emit": (C.c_int, [_VP, C.POINTER(IsoGrid), _VP, _VP, _I32, _VP, _VP, _I32, _VP]),
    "pxt_max_pairwise_distance_workspace_bytes": (_I64, [_I32]),
    "pxt_max_pairwise_distance": (C.c_int, [_VP, _I32, _VP, _VP, _VP]),
    "pxt_mesh_raster_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "pxt_mesh_raster": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "pxt_mesh_render": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pxt_mesh_render_textured": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _I32, _I32, _I32,
                                           _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pxt_mesh_render_frame_workspace_bytes": (_I64, [_I32, _I32, _VP]),
    "pxt_mesh_render_frame": (C.c_int, [_VP, _I32, _VP, _I32, _VP, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _I32, _VP, _VP,
                                        _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pxt_mesh_render_frame_batch_workspace_bytes": (_I64, [_I32, _VP, _I32, _VP, _VP]),
    "pxt_mesh_render_frame_batch": (C.c_int, [C.POINTER(MeshDesc), _I32, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP,
                                              _VP, _VP, _VP, _VP]),
    "pxt_mesh_render_frame_batch_posed": (C.c_int, [C.POINTER(MeshDesc), _I32, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP,
                                                    _VP, _VP, _VP, _VP, C.POINTER(MeshViewPose), _VP, _VP]),
    "pxt_mesh_render_scene_batch_workspace_bytes": (_I64, [_I32, _VP, _I32, _VP, _VP]),
    "pxt_mesh_render_scene_batch": (C.c_int, [C.POINTER(MeshDesc), _I32, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP,
                                              _VP, _VP, _I32, _VP, _I64, _VP, _VP, _VP, _VP]),
}


def lib() -> C.CDLL:
    """Loads the native library once; raises PxtError if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise PxtError(
            f"{LIB_PATH} not built. Run `python -m pixtrack_amd._build` (hipcc, gfx950). "
            "There is no CPU fallback for the product path."
        )
    L = C.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    missing = []
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            missing.append(name)  # calling it later raises AttributeError (loud, no fallback)
            continue
        fn.restype = res
        fn.argtypes = args
    L._pxt_missing = missing
    if L.pxt_version() != ABI_VERSION:
        raise PxtError(f"ABI mismatch: library {L.pxt_version()} != binding {ABI_VERSION}; rebuild")
    _lib = L
    return L


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().pxt_last_error().decode(errors="replace")
        raise PxtError(f"{what} failed with code {code}: {msg}")


def stream_ptr(device: torch.device) -> int:
    """The raw hipStream_t of torch's current stream on ``device``."""
    return int(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise PxtError(f"{name} must live on a ROCm device (got {t.device}); no CPU path exists")


def pose_floats(T) -> list:
    """The host floats (row-major R, then t) of a Pose / tensor / sequence; the op they go to checks that they are 12."""
    data = T.as12() if hasattr(T, "as12") else T
    if torch.is_tensor(data):
        data = data.detach().cpu().reshape(-1).tolist()
    return [float(x) for x in data]


def host_pose12(T) -> "C.Array":
    """`pose_floats` as a C array of exactly 12, for *_host arguments."""
    vals = pose_floats(T)
    assert len(vals) == 12
    return (C.c_float * 12)(*vals)


def dptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()
