"""``torch.ops.pixtrack.*``: the C-ABI entry points of libpixtrack_hip.so (include/pixtrack_hip.h)
registered as ``torch.library`` custom ops on the ROCm device (dispatch key CUDA == HIP on a
ROCm build of torch).  This is the seam SURVEY.md 8(b) / BASELINE north_star ask for: Python host
code hands ``torch.Tensor``s to the ops, the op bodies are the only place where ctypes touches the
hot path (pointers, sizes, the current HIP stream).

Reference call sites the ops stand in for:
  lm_refine            pixloc BaseRefiner.refine_pose_using_features -> opt.run per level
                       (pixtrack/localization/pixloc_pose_refiners.py:255-262)
  lm_information       (no reference counterpart) the LM's normal equations at a given pose, K problems per launch
  lm_point_report      (opt-in) the per-point terms of one LM iteration at a given pose, K problems per launch: what
                       DebugTracker keeps of a refinement's points at debug >= 2 (pixtrack/localization/tracker.py:26-30)
  sample_sparse        PoseTrackerRefiner.interp_sparse_observations (:327-368, interpolator :351)
  score_pose_hypotheses  (no reference counterpart) M pose hypotheses scored in one launch (relocalizer.py)
  unet_forward_batch   self.model({"image": ...}) (pixtrack/localization/feature_extractor.py:48)
  ngp_render[_both]    testbed.render(w, h, spp, True) (pixtrack/visualization/run_vis_on_poses.py:51)
  depth_mask           get_mask morphology (pixtrack/pose_trackers/pixloc_tracker_r9.py:207-214)
  rgba_to_u8           get_nerf_image's alpha threshold / *255 / uint8 (run_vis_on_poses.py:52-54)
  resize_linear        pixloc resize(image, size, max, "linear") (feature_extractor.py:45)
  points_from_depth    (opt-in) stands in for the SfM points of the nearest mapping image as the points a frame is
                       refined on (pixloc_pose_refiners.py:282-290): a lattice of the Depth render, back-projected
  points_from_depth_views  (opt-in) the same from the depth planes a mesh template's frame call drew, up to 16 views of
                       different sizes in one chain of three launches (mesh_render.points_reference restates it)
  pose_errors          (opt-in) ADD / ADD-S of F frames against ground truth in one call: the per-frame loop of
                       notebooks/GetMetrics.ipynb (get_metrics) and evaluation.adds_distance
  depth_agreement      (opt-in, no reference counterpart) P pairs of Depth renders compared pixel by pixel: the counts
                       behind VSD, silhouette IoU and depth error of a run without a mesh (render_evaluation.py)
  symmetric_pose_errors  (opt-in, no reference counterpart) BOP's MSSD / MSPD of F frames over a set of S symmetry
                       transforms in one call: F * S * V transform-project-compare triples (evaluation.py, symmetry.py)
  sensor_vsd           (opt-in, no reference counterpart) P pairs of Depth renders compared with each other and with the
                       frames' sensor depth images: the counts behind BOP's occlusion-aware VSD and the visible
                       fraction (sensor_evaluation.py)
  depth_refine         (opt-in, no reference counterpart) K sensor-depth pose refinements in one launch, each started at
                       12 floats or at an lm_refine record read on the device (depth_refinement.py)
  occlusion_mask       (opt-in, no reference counterpart) get_mask's plane minus the pixels where the frame's sensor depth
                       image lies in front of the mask view's Depth render, opened and grown (occlusion.py)
  occlusion_mask_views (opt-in) occlusion_mask for up to 16 image pairs of different sizes in one chain of two
                       launches, each pair's outputs bit for bit the single call's: the mesh objects of one RGB-D frame
  points_visible       (opt-in, no reference counterpart) the LM's point mask minus the points that project onto that
                       occluder plane
  mesh_render_scene_batch  (opt-in, no reference counterpart) mesh_render_frame_batch for objects that share an image:
                       per view also the pixels where another tracked mesh of its scene lies in front, grown
  mask_exclude         (opt-in, no reference counterpart) a mask minus such an occluder plane
  mesh_render_frame_batch_posed  (opt-in, no reference counterpart) mesh_render_frame_batch whose views take their pose
                       on the device from the record of an lm_refine launch queued ahead of it (render-ahead for mesh
                       templates)

All ops are out-variants (they write into tensors the caller allocated and mutate nothing else), so
the caller decides buffer reuse.  Context handles (``pxt_unet*`` / ``pxt_ngp*``) travel as ints.
There is no CPU implementation: the ops are registered for the CUDA(HIP) key only, so a call with
CPU tensors fails in the dispatcher, and a missing library raises ``PxtError`` at first use.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import torch

from . import _lib

_NS = "pixtrack"
_DEF = torch.library.Library(_NS, "DEF")

SCHEMAS = {
    "lm_refine": (
        "(Tensor p3d, Tensor? point_mask, Tensor[] fmaps, Tensor[] frefs, int[] channels, float[] cameras, "
        "int[] ndist, float[] lambdas, float[] T_init, int num_iters, int pad, int loss, float loss_alpha, "
        "float loss_scale, float grad_stop, float dt_stop, float dR_stop, int min_valid, int n_workgroups, "
        "Tensor(a!) record, Tensor(b!) workspace, bool want_log, int spin_limit=0, float[]? cam_conv=None, "
        "int[]? cam_slots=None, Tensor(c!)? cam_out=None, int lm_path=0, int guard_level=-1, Tensor? guard_flags=None, "
        "int[]? guard_geo=None) -> ()"),
    # K problems in one persistent launch (pxt_lm_refine_batch): per-problem tensors as lists, per-level tensors and
    # records flattened problem-major (n_levels[k] entries each), conf shared; n_workgroups is per problem
    "lm_refine_batch": (
        "(Tensor[] p3d, Tensor?[] point_masks, int[] n_levels, Tensor[] fmaps, Tensor[] frefs, int[] channels, "
        "float[] cameras, int[] ndist, float[] lambdas, float[] T_init, int num_iters, int pad, int loss, float loss_alpha, "
        "float loss_scale, float grad_stop, float dt_stop, float dR_stop, int min_valid, int n_workgroups, "
        "Tensor(a!)[] records, Tensor(b!)[] workspaces, Tensor(c!) batch_workspace, bool want_log, int spin_limit=0, "
        "float[]? cam_conv=None, int[]? cam_slots=None, Tensor(d!)[]? cam_outs=None, int lm_path=0, "
        "int[]? cam_enabled=None) -> ()"),
    # K (points, level, pose) problems in one launch (pxt_lm_information): per problem p3d [N, 3], an optional uint8 mask,
    # the level's query map [h, w, cstride] and reference records [N, cstride], 10 camera floats, a pose tensor (device
    # or pinned host: 12 floats, or an lm_refine record when pose_is_lm_record) and a 48-float record (device or pinned)
    "lm_information": (
        "(Tensor[] p3d, Tensor?[] point_masks, Tensor[] fmaps, Tensor[] frefs, int[] channels, float[] cameras, "
        "int[] ndist, Tensor[] poses, bool pose_is_lm_record, int pad, int loss, float loss_alpha, float loss_scale, "
        "int min_valid, Tensor(a!)[] records, Tensor(b!) workspace) -> ()"),
    # K (points, level, pose) problems in one launch (pxt_lm_point_report): the arguments of lm_information, with per
    # problem the inlier threshold on rho', an optional device tensor [N, 8] of point records (None: summary only) and a
    # 16-float summary (device or pinned host)
    "lm_point_report": (
        "(Tensor[] p3d, Tensor?[] point_masks, Tensor[] fmaps, Tensor[] frefs, int[] channels, float[] cameras, "
        "int[] ndist, Tensor[] poses, bool pose_is_lm_record, int pad, int loss, float loss_alpha, float loss_scale, "
        "int min_valid, float[] inlier_weights, Tensor(a!)?[] points, Tensor(b!)[] summaries, Tensor(c!) workspace) -> ()"),
    "sample_sparse": (
        "(Tensor p3d, float[] T, Tensor[] fmaps, int[] channels, float[] cameras, int[] ndist, int pad, "
        "bool normalize, Tensor(a!)[] outs, Tensor(b!) valid, int[]? windows=None) -> ()"),
    # M pose hypotheses against one query map (pxt_score_pose_hypotheses): poses [M, 12], ranges [M, 2] int32 into the
    # bank (p3d [N, 3], fref [N, cstride], valid [N] uint8 or None), out [M, 4]
    "score_pose_hypotheses": (
        "(Tensor fmap, int channels, float[] camera, int ndist, Tensor p3d, Tensor fref, Tensor? valid, Tensor poses, "
        "Tensor ranges, int pad, int loss, float loss_alpha, float loss_scale, Tensor(a!) out) -> ()"),
    "unet_forward_batch": (
        "(int ctx, Tensor[] images, Tensor?[] masks, bool[] normalize, Tensor(a!)[] outs, Tensor(b!) workspace, "
        "Tensor? sample_p3d=None, float[]? sample_pose_camera=None, int[]? sample_ints=None, Tensor? second_p3d=None, "
        "float[]? second_pose_camera=None, int[]? second_ints=None) -> ()"),
    "ngp_render": (
        "(int ctx, float[] view, int width, int height, int spp, int mode, Tensor(a!) out, Tensor(b!)? stats) -> ()"),
    "ngp_render_both": (
        "(int ctx, float[] view, int width, int height, int spp, Tensor(a!) rgba, Tensor(b!) depth, "
        "Tensor(c!)? stats) -> ()"),
    "ngp_render_both_from_pose": (
        "(int ctx, float[] view, Tensor pose_record, float[] conv, int width, int height, int spp, int mode, "
        "Tensor(a!) rgba, Tensor(b!)? depth, Tensor(c!) cam_out, Tensor(d!)? stats) -> ()"),
    "ngp_render_frame": (
        "(int ctx, float[] view, int width, int height, int spp, int mode, bool camera_from_slot, Tensor(a!)? rgba, "
        "Tensor(b!)? depth, Tensor(c!)? rgb_u8, Tensor(d!)? depth_nz, Tensor(e!)? stats) -> ()"),
    # K renders of K different contexts as one chain of launches (pxt_ngp_render_frame_batch): views = K x 25 floats, sizes =
    # K x (width, height), modes = K x {0 Shade, 1 Depth, 2 both}; rgb_u8: one tensor per render whose mode is 0 / 2, in render
    # order; depth_nz: one per render whose mode is 1 / 2; depth_float (optional): the float32 [H, W, 4] Depth image of
    # every render whose mode is 1 / 2, in render order
    "ngp_render_frame_batch": (
        "(int[] ctxs, float[] views, int[] sizes, int spp, int[] modes, bool camera_from_slot, Tensor(a!)[] rgb_u8, "
        "Tensor(b!)[] depth_nz, Tensor(c!) workspace, Tensor(d!)[] stats, Tensor(e!)[]? depth_float=None) -> ()"),
    "depth_mask": "(Tensor depth_rgba, int n_erode, int n_dilate, Tensor(a!) mask, Tensor(b!) scratch) -> ()",
    "depth_mask_plane": "(Tensor depth_nz, int n_erode, int n_dilate, Tensor(a!) mask) -> ()",
    "rgba_to_u8": "(Tensor rgba, float alpha_thresh, Tensor(a!) out) -> ()",
    "resize_linear": "(Tensor src, Tensor(a!) dst) -> ()",
    "resize_activity": "(Tensor? mask, Tensor? image_u8, int H, int W, Tensor(a!) active) -> ()",
    "conv3x3_nhwc_f16": "(Tensor x, Tensor weight, Tensor bias, bool relu, Tensor(a!) out) -> ()",
    # depth [H, W, 4] of a Depth render -> p3d [n_max, 3], slot_valid uint8 [n_max], record int32 [4] (device or pinned):
    # {accepted pixels, stride, points, candidates}; xform = 12 floats [M | b] (pxt_points_from_depth)
    "points_from_depth": (
        "(Tensor depth, float[] xform, float focal, float depth_scale, float min_alpha, int erode, int n_max, "
        "Tensor(a!) p3d, Tensor(b!) slot_valid, Tensor(c!) record, Tensor(d!) workspace) -> ()"),
    # depth: K <= 16 planes [H_k, W_k, 4] of a mesh frame call, views = K x 20 floats (the records the planes were drawn
    # with) -> p3d [K, n_max, 3], slot_valid uint8 [K, n_max], record int32 [K, 4] (device or pinned): per view
    # {accepted pixels, stride, points, candidates} (pxt_points_from_depth_views); workspace: uint8,
    # pxt_points_from_depth_views_workspace_bytes(K, sizes)
    "points_from_depth_views": (
        "(Tensor[] depth, float[] views, float min_alpha, int erode, int n_max, Tensor(a!) p3d, Tensor(b!) slot_valid, "
        "Tensor(c!) record, Tensor(d!) workspace) -> ()"),
    # centred vertices [V, 3], rel_poses [F, 12] (evaluation.relative_poses) -> records [F, 8]: ADD, its max, ADD-S, its
    # max, V, 0, 0, status (pxt_pose_errors); workspace: uint8, pxt_pose_errors_workspace_bytes(F, V)
    "pose_errors": (
        "(Tensor vertices, Tensor rel_poses, bool want_adds, Tensor(a!) records, Tensor(b!) workspace) -> ()"),
    # depth_est, depth_gt [P, H, W, 4] (Depth renders; may be the same tensor), tq = 1..16 thresholds in units of
    # depth / alpha -> records int32 [P, 24] (the uint32 words of pxt_depth_agreement); workspace: uint8,
    # pxt_depth_agreement_workspace_bytes(P, W, H)
    "depth_agreement": (
        "(Tensor depth_est, Tensor depth_gt, float min_alpha, float[] tq, Tensor(a!) records, "
        "Tensor(b!) workspace) -> ()"),
    # centred vertices [V, 3], syms [S, 12] and frames [F, 40] (rel, est, gt, fx fy cx cy; evaluation.symmetric_frames)
    # -> records [F, 8]: MSSD, its symmetry, MSPD, its symmetry, V, S, 0, status (pxt_symmetric_pose_errors); workspace:
    # uint8, pxt_symmetric_pose_errors_workspace_bytes(F, S, V)
    "symmetric_pose_errors": (
        "(Tensor vertices, Tensor syms, Tensor frames, Tensor(a!) records, Tensor(b!) workspace) -> ()"),
    # depth_est, depth_gt [P, H, W, 4] (Depth renders), sensor [P, H, W] uint16 (or int16 holding the same bits) raw depth
    # counts, ray [H, W] float32 or None, shift = (shift_x, shift_y), tq = 1..16 thresholds in units of depth / alpha
    # -> records int32 [P, 32] (the uint32 words of pxt_sensor_vsd); workspace: uint8,
    # pxt_sensor_vsd_workspace_bytes(P, W, H)
    "sensor_vsd": (
        "(Tensor depth_est, Tensor depth_gt, Tensor sensor, Tensor? ray, int[] shift, float min_alpha, float sensor_q, "
        "float delta_q, float[] tq, Tensor(a!) records, Tensor(b!) workspace) -> ()"),
    # K sensor-depth refinements in one launch (pxt_depth_refine): per problem p3d [N, 3] (N <= 4096), an optional uint8
    # mask, the sensor image [H, W] uint16 (or int16 holding the same bits), its scale, 10 camera floats, a pose tensor
    # (device or pinned host: 12 floats, or an lm_refine record when pose_is_lm_record), 21 prior floats, a 32-float
    # record (device or pinned), an optional log [num_iters, 20] and optional codes uint8 [num_iters + 1, N]
    "depth_refine": (
        "(Tensor[] p3d, Tensor?[] point_masks, Tensor[] sensors, float[] sensor_scales, float[] cameras, int[] ndist, "
        "Tensor[] poses, bool pose_is_lm_record, float[] priors, int num_iters, int pad, int loss, float loss_alpha, "
        "float loss_scale, float[] lambdas, float max_residual, float max_edge, float grad_stop, float dt_stop, "
        "float dR_stop, int min_valid, Tensor(a!)[] records, Tensor(b!)?[] logs, Tensor(c!)?[] codes, "
        "Tensor(d!) workspace) -> ()"),
    # depth [H, W, 4] (a Depth render), sensor [H, W] uint16 (or int16 holding the same bits), the frame's plain mask
    # uint8 [H, W], shift = (shift_x, shift_y), radii = (r_open, r_grow) -> mask uint8 [H, W], occluder uint8 [H, W],
    # record int32 [16] (device or pinned); workspace: uint8, pxt_occlusion_mask_workspace_bytes(W, H)
    "occlusion_mask": (
        "(Tensor depth, Tensor sensor, Tensor mask_in, int[] shift, float min_alpha, float sensor_q, float delta_q, "
        "int[] radii, Tensor(a!) mask, Tensor(b!) occluder, Tensor(c!) record, Tensor(d!) workspace) -> ()"),
    # occlusion_mask for K <= 16 image pairs of different sizes in one chain of two launches (pxt_occlusion_mask_views):
    # per view depth [H_k, W_k, 4], sensor [H_k, W_k] (several views may name one tensor), the plain mask, shifts = K x
    # (shift_x, shift_y), quanta = K x (sensor_q, delta_q); min_alpha and radii hold for the call -> per view mask and
    # occluder, records int32 [K, 16] (device or pinned); workspace: uint8, pxt_occlusion_mask_views_workspace_bytes(K,
    # sizes).  View k's outputs are bit for bit occlusion_mask's on that pair alone
    "occlusion_mask_views": (
        "(Tensor[] depth, Tensor[] sensors, Tensor[] masks_in, int[] shifts, float min_alpha, float[] quanta, "
        "int[] radii, Tensor(a!)[] masks, Tensor(b!)[] occluders, Tensor(c!) records, Tensor(d!) workspace) -> ()"),
    # p3d [N, 3], an optional uint8 mask [N], 12 pose floats, the unscaled query camera (10 floats, ndist), the occluder
    # plane of occlusion_mask -> valid uint8 [N] and words 8..10 of the same record (pxt_points_visible)
    "points_visible": (
        "(Tensor p3d, Tensor? valid_in, float[] pose, float[] camera, int ndist, Tensor occluder, Tensor(a!) valid, "
        "Tensor(b!) record) -> ()"),
    # mask_in uint8 [H, W] minus an occluder plane uint8 [H, W] that another call made -> mask uint8 [H, W] (may be
    # mask_in) and words 0, 1 of record (int32, >= 2 words, device or pinned): n_mask_in, n_mask_out (pxt_mask_exclude)
    "mask_exclude": "(Tensor mask_in, Tensor occluder, Tensor(a!) mask, Tensor(b!) record) -> ()",
    # network query (pxt_ngp_query): pos, dir [n, 3] (ngp coordinates, unit view directions) -> out [n, 4] = (density
    # logit, r, g, b)
    "ngp_query": "(int ctx, Tensor pos, Tensor dir, Tensor(a!) out) -> ()",
    # values [nz, ny, nx] float32, grid = (iso, origin xyz, spacing xyz) -> counts int32 [2] (vertices, triangles; device
    # or pinned) and the per-point records in workspace: uint8, pxt_iso_surface_workspace_bytes(nx, ny, nz)
    "iso_surface_count": "(Tensor values, float[] grid, Tensor(a!) workspace, Tensor(b!) counts) -> ()",
    # the same values, grid and workspace -> vertices [n, 3] float32, normals the same or None, triangles [m, 3] int32,
    # n and m as iso_surface_count gave them
    "iso_surface_emit": (
        "(Tensor values, float[] grid, Tensor workspace, Tensor(a!) vertices, Tensor(b!)? normals, "
        "Tensor(c!) triangles) -> ()"),
    # points [n, 3] -> out int32 [4] (device or pinned): bits of float d, i, j, 1 (pxt_max_pairwise_distance); workspace:
    # uint8, pxt_max_pairwise_distance_workspace_bytes(n)
    "max_pairwise_distance": "(Tensor points, Tensor(a!) out, Tensor(b!) workspace) -> ()",
    # vertices [V, 3] float32, triangles [T, 3] int32, views [P, 20] float32 (mesh_render.view_record) -> depth
    # [P, H, W, 4] (a Depth render's layout), triangle_ids int32 [P, H, W] or None, records int32 [P, 16] (the uint32
    # words of pxt_mesh_raster); workspace: uint8, pxt_mesh_raster_workspace_bytes(P, T, W, H)
    "mesh_raster": (
        "(Tensor vertices, Tensor triangles, Tensor views, Tensor(a!) depth, Tensor(b!)? triangle_ids, "
        "Tensor(c!) records, Tensor(d!) workspace) -> ()"),
    # the same mesh with colors [V, 3] float32 (0..1) -> any of rgba [P, H, W, 4], rgb_u8 uint8 [P, H, W, 3], depth
    # [P, H, W, 4], depth_nz uint8 [P, H, W], triangle_ids int32 [P, H, W] (at least one; pxt_mesh_render), records
    # and workspace as mesh_raster.  width / height say the size: no output is mandatory
    "mesh_render": (
        "(Tensor vertices, Tensor triangles, Tensor colors, Tensor views, int width, int height, Tensor(a!)? rgba, "
        "Tensor(b!)? rgb_u8, Tensor(c!)? depth, Tensor(d!)? depth_nz, Tensor(e!)? triangle_ids, Tensor(f!) records, "
        "Tensor(g!) workspace) -> ()"),
    # the same with a texture map in place of the colours: uvs [n, 2] float32, triangle_uvs int32 [T, 3] (corner k of
    # triangle t uses uvs[triangle_uvs[t, k]]), texture uint8 [Ht, Wt, 4] (r g b and an ignored byte;
    # pxt_mesh_render_textured)
    "mesh_render_textured": (
        "(Tensor vertices, Tensor triangles, Tensor uvs, Tensor triangle_uvs, Tensor texture, Tensor views, int width, "
        "int height, Tensor(a!)? rgba, Tensor(b!)? rgb_u8, Tensor(c!)? depth, Tensor(d!)? depth_nz, "
        "Tensor(e!)? triangle_ids, Tensor(f!) records, Tensor(g!) workspace) -> ()"),
    # a tracker frame's views of one mesh in one call (pxt_mesh_render_frame): colors, or uvs + triangle_uvs + texture;
    # views [P, 20], P <= 8; geometry = P x (width, height, supersample in 1, 2, 4); offsets = P x (rgba, rgb_u8,
    # depth, depth_nz): the byte offset of the view's plane in the flat buffer of that name (rgba, depth: float32;
    # rgb_u8, depth_nz: uint8), -1 for an output the view does not ask for; records int32 [P, 16]; workspace: uint8,
    # pxt_mesh_render_frame_workspace_bytes(P, T, geometry)
    "mesh_render_frame": (
        "(Tensor vertices, Tensor triangles, Tensor? colors, Tensor? uvs, Tensor? triangle_uvs, Tensor? texture, "
        "Tensor views, int[] geometry, int[] offsets, Tensor(a!)? rgba, Tensor(b!)? rgb_u8, Tensor(c!)? depth, "
        "Tensor(d!)? depth_nz, Tensor(e!) records, Tensor(f!) workspace) -> ()"),
    # mesh_render_frame for views of up to 16 DIFFERENT meshes in one chain (pxt_mesh_render_frame_batch): one list
    # entry per mesh (colors[m], or uvs[m] + triangle_uvs[m] + texture[m]; the others None); view_mesh = the mesh of
    # each of the P <= 32 views; views: a CPU float32 [P, 20] tensor - the floats travel in the call's parameter record;
    # geometry, offsets, the four flat buffers and records as mesh_render_frame; workspace: uint8,
    # pxt_mesh_render_frame_batch_workspace_bytes(...), one per stream
    "mesh_render_frame_batch": (
        "(Tensor[] vertices, Tensor[] triangles, Tensor?[] colors, Tensor?[] uvs, Tensor?[] triangle_uvs, "
        "Tensor?[] texture, int[] view_mesh, Tensor views, int[] geometry, int[] offsets, Tensor(a!)? rgba, "
        "Tensor(b!)? rgb_u8, Tensor(c!)? depth, Tensor(d!)? depth_nz, Tensor(e!) records, Tensor(f!) workspace) -> ()"),
    # mesh_render_frame_batch whose views take their pose on the device (pxt_mesh_render_frame_batch_posed):
    # pose_records = per view None (the view is drawn from its 20 host floats) or the float32 output record of an LM
    # launch queued ahead on the same stream (>= 16 floats, device or pinned host memory: [0..11] the pose, [12] failed,
    # [13] status); radii = per view the mesh's radius (depth_q = 1 / (|t| + radius), ignored for an un-posed view);
    # views_out: None or float32 [P, 24], device or pinned host - the floats each posed view was drawn with and, stored
    # last, word 20 = 1.0 (the refinement succeeded) or -1.0.  Everything else as mesh_render_frame_batch, workspace
    # included
    "mesh_render_frame_batch_posed": (
        "(Tensor[] vertices, Tensor[] triangles, Tensor?[] colors, Tensor?[] uvs, Tensor?[] triangle_uvs, "
        "Tensor?[] texture, int[] view_mesh, Tensor views, int[] geometry, int[] offsets, Tensor?[] pose_records, "
        "float[] radii, Tensor(a!)? rgba, Tensor(b!)? rgb_u8, Tensor(c!)? depth, Tensor(d!)? depth_nz, "
        "Tensor(e!) records, Tensor(f!) workspace, Tensor(g!)? views_out) -> ()"),
    # mesh_render_frame_batch for objects that share an image (pxt_mesh_render_scene_batch): view_scene = the scene of
    # each view (-1: none; the views of one scene are one camera, supersample 1), occluder_offsets = the byte offset of
    # each view's uint8 [H, W] plane in the flat buffer occluder (a multiple of 4; -1: the view wants none) -> where
    # another member of the view's scene lies in front, grown by r_grow in 0..8; records words 10, 11 = hidden pixels,
    # occluder pixels.  Everything else as mesh_render_frame_batch, bit for bit; workspace:
    # pxt_mesh_render_scene_batch_workspace_bytes(...)
    "mesh_render_scene_batch": (
        "(Tensor[] vertices, Tensor[] triangles, Tensor?[] colors, Tensor?[] uvs, Tensor?[] triangle_uvs, "
        "Tensor?[] texture, int[] view_mesh, Tensor views, int[] geometry, int[] offsets, int[] view_scene, int r_grow, "
        "int[] occluder_offsets, Tensor(a!)? rgba, Tensor(b!)? rgb_u8, Tensor(c!)? depth, Tensor(d!)? depth_nz, "
        "Tensor(e!)? occluder, Tensor(f!) records, Tensor(g!) workspace) -> ()"),
}
for _name, _schema in SCHEMAS.items():
    _DEF.define(_name + _schema)

VIEW_FLOATS = 12 + 2 + 3 + 3 + 4 + 1  # cam 3x4, focal, k1, aabb_min, aabb_max, background, min_transmittance


def _stream(t: torch.Tensor) -> int:
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.PxtError(f"{what} must be a contiguous float32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    return t


# ------------------------------------------------------------------------------------------- LM
def _lm_refine(p3d, point_mask, fmaps, frefs, channels, cameras, ndist, lambdas, T_init, num_iters, pad, loss,
               loss_alpha, loss_scale, grad_stop, dt_stop, dR_stop, min_valid, n_workgroups, record, workspace,
               want_log, spin_limit=0, cam_conv=None, cam_slots=None, cam_out=None, lm_path=0, guard_level=-1,
               guard_flags=None, guard_geo=None):
    """``guard_level`` (index in execution order), ``guard_flags`` (uint8 device tensor) and ``guard_geo`` = [tile_rows,
    tiles_per_row, tile_x0, tile_y0]: that level's map holds data only in the tiles whose flag is 1
    (pxt_lm_tile_guard, pxt_lm_refine_guarded); a launch that reads another tile ends with status PXT_E_GUARD."""
    L = _lib.lib()
    n_levels = len(fmaps)
    if not (1 <= n_levels <= _lib.PXT_MAX_LEVELS) or len(frefs) != n_levels or len(channels) != n_levels:
        raise _lib.PxtError(f"lm_refine: {n_levels} levels (1..{_lib.PXT_MAX_LEVELS}), {len(frefs)} frefs, {len(channels)} channels")
    if len(cameras) != 10 * n_levels or len(lambdas) != 6 * n_levels or len(ndist) != n_levels or len(T_init) != 12:
        raise _lib.PxtError("lm_refine: cameras need 10, lambdas 6 floats per level, T_init 12 floats")
    _f32c(p3d, "p3d")
    n = int(p3d.shape[0])
    arr = (_lib.LmLevel * n_levels)()
    for i in range(n_levels):
        fm, fr = _f32c(fmaps[i], "fmap"), _f32c(frefs[i], "fref")
        h, w, cs = fm.shape
        if tuple(fr.shape) != (n, cs):
            raise _lib.PxtError(f"lm_refine: fref of level {i} is {tuple(fr.shape)}, expected {(n, cs)}")
        arr[i].fmap, arr[i].fref = fm.data_ptr(), fr.data_ptr()
        arr[i].h, arr[i].w, arr[i].C, arr[i].cstride = h, w, int(channels[i]), cs
        arr[i].cam[:] = cameras[10 * i:10 * i + 10]
        arr[i].ndist = int(ndist[i])
        arr[i].lambda_[:] = lambdas[6 * i:6 * i + 6]
    guard = None
    if guard_flags is not None:
        if guard_geo is None or len(guard_geo) != 4:
            raise _lib.PxtError("lm_refine: guard_geo holds tile_rows, tiles_per_row, tile_x0, tile_y0")
        gl, flags = guard_level, guard_flags
        tile_rows, tiles_per_row, tile_x0, tile_y0 = guard_geo
        if not (0 <= int(gl) < n_levels) or flags.dtype != torch.uint8 or not flags.is_cuda or not flags.is_contiguous():
            raise _lib.PxtError("lm_refine: tile_guard names a level and a contiguous uint8 device tensor of flags")
        rows = (int(tile_y0) + arr[int(gl)].h - 1) // max(int(tile_rows), 1) + 1
        if int(tile_rows) < 1 or flags.numel() < rows * int(tiles_per_row):
            raise _lib.PxtError(f"lm_refine: tile_guard needs {rows} x {int(tiles_per_row)} flags, got {flags.numel()}")
        guard = _lib.LmTileGuard()
        guard.level, guard.tile_flags = int(gl), flags.data_ptr()
        guard.tile_rows, guard.tiles_per_row, guard.tile_x0, guard.tile_y0 = (int(tile_rows), int(tiles_per_row),
                                                                              int(tile_x0), int(tile_y0))
    conf = _lib.LmConf()
    conf.num_iters, conf.pad, conf.loss = int(num_iters), int(pad), int(loss)
    conf.loss_alpha, conf.loss_scale = float(loss_alpha), float(loss_scale)
    conf.grad_stop, conf.dt_stop, conf.dR_stop = float(grad_stop), float(dt_stop), float(dR_stop)
    conf.min_valid, conf.n_workgroups, conf.spin_limit = int(min_valid), int(n_workgroups), int(spin_limit)
    conf.path = int(lm_path)
    nh = 16 + _lib.PXT_MAX_LEVELS
    need = nh + (n_levels * int(num_iters) * _lib.PXT_LM_LOG_STRIDE if want_log else 0)
    if record.dtype != torch.float32 or record.numel() < need or not record.is_contiguous():
        raise _lib.PxtError(f"lm_refine: record needs {need} contiguous float32 values")
    if not (record.is_cuda or record.is_pinned()):
        raise _lib.PxtError("lm_refine: record must be device memory or pinned host memory")
    if point_mask is not None and (point_mask.dtype != torch.uint8 or not point_mask.is_contiguous()):
        raise _lib.PxtError("lm_refine: point_mask must be contiguous uint8")
    base = record.data_ptr()
    T0 = (C.c_float * 12)(*[float(x) for x in T_init])
    cam = None
    if cam_conv is not None:  # the kernel's epilogue also derives the next render's camera (pxt_lm_refine_cam)
        if len(cam_conv) != 27:
            raise _lib.PxtError("lm_refine: cam_conv holds 27 doubles (Testbed.pose_conversion)")
        slots = [int(x) for x in (cam_slots or [])]
        if len(slots) > 2 or (not slots and cam_out is None):
            raise _lib.PxtError("lm_refine: at most two camera slots; at least one slot or cam_out")
        cam = _lib.LmCamera()
        cam.conv27[:] = [float(x) for x in cam_conv]
        for k in range(2):
            cam.cam_slot[k] = slots[k] if k < len(slots) and slots[k] else None
        cam.cam_out13 = None
        if cam_out is not None:
            if cam_out.dtype != torch.float32 or cam_out.numel() < 13 or not (cam_out.is_cuda or cam_out.is_pinned()):
                raise _lib.PxtError("lm_refine: cam_out must be a pinned host (or device) float32 tensor of >= 13 elements")
            cam.cam_out13 = cam_out.data_ptr()
        if guard is None:
            _lib.check(
                L.pxt_lm_refine_cam(p3d.data_ptr(), _lib.dptr(point_mask), n, arr, n_levels, T0, C.byref(conf), base,
                                    base + 4 * nh if want_log else None, workspace.data_ptr(), C.byref(cam), _stream(p3d)),
                "pxt_lm_refine_cam")
            return
    if guard is not None:
        _lib.check(
            L.pxt_lm_refine_guarded(p3d.data_ptr(), _lib.dptr(point_mask), n, arr, n_levels, T0, C.byref(conf), base,
                                    base + 4 * nh if want_log else None, workspace.data_ptr(),
                                    C.byref(cam) if cam is not None else None, C.byref(guard), _stream(p3d)),
            "pxt_lm_refine_guarded")
        return
    _lib.check(
        L.pxt_lm_refine(p3d.data_ptr(), _lib.dptr(point_mask), n, arr, n_levels, T0, C.byref(conf), base,
                        base + 4 * nh if want_log else None, workspace.data_ptr(), _stream(p3d)),
        "pxt_lm_refine")


def _lm_refine_batch(p3d, point_masks, n_levels, fmaps, frefs, channels, cameras, ndist, lambdas, T_init, num_iters, pad,
                     loss, loss_alpha, loss_scale, grad_stop, dt_stop, dR_stop, min_valid, n_workgroups, records,
                     workspaces, batch_workspace, want_log, spin_limit=0, cam_conv=None, cam_slots=None, cam_outs=None,
                     lm_path=0, cam_enabled=None):
    L = _lib.lib()
    K = len(p3d)
    n_levels = [int(x) for x in n_levels]
    nl_tot = sum(n_levels)
    if not (1 <= K <= _lib.PXT_LM_MAX_BATCH) or len(n_levels) != K or len(records) != K or len(workspaces) != K \
            or len(point_masks) != K or len(T_init) != 12 * K:
        raise _lib.PxtError(f"lm_refine_batch: {K} problems (1..{_lib.PXT_LM_MAX_BATCH}) need one record, workspace, mask slot "
                            "and 12 pose floats each")
    if len(fmaps) != nl_tot or len(frefs) != nl_tot or len(channels) != nl_tot or len(cameras) != 10 * nl_tot \
            or len(lambdas) != 6 * nl_tot or len(ndist) != nl_tot:
        raise _lib.PxtError("lm_refine_batch: per level one fmap, fref, channel count, ndist, 10 camera and 6 lambda floats")
    conf = _lib.LmConf()
    conf.num_iters, conf.pad, conf.loss = int(num_iters), int(pad), int(loss)
    conf.loss_alpha, conf.loss_scale = float(loss_alpha), float(loss_scale)
    conf.grad_stop, conf.dt_stop, conf.dR_stop = float(grad_stop), float(dt_stop), float(dR_stop)
    conf.min_valid, conf.n_workgroups, conf.spin_limit = int(min_valid), int(n_workgroups), int(spin_limit)
    conf.path = int(lm_path)
    nh = 16 + _lib.PXT_MAX_LEVELS
    if cam_conv is not None and (len(cam_conv) != 27 * K or len(cam_slots or []) != 2 * K
                                 or (cam_outs is not None and len(cam_outs) != K)):
        raise _lib.PxtError("lm_refine_batch: cam_conv holds 27 doubles, cam_slots 2 pointers (0 = none) per problem")
    probs = (_lib.LmProblem * K)()
    keep = []  # ctypes records the problem array points to
    li = 0
    for k in range(K):
        _f32c(p3d[k], "p3d")
        n = int(p3d[k].shape[0])
        nl = n_levels[k]
        if not (1 <= nl <= _lib.PXT_MAX_LEVELS):
            raise _lib.PxtError(f"lm_refine_batch: problem {k} has {nl} levels")
        arr = (_lib.LmLevel * nl)()
        for i in range(nl):
            fm, fr = _f32c(fmaps[li], "fmap"), _f32c(frefs[li], "fref")
            h, w, cs = fm.shape
            if tuple(fr.shape) != (n, cs):
                raise _lib.PxtError(f"lm_refine_batch: fref of problem {k} level {i} is {tuple(fr.shape)}, expected {(n, cs)}")
            arr[i].fmap, arr[i].fref = fm.data_ptr(), fr.data_ptr()
            arr[i].h, arr[i].w, arr[i].C, arr[i].cstride = h, w, int(channels[li]), cs
            arr[i].cam[:] = cameras[10 * li:10 * li + 10]
            arr[i].ndist = int(ndist[li])
            arr[i].lambda_[:] = lambdas[6 * li:6 * li + 6]
            li += 1
        rec = records[k]
        need = nh + (nl * int(num_iters) * _lib.PXT_LM_LOG_STRIDE if want_log else 0)
        if rec.dtype != torch.float32 or rec.numel() < need or not rec.is_contiguous() or not (rec.is_cuda or rec.is_pinned()):
            raise _lib.PxtError(f"lm_refine_batch: record {k} needs {need} contiguous float32 values in device or pinned memory")
        mk = point_masks[k]
        if mk is not None and (mk.dtype != torch.uint8 or not mk.is_contiguous() or mk.numel() != n):
            raise _lib.PxtError("lm_refine_batch: point masks are contiguous uint8 [n_points]")
        T0 = (C.c_float * 12)(*[float(x) for x in T_init[12 * k:12 * k + 12]])
        q = probs[k]
        q.p3d, q.point_mask, q.n_points = p3d[k].data_ptr(), _lib.dptr(mk), n
        q.levels_host, q.n_levels, q.T_init_host = arr, nl, T0
        q.out = rec.data_ptr()
        q.log = rec.data_ptr() + 4 * nh if want_log else None
        q.workspace = workspaces[k].data_ptr()
        cam = None
        if cam_conv is not None and (cam_enabled is None or cam_enabled[k]):
            cam = _lib.LmCamera()
            cam.conv27[:] = [float(x) for x in cam_conv[27 * k:27 * k + 27]]
            for j in range(2):
                cam.cam_slot[j] = int(cam_slots[2 * k + j]) or None
            cam.cam_out13 = None
            if cam_outs is not None:
                co = cam_outs[k]
                if co.dtype != torch.float32 or co.numel() < 13 or not (co.is_cuda or co.is_pinned()):
                    raise _lib.PxtError("lm_refine_batch: cam_outs are pinned host (or device) float32 tensors of >= 13 elements")
                cam.cam_out13 = co.data_ptr()
            q.cam_host = C.pointer(cam)
        keep.append((arr, T0, cam))
    if batch_workspace.numel() * batch_workspace.element_size() < int(L.pxt_lm_batch_workspace_bytes(K)):
        raise _lib.PxtError("lm_refine_batch: batch_workspace smaller than pxt_lm_batch_workspace_bytes(K)")
    _lib.check(L.pxt_lm_refine_batch(probs, K, C.byref(conf), batch_workspace.data_ptr(), _stream(p3d[0])),
               "pxt_lm_refine_batch")


def _lm_evaluate(op, problems, conf, records, workspace, *, entry, workspace_bytes, Problem, max_problems, record_name,
                 n_record, own, extras=(), extra_names=""):
    """The K (points, level, pose) problems of lm_information / lm_point_report: checked, packed and launched through
    ``entry``.  ``problems`` = the ops' common per-problem arguments in schema order (p3d ... pose_is_lm_record),
    ``conf`` = (pad, loss, loss_alpha, loss_scale, min_valid).  ``own(q, k, n)`` checks and sets what only ``op`` has
    (one list per problem in ``extras``, and the record's pointer) and returns the (tensor, name) pairs the kernel
    dereferences besides."""
    p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record = problems
    pad, loss, loss_alpha, loss_scale, min_valid = conf
    K = len(p3d)
    if not (1 <= K <= max_problems):
        raise _lib.PxtError(f"{op}: {K} problems (1..{max_problems})")
    if any(len(x) != K for x in (point_masks, fmaps, frefs, channels, ndist, poses, records, *extras)) \
            or len(cameras) != 10 * K:
        raise _lib.PxtError(f"{op}: per problem one mask slot, map, reference table, channel count, ndist, pose, "
                            f"{extra_names}{record_name} and 10 camera floats")
    _lib.require_gpu(workspace, "workspace")
    dev = workspace.device
    probs = (Problem * K)()
    for k in range(K):
        pts, fm, fr = _f32c(p3d[k], "p3d"), _f32c(fmaps[k], "fmap"), _f32c(frefs[k], "fref")
        n = int(pts.shape[0])
        if fm.dim() != 3 or tuple(pts.shape) != (n, 3) or tuple(fr.shape) != (n, int(fm.shape[2])):
            raise _lib.PxtError(f"{op}: problem {k}: p3d {tuple(pts.shape)}, fmap {tuple(fm.shape)}, fref "
                                f"{tuple(fr.shape)}; expected [N, 3], [h, w, cstride], [N, cstride]")
        mk = point_masks[k]
        if mk is not None and (mk.dtype != torch.uint8 or not mk.is_contiguous() or mk.numel() != n):
            raise _lib.PxtError(f"{op}: point masks are contiguous uint8 [n_points]")
        q = probs[k]
        more = own(q, k, n)
        # what the kernel dereferences must be device memory of one device (a host pointer there is a memory fault,
        # not an error); the pose and the record may also be pinned host memory
        for t, name in ((pts, "p3d"), (fm, "fmap"), (fr, "fref"), (mk, "point_mask"), *more):
            if t is None:
                continue
            _lib.require_gpu(t, name)
            if t.device != dev:
                raise _lib.PxtError(f"{op}: {name} of problem {k} is on {t.device}, the workspace on {dev}")
        need = 16 if pose_is_lm_record else 12
        for t, name, count in ((poses[k], "pose", need), (records[k], record_name, n_record)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < count \
                    or not ((t.is_cuda and t.device == dev) or t.is_pinned()):
                raise _lib.PxtError(f"{op}: {name} {k} needs {count} contiguous float32 values in device or pinned memory")
        q.p3d, q.point_mask, q.n_points = pts.data_ptr(), _lib.dptr(mk), n
        h, w, cs = (int(x) for x in fm.shape)
        q.level.fmap, q.level.fref = fm.data_ptr(), fr.data_ptr()
        q.level.h, q.level.w, q.level.C, q.level.cstride = h, w, int(channels[k]), cs
        q.level.cam[:] = [float(x) for x in cameras[10 * k:10 * k + 10]]
        q.level.ndist = int(ndist[k])
        q.pose, q.pose_is_lm_record = poses[k].data_ptr(), int(bool(pose_is_lm_record))
    if workspace.numel() * workspace.element_size() < int(workspace_bytes(K)):
        raise _lib.PxtError(f"{op}: workspace smaller than {workspace_bytes.__name__}(K)")
    conf = _lib.LmConf()
    conf.pad, conf.loss, conf.loss_alpha, conf.loss_scale = int(pad), int(loss), float(loss_alpha), float(loss_scale)
    conf.min_valid = int(min_valid)
    _lib.check(entry(probs, K, C.byref(conf), workspace.data_ptr(), _stream(workspace)), entry.__name__)


def _lm_information(p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record, pad, loss,
                    loss_alpha, loss_scale, min_valid, records, workspace):
    def own(q, k, n):
        q.out = records[k].data_ptr()
        return ()

    L = _lib.lib()
    _lm_evaluate("lm_information", (p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record),
                 (pad, loss, loss_alpha, loss_scale, min_valid), records, workspace, entry=L.pxt_lm_information,
                 workspace_bytes=L.pxt_lm_information_workspace_bytes, Problem=_lib.LmInfoProblem,
                 max_problems=_lib.PXT_LM_INFO_MAX_PROBLEMS, record_name="record", n_record=_lib.PXT_LM_INFO_RECORD, own=own)


def _lm_point_report(p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record, pad, loss,
                     loss_alpha, loss_scale, min_valid, inlier_weights, points, summaries, workspace):
    def own(q, k, n):
        out = points[k]
        if out is not None and (out.dtype != torch.float32 or not out.is_contiguous()
                                or tuple(out.shape) != (n, _lib.PXT_LM_POINT_RECORD)):
            raise _lib.PxtError(f"lm_point_report: points of problem {k} are a contiguous float32 [{n}, "
                                f"{_lib.PXT_LM_POINT_RECORD}] tensor (got {tuple(out.shape)}, {out.dtype})")
        q.inlier_weight, q.points, q.summary = float(inlier_weights[k]), _lib.dptr(out), summaries[k].data_ptr()
        return ((out, "points"),)

    L = _lib.lib()
    _lm_evaluate("lm_point_report", (p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record),
                 (pad, loss, loss_alpha, loss_scale, min_valid), summaries, workspace, entry=L.pxt_lm_point_report,
                 workspace_bytes=L.pxt_lm_point_report_workspace_bytes, Problem=_lib.LmReportProblem,
                 max_problems=_lib.PXT_LM_REPORT_MAX_PROBLEMS, record_name="summary", n_record=_lib.PXT_LM_REPORT_SUMMARY,
                 own=own, extras=(inlier_weights, points), extra_names="inlier weight, points slot, ")


# ------------------------------------------------------------------------------------ sampling
def _sample_sparse(p3d, T, fmaps, channels, cameras, ndist, pad, normalize, outs, valid, windows=None):
    L = _lib.lib()
    n_levels = len(fmaps)
    if len(outs) != n_levels or len(cameras) != 10 * n_levels or len(T) != 12:
        raise _lib.PxtError("sample_sparse: one out tensor and 10 camera floats per level, T of 12 floats")
    if windows is not None and len(windows) != 4 * n_levels:
        raise _lib.PxtError("sample_sparse: windows holds (x0, y0, full_w, full_h) per level")
    _f32c(p3d, "p3d")
    n = int(p3d.shape[0])
    arr = (_lib.SampleLevel * n_levels)()
    for i in range(n_levels):
        fm, out = _f32c(fmaps[i], "fmap"), _f32c(outs[i], "out")
        h, w, cs = fm.shape
        if tuple(out.shape) != (n, cs):
            raise _lib.PxtError(f"sample_sparse: out of level {i} is {tuple(out.shape)}, expected {(n, cs)}")
        arr[i].fmap, arr[i].out = fm.data_ptr(), out.data_ptr()
        arr[i].h, arr[i].w, arr[i].C, arr[i].cstride = h, w, int(channels[i]), cs
        arr[i].cam[:] = cameras[10 * i:10 * i + 10]
        arr[i].ndist = int(ndist[i])
        if windows is not None:  # (x0, y0, full_w, full_h) per level: the map is a window of the full level
            arr[i].x0, arr[i].y0, arr[i].full_w, arr[i].full_h = (int(x) for x in windows[4 * i:4 * i + 4])
    if valid.dtype != torch.uint8 or valid.numel() != n:
        raise _lib.PxtError("sample_sparse: valid must be uint8 [n_points]")
    T12 = (C.c_float * 12)(*[float(x) for x in T])
    _lib.check(L.pxt_sample_sparse(p3d.data_ptr(), n, T12, arr, n_levels, int(pad), int(bool(normalize)),
                                   valid.data_ptr(), _stream(p3d)), "pxt_sample_sparse")


# ------------------------------------------------------------------------------ relocalisation
def _score_pose_hypotheses(fmap, channels, camera, ndist, p3d, fref, valid, poses, ranges, pad, loss, loss_alpha, loss_scale,
                           out):
    L = _lib.lib()
    _f32c(fmap, "fmap")
    _f32c(p3d, "p3d")
    _f32c(fref, "fref")
    _f32c(poses, "poses")
    _f32c(out, "out")
    if fmap.dim() != 3 or len(camera) != 10:
        raise _lib.PxtError("score_pose_hypotheses: fmap is [h, w, cstride], camera 10 floats")
    h, w, cs = (int(x) for x in fmap.shape)
    n = int(p3d.shape[0])
    if tuple(p3d.shape) != (n, 3) or tuple(fref.shape) != (n, cs):
        raise _lib.PxtError(f"score_pose_hypotheses: p3d {tuple(p3d.shape)} / fref {tuple(fref.shape)}, expected "
                            f"{(n, 3)} / {(n, cs)}")
    if valid is not None and (valid.dtype != torch.uint8 or not valid.is_contiguous() or valid.numel() != n):
        raise _lib.PxtError("score_pose_hypotheses: valid must be contiguous uint8 [n_points]")
    M = int(poses.shape[0]) if poses.dim() == 2 else -1
    if M < 1 or tuple(poses.shape) != (M, 12):
        raise _lib.PxtError(f"score_pose_hypotheses: poses is {tuple(poses.shape)}, expected [M >= 1, 12]")
    if ranges.dtype != torch.int32 or not ranges.is_contiguous() or tuple(ranges.shape) != (M, 2):
        raise _lib.PxtError("score_pose_hypotheses: ranges must be contiguous int32 [M, 2]")
    if out.numel() != 4 * M:
        raise _lib.PxtError("score_pose_hypotheses: out holds 4 floats per hypothesis")
    # every buffer the kernel reads or writes must be device memory of the map's device (a host pointer in the kernel
    # would be a memory fault, not an error)
    for t, name in ((fmap, "fmap"), (p3d, "p3d"), (fref, "fref"), (valid, "valid"), (poses, "poses"), (ranges, "ranges"),
                    (out, "out")):
        if t is None:
            continue
        _lib.require_gpu(t, name)
        if t.device != fmap.device:
            raise _lib.PxtError(f"score_pose_hypotheses: {name} is on {t.device}, the map on {fmap.device}")
    mp = _lib.RelocMap()
    mp.fmap, mp.h, mp.w, mp.C, mp.cstride = fmap.data_ptr(), h, w, int(channels), cs
    mp.cam[:] = [float(x) for x in camera]
    mp.ndist = int(ndist)
    bank = _lib.RelocBank()
    bank.p3d, bank.fref, bank.valid, bank.n_points = p3d.data_ptr(), fref.data_ptr(), _lib.dptr(valid), n
    conf = _lib.LmConf()
    conf.pad, conf.loss, conf.loss_alpha, conf.loss_scale = int(pad), int(loss), float(loss_alpha), float(loss_scale)
    _lib.check(L.pxt_score_pose_hypotheses(C.byref(mp), C.byref(bank), poses.data_ptr(), ranges.data_ptr(), M, C.byref(conf),
                                           out.data_ptr(), _stream(fmap)), "pxt_score_pose_hypotheses")


# ---------------------------------------------------------------------------------------- UNet
def _unet_points(images, n, sample_p3d, sample_pose_camera, sample_ints):
    points = None
    if sample_p3d is not None:
        if n > 2 or sample_pose_camera is None or sample_ints is None or len(sample_pose_camera) != 22 or len(sample_ints) < 6:
            raise _lib.PxtError("unet_forward_batch: sample points go with one image or a pair, 22 floats (pose, camera) "
                                "and 6 ints (ndist, pad, x0, y0, full_w, full_h)")
        _f32c(sample_p3d, "sample_p3d")
        _lib.require_gpu(sample_p3d, "sample_p3d")
        if sample_p3d.dim() != 2 or sample_p3d.shape[1] != 3 or sample_p3d.device != images[0].device:
            raise _lib.PxtError("unet_forward_batch: sample_p3d is [N, 3] on the images' device")
        points = _lib.UnetSamplePoints()
        points.p3d, points.n_points = sample_p3d.data_ptr(), int(sample_p3d.shape[0])
        points.T[:] = [float(x) for x in sample_pose_camera[:12]]
        points.cam[:] = [float(x) for x in sample_pose_camera[12:]]
        points.ndist, points.pad, points.x0, points.y0, points.full_w, points.full_h = (int(x) for x in sample_ints[:6])
    return points


def _unet_forward_batch(ctx, images, masks, normalize, outs, workspace, sample_p3d=None, sample_pose_camera=None,
                        sample_ints=None, second_p3d=None, second_pose_camera=None, second_ints=None):
    """``sample_*`` (optional, one or two images): the points the FIRST image's fine map will be sampled at and nothing
    else will read it for (pxt_unet_sample_points: p3d [N, 3] on the device; 12 pose + 10 fine-level camera floats;
    ndist, pad, x0, y0, full_w, full_h) - the pass then computes only the fine tiles those samples
    depend on.  ``second_*`` (a pair only): the SECOND image's record as a QUERY (pxt_unet_query_points; second_ints holds
    a seventh value, the margin), whose flags the LM's tile guard reads afterwards (UNet.query_tiles)."""
    L = _lib.lib()
    n = len(images)
    points = _unet_points(images, n, sample_p3d, sample_pose_camera, sample_ints)
    second = None
    if second_p3d is not None:
        if n != 2:
            raise _lib.PxtError("unet_forward_batch: the second image's points go with a pair of images")
        if second_ints is None or len(second_ints) != 7:
            raise _lib.PxtError("unet_forward_batch: second_ints holds ndist, pad, x0, y0, full_w, full_h, margin")
        second = _lib.UnetQueryPoints()
        second.points = _unet_points(images, n, second_p3d, second_pose_camera, second_ints)
        second.margin = int(second_ints[6])
    if n == 0 or len(masks) != n or len(normalize) != n or len(outs) != 3 * n:
        raise _lib.PxtError("unet_forward_batch: per image one mask slot, one normalize flag and three output maps")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    H, W = sizes[0]
    # two images of different sizes (a frame's reference render and its query with real assets): two single-image
    # passes side by side (pxt_unet_forward_pair); any other batch holds images of one size
    pair = n == 2 and sizes[1] != sizes[0]
    for im, mk, hw in zip(images, masks, sizes):
        if im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous() or im.dtype not in (torch.float32, torch.uint8):
            raise _lib.PxtError("unet_forward_batch: images are contiguous HWC, 3 channels, float32 or uint8")
        if hw != (H, W) and not pair:
            raise _lib.PxtError("unet_forward_batch: a batch of more than two holds images of one size")
        if mk is not None and (mk.dtype != torch.uint8 or tuple(mk.shape) != hw or not mk.is_contiguous()):
            raise _lib.PxtError("unet_forward_batch: masks are contiguous uint8 [H, W]")
    Hs = (C.c_int32 * 2)(sizes[0][0], sizes[-1][0])
    Ws = (C.c_int32 * 2)(sizes[0][1], sizes[-1][1])
    need = int(L.pxt_unet_workspace_bytes_pair(ctx, Hs, Ws)) if pair else int(L.pxt_unet_workspace_bytes_batch(ctx, n, H, W))
    if need <= 0:
        raise _lib.PxtError(f"images {sizes} are not supported by the 4-level encoder")
    if workspace.numel() * workspace.element_size() < need:
        raise _lib.PxtError(f"unet_forward_batch: workspace holds {workspace.numel()} bytes, {need} needed")
    for o in outs:
        _f32c(o, "out map")
    imgs = (C.c_void_p * n)(*[im.data_ptr() for im in images])
    is_u8 = (C.c_int32 * n)(*[int(im.dtype == torch.uint8) for im in images])
    mks = (C.c_void_p * n)(*[_lib.dptr(m) for m in masks])
    norm = (C.c_int32 * n)(*[int(bool(x)) for x in normalize])
    ptrs = (C.c_void_p * (3 * n))(*[o.data_ptr() for o in outs])
    cs = (C.c_int32 * 3)(*[int(o.shape[2]) for o in outs[:3]])
    if points is not None and n == 1:
        _lib.check(L.pxt_unet_forward_sampled(ctx, imgs[0], is_u8[0], mks[0], H, W, ptrs, cs, norm[0], workspace.data_ptr(),
                                              _stream(images[0]), C.byref(points)), "pxt_unet_forward_sampled")
    elif second is not None:
        _lib.check(L.pxt_unet_forward_pair_tiles(ctx, imgs, is_u8, mks, Hs, Ws, ptrs, cs, norm, workspace.data_ptr(),
                                                 _stream(images[0]), C.byref(points) if points is not None else None,
                                                 C.byref(second)), "pxt_unet_forward_pair_tiles")
    elif points is not None:  # (equal sizes too: the two-image batch entry runs through the pair entry)
        pp = (C.POINTER(_lib.UnetSamplePoints) * 2)(C.pointer(points), None)
        _lib.check(L.pxt_unet_forward_pair_sampled(ctx, imgs, is_u8, mks, Hs, Ws, ptrs, cs, norm, workspace.data_ptr(),
                                                   _stream(images[0]), pp), "pxt_unet_forward_pair_sampled")
    elif pair:
        _lib.check(L.pxt_unet_forward_pair(ctx, imgs, is_u8, mks, Hs, Ws, ptrs, cs, norm, workspace.data_ptr(),
                                           _stream(images[0])), "pxt_unet_forward_pair")
    else:
        _lib.check(L.pxt_unet_forward_batch(ctx, n, imgs, is_u8, mks, H, W, ptrs, cs, norm, workspace.data_ptr(),
                                            _stream(images[0])), "pxt_unet_forward_batch")


def _conv3x3(x, weight, bias, relu, out):
    H, W, Cin = (int(s) for s in x.shape)
    Cout = int(weight.shape[0])
    _lib.check(_lib.lib().pxt_conv3x3_nhwc_f16(x.data_ptr(), H, W, Cin, weight.data_ptr(), bias.data_ptr(), Cout,
                                               int(bool(relu)), out.data_ptr(), _stream(x)), "pxt_conv3x3_nhwc_f16")


# ---------------------------------------------------------------------------------------- NeRF
def _view(view: Sequence[float], width, height, spp, mode) -> "_lib.NgpView":
    if len(view) != VIEW_FLOATS:
        raise _lib.PxtError(f"ngp view record has {len(view)} floats, expected {VIEW_FLOATS}")
    v = _lib.NgpView()
    v.cam[:] = view[0:12]
    v.focal, v.k1 = view[12], view[13]
    v.aabb_min[:] = view[14:17]
    v.aabb_max[:] = view[17:20]
    v.background[:] = view[20:24]
    v.min_transmittance = view[24]
    v.width, v.height, v.spp, v.mode = int(width), int(height), int(spp), int(mode)
    return v


def _check_frame(t: torch.Tensor, width, height, what):
    _f32c(t, what)
    if tuple(t.shape) != (height, width, 4):
        raise _lib.PxtError(f"{what} must be [{height}, {width}, 4] (got {tuple(t.shape)})")


def _ngp_render(ctx, view, width, height, spp, mode, out, stats):
    _check_frame(out, width, height, "out")
    v = _view(view, width, height, spp, mode)
    _lib.check(_lib.lib().pxt_ngp_render(ctx, C.byref(v), out.data_ptr(), _lib.dptr(stats), _stream(out)),
               "pxt_ngp_render")


def _ngp_render_both(ctx, view, width, height, spp, rgba, depth, stats):
    _check_frame(rgba, width, height, "rgba")
    _check_frame(depth, width, height, "depth")
    v = _view(view, width, height, spp, 0)
    _lib.check(_lib.lib().pxt_ngp_render_both(ctx, C.byref(v), rgba.data_ptr(), depth.data_ptr(), _lib.dptr(stats),
                                              _stream(rgba)), "pxt_ngp_render_both")


def _ngp_render_both_from_pose(ctx, view, pose_record, conv, width, height, spp, mode, rgba, depth, cam_out, stats):
    """pxt_ngp_render_both with the camera derived ON THE DEVICE from `pose_record` (pinned float32, >= 12 floats:
    the record pxt_lm_refine writes), so that the render can be enqueued behind the LM launch.  `cam_out`: pinned
    float32 [>= 13], receives the camera + a completion word.  `depth` given: Shade + Depth in one march (`mode`
    ignored); None: one render in `mode` (0 Shade, 1 Depth) into `rgba`."""
    _check_frame(rgba, width, height, "rgba")
    if depth is not None:
        _check_frame(depth, width, height, "depth")
    for t, n, what in ((pose_record, 12, "pose_record"), (cam_out, 13, "cam_out")):
        if t.dtype != torch.float32 or t.numel() < n or t.is_cuda or not t.is_pinned():
            raise _lib.PxtError(f"{what} must be a pinned host float32 tensor of >= {n} elements")
    if len(conv) != 27:
        raise _lib.PxtError("conv holds 27 doubles (nerf2sfm centroid, 3/avglen, R, totp, snapshot scale, offset)")
    v = _view(view, width, height, spp, int(mode) if depth is None else 0)
    cv = (C.c_double * 27)(*[float(x) for x in conv])
    _lib.check(_lib.lib().pxt_ngp_render_both_from_pose(ctx, C.byref(v), pose_record.data_ptr(), cv, cam_out.data_ptr(),
                                                        rgba.data_ptr(), _lib.dptr(depth), _lib.dptr(stats),
                                                        _stream(rgba)), "pxt_ngp_render_both_from_pose")


def _ngp_render_frame(ctx, view, width, height, spp, mode, camera_from_slot, rgba, depth, rgb_u8, depth_nz, stats):
    """pxt_ngp_render_frame: one render (mode 0 Shade / 1 Depth / 2 both in one march) whose last kernel also writes the
    8-bit planes the tracker consumes - `rgb_u8` uint8 [H, W, 3] (get_nerf_image's image), `depth_nz` uint8 [H, W]
    (get_mask's `uint8(depth * 255) != 0`) - so that the float images (`rgba`, `depth`) are optional; with
    `camera_from_slot` the camera comes from the context's slot (written by lm_refine's epilogue: cam_slots)."""
    width, height, mode = int(width), int(height), int(mode)
    if mode not in (0, 1, 2):
        raise _lib.PxtError("ngp_render_frame: mode is 0 (Shade), 1 (Depth) or 2 (both)")
    for t, what in ((rgba, "rgba"), (depth, "depth")):
        if t is not None:
            _check_frame(t, width, height, what)
    if rgb_u8 is not None and (rgb_u8.dtype != torch.uint8 or tuple(rgb_u8.shape) != (height, width, 3)
                               or not rgb_u8.is_contiguous() or not rgb_u8.is_cuda):
        raise _lib.PxtError("ngp_render_frame: rgb_u8 is a contiguous device uint8 [H, W, 3]")
    if depth_nz is not None and (depth_nz.dtype != torch.uint8 or tuple(depth_nz.shape) != (height, width)
                                 or not depth_nz.is_contiguous() or not depth_nz.is_cuda):
        raise _lib.PxtError("ngp_render_frame: depth_nz is a contiguous device uint8 [H, W]")
    ref = next((t for t in (rgba, depth, rgb_u8, depth_nz) if t is not None), None)
    if ref is None:
        raise _lib.PxtError("ngp_render_frame: no output")
    o = _lib.NgpOutputs(_lib.dptr(rgba), _lib.dptr(depth), _lib.dptr(rgb_u8), _lib.dptr(depth_nz))
    v = _view(view, width, height, spp, 0 if mode == 2 else mode)
    _lib.check(_lib.lib().pxt_ngp_render_frame(ctx, C.byref(v), mode, int(bool(camera_from_slot)), C.byref(o),
                                               _lib.dptr(stats), _stream(ref)), "pxt_ngp_render_frame")


def _ngp_render_frame_batch(ctxs, views, sizes, spp, modes, camera_from_slot, rgb_u8, depth_nz, workspace, stats,
                            depth_float=None):
    """pxt_ngp_render_frame_batch: K renders of K renderer contexts - a frame's Depth + Shade pair, or K objects in lock-step -
    as ONE staged chain of launches; bit for bit K calls of ngp_render_frame.  8-bit outputs only (what the tracker consumes)."""
    K, modes = len(ctxs), [int(m) for m in modes]
    if not (1 <= K <= _lib.PXT_NGP_MAX_BATCH) or len(views) != K * VIEW_FLOATS or len(sizes) != 2 * K or len(modes) != K:
        raise _lib.PxtError(f"ngp_render_frame_batch: {K} renders (1..{_lib.PXT_NGP_MAX_BATCH}) need {VIEW_FLOATS} view floats, "
                            "(width, height) and a mode each")
    if any(m not in (0, 1, 2) for m in modes):
        raise _lib.PxtError("ngp_render_frame_batch: a mode is 0 (Shade), 1 (Depth) or 2 (both)")
    if len(rgb_u8) != sum(m != 1 for m in modes) or len(depth_nz) != sum(m != 0 for m in modes):
        raise _lib.PxtError("ngp_render_frame_batch: one rgb_u8 per render of mode 0 / 2, one depth_nz per render of mode 1 / 2")
    if depth_float is not None and len(depth_float) != len(depth_nz):
        raise _lib.PxtError("ngp_render_frame_batch: depth_float holds one image per render of mode 1 / 2")
    L = _lib.lib()
    need = int(L.pxt_ngp_batch_workspace_bytes(K)) if K > 2 else 0  # (<= 2 renders: the records travel as kernel arguments)
    if workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"ngp_render_frame_batch: workspace is a contiguous device uint8 tensor of >= {need} bytes")
    if len(stats) not in (0, K) or any(t.dtype != torch.int64 or t.numel() < 4 or not t.is_contiguous() for t in stats):
        raise _lib.PxtError("ngp_render_frame_batch: stats is empty or one contiguous int64 [4] per render")
    vs = (_lib.NgpView * K)()
    outs = (_lib.NgpOutputs * K)()
    cp = (C.c_void_p * K)(*[int(c) for c in ctxs])
    mp = (C.c_int32 * K)(*modes)
    sp = (C.c_void_p * K)()
    i_u8 = i_nz = 0
    for k in range(K):
        w, h = int(sizes[2 * k]), int(sizes[2 * k + 1])
        vs[k] = _view(views[k * VIEW_FLOATS:(k + 1) * VIEW_FLOATS], w, h, spp, 0 if modes[k] == 2 else modes[k])
        u8 = nz = df = None
        if modes[k] != 1:
            u8, i_u8 = rgb_u8[i_u8], i_u8 + 1
        if modes[k] != 0:
            nz, i_nz = depth_nz[i_nz], i_nz + 1
            if depth_float is not None:
                df = depth_float[i_nz - 1]
                _check_frame(df, w, h, "depth_float")
                if df.device != workspace.device:
                    raise _lib.PxtError("ngp_render_frame_batch: depth_float lives on the workspace's device")
        if u8 is not None and (u8.dtype != torch.uint8 or tuple(u8.shape) != (h, w, 3) or not u8.is_contiguous()
                               or u8.device != workspace.device):
            raise _lib.PxtError("ngp_render_frame_batch: rgb_u8 is a contiguous device uint8 [H, W, 3]")
        if nz is not None and (nz.dtype != torch.uint8 or tuple(nz.shape) != (h, w) or not nz.is_contiguous()
                               or nz.device != workspace.device):
            raise _lib.PxtError("ngp_render_frame_batch: depth_nz is a contiguous device uint8 [H, W]")
        # (a Depth render writes its float image through `rgba`, a two-output march through `depth_rgba`)
        outs[k] = _lib.NgpOutputs(_lib.dptr(df) if modes[k] == 1 else None, _lib.dptr(df) if modes[k] == 2 else None,
                                  _lib.dptr(u8), _lib.dptr(nz))
        sp[k] = stats[k].data_ptr() if stats else None
    _lib.check(L.pxt_ngp_render_frame_batch(cp, vs, K, mp, int(bool(camera_from_slot)), outs,
                                            sp if stats else None, workspace.data_ptr() if workspace.numel() else None,
                                            _stream(workspace)),
               "pxt_ngp_render_frame_batch")


# ----------------------------------------------------------------------------------- image ops
def _mask_out(mask, H, W, like, what):
    """The output of the two mask entries: the kernels write it as a dense [H][W] byte plane on the input's device, and
    store four bytes as one dword when W % 4 == 0 (include/pixtrack_hip.h)."""
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
        raise _lib.PxtError(f"{what}: mask is uint8 [H, W]")
    if not mask.is_contiguous() or mask.device != like.device:
        raise _lib.PxtError(f"{what}: mask is contiguous and on the input's device (got strides {tuple(mask.stride())}, "
                            f"{mask.device} vs {like.device})")
    if W % 4 == 0 and mask.data_ptr() % 4 != 0:
        raise _lib.PxtError(f"{what}: mask must be 4-byte aligned when W % 4 == 0 (W = {W})")


def _depth_mask_plane(depth_nz, n_erode, n_dilate, mask):
    if depth_nz.dtype != torch.uint8 or depth_nz.dim() != 2 or not depth_nz.is_contiguous():
        raise _lib.PxtError("depth_mask_plane: depth_nz is a contiguous uint8 [H, W]")
    H, W = int(depth_nz.shape[0]), int(depth_nz.shape[1])
    _mask_out(mask, H, W, depth_nz, "depth_mask_plane")
    tmp = None
    if 2 * (int(n_erode) + int(n_dilate)) > 16:
        tmp = torch.empty(2 * H * W, dtype=torch.uint8, device=depth_nz.device)
    _lib.check(_lib.lib().pxt_depth_mask_plane(depth_nz.data_ptr(), H, W, int(n_erode), int(n_dilate), mask.data_ptr(),
                                               _lib.dptr(tmp), _stream(depth_nz)), "pxt_depth_mask_plane")


def _depth_mask(depth_rgba, n_erode, n_dilate, mask, scratch):
    _f32c(depth_rgba, "depth_rgba")
    H, W = int(depth_rgba.shape[0]), int(depth_rgba.shape[1])
    _mask_out(mask, H, W, depth_rgba, "depth_mask")
    if scratch.numel() < 2 * H * W:
        raise _lib.PxtError("depth_mask: scratch holds 2*H*W bytes")
    _lib.check(_lib.lib().pxt_depth_mask(depth_rgba.data_ptr(), H, W, int(n_erode), int(n_dilate), mask.data_ptr(),
                                         scratch.data_ptr(), _stream(depth_rgba)), "pxt_depth_mask")


def _rgba_to_u8(rgba, alpha_thresh, out):
    _f32c(rgba, "rgba")
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3):
        raise _lib.PxtError("rgba_to_u8: out is uint8 [H, W, 3]")
    _lib.check(_lib.lib().pxt_rgba_to_u8(rgba.data_ptr(), H, W, float(alpha_thresh), out.data_ptr(), _stream(rgba)),
               "pxt_rgba_to_u8")


def _resize_linear(src, dst):
    _f32c(src, "src")
    _f32c(dst, "dst")
    H, W, Cc = (int(s) for s in src.shape)
    Ho, Wo, Co = (int(s) for s in dst.shape)
    if Co != Cc:
        raise _lib.PxtError("resize_linear: channel counts differ")
    _lib.check(_lib.lib().pxt_resize_linear(src.data_ptr(), H, W, Cc, dst.data_ptr(), Ho, Wo, _stream(src)),
               "pxt_resize_linear")


def _resize_activity(mask, image_u8, H, W, active):
    if (mask is None) == (image_u8 is None):
        raise _lib.PxtError("resize_activity: exactly one of mask / image_u8")
    src = mask if mask is not None else image_u8
    if src.dtype != torch.uint8 or not src.is_contiguous() or active.dtype != torch.uint8 or not active.is_contiguous():
        raise _lib.PxtError("resize_activity: contiguous uint8 tensors")
    Ho, Wo = int(active.shape[0]), int(active.shape[1])
    _lib.check(_lib.lib().pxt_resize_activity(_lib.dptr(mask), _lib.dptr(image_u8), int(H), int(W), Ho, Wo, active.data_ptr(),
                                              _stream(active)), "pxt_resize_activity")


def _points_from_depth(depth, xform, focal, depth_scale, min_alpha, erode, n_max, p3d, slot_valid, record, workspace):
    L = _lib.lib()
    _f32c(depth, "depth")
    _f32c(p3d, "p3d")
    if depth.dim() != 3 or int(depth.shape[2]) != 4:
        raise _lib.PxtError(f"points_from_depth: depth is [H, W, 4] (got {tuple(depth.shape)})")
    H, W, n_max = int(depth.shape[0]), int(depth.shape[1]), int(n_max)
    if len(xform) != 12:
        raise _lib.PxtError("points_from_depth: xform holds 12 floats ([M | b], 3 x 4 row-major)")
    if int(erode) not in (0, 1, 2) or n_max < 1:
        raise _lib.PxtError("points_from_depth: erode is 0, 1 or 2 and n_max >= 1")
    if tuple(p3d.shape) != (n_max, 3):
        raise _lib.PxtError(f"points_from_depth: p3d is {tuple(p3d.shape)}, expected {(n_max, 3)}")
    if slot_valid.dtype != torch.uint8 or slot_valid.numel() != n_max or not slot_valid.is_contiguous():
        raise _lib.PxtError("points_from_depth: slot_valid is a contiguous uint8 [n_max]")
    if record.dtype != torch.int32 or record.numel() < 4 or not record.is_contiguous():
        raise _lib.PxtError("points_from_depth: record holds 4 contiguous int32 values")
    need = int(L.pxt_points_from_depth_workspace_bytes(W, H))
    if need <= 0:
        raise _lib.PxtError(f"points_from_depth: a {W} x {H} image is not supported")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"points_from_depth: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of the depth image's device (a host pointer there is a memory fault,
    # not an error); the record may also be pinned host memory
    for t, name in ((depth, "depth"), (p3d, "p3d"), (slot_valid, "slot_valid"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != depth.device:
            raise _lib.PxtError(f"points_from_depth: {name} is on {t.device}, the depth image on {depth.device}")
    if not ((record.is_cuda and record.device == depth.device) or record.is_pinned()):
        raise _lib.PxtError("points_from_depth: record must be memory of the depth image's device or pinned host memory")
    xf = (C.c_float * 12)(*[float(x) for x in xform])
    _lib.check(L.pxt_points_from_depth(depth.data_ptr(), W, H, xf, float(focal), float(depth_scale), float(min_alpha),
                                       int(erode), n_max, p3d.data_ptr(), slot_valid.data_ptr(), record.data_ptr(),
                                       workspace.data_ptr(), _stream(depth)), "pxt_points_from_depth")


def _points_from_depth_views(depth, views, min_alpha, erode, n_max, p3d, slot_valid, record, workspace):
    L = _lib.lib()
    what = "points_from_depth_views"
    K, n_max = len(depth), int(n_max)
    if not (1 <= K <= _lib.PXT_POINTS_MAX_VIEWS):
        raise _lib.PxtError(f"{what}: 1..{_lib.PXT_POINTS_MAX_VIEWS} depth planes (got {K})")
    sizes = []
    for k, d in enumerate(depth):
        _f32c(d, f"depth[{k}]")
        if d.dim() != 3 or int(d.shape[2]) != 4:
            raise _lib.PxtError(f"{what}: depth[{k}] is [H, W, 4] (got {tuple(d.shape)})")
        sizes += [int(d.shape[1]), int(d.shape[0])]
    _f32c(p3d, "p3d")
    if len(views) != K * _lib.PXT_MESH_VIEW:
        raise _lib.PxtError(f"{what}: views holds {_lib.PXT_MESH_VIEW} floats per plane ({K * _lib.PXT_MESH_VIEW}; got "
                            f"{len(views)})")
    if int(erode) not in (0, 1, 2) or n_max < 1:
        raise _lib.PxtError(f"{what}: erode is 0, 1 or 2 and n_max >= 1")
    if tuple(p3d.shape) != (K, n_max, 3):
        raise _lib.PxtError(f"{what}: p3d is {tuple(p3d.shape)}, expected {(K, n_max, 3)}")
    if slot_valid.dtype != torch.uint8 or tuple(slot_valid.shape) != (K, n_max) or not slot_valid.is_contiguous():
        raise _lib.PxtError(f"{what}: slot_valid is a contiguous uint8 [{K}, n_max]")
    if record.dtype != torch.int32 or tuple(record.shape) != (K, 4) or not record.is_contiguous():
        raise _lib.PxtError(f"{what}: record is a contiguous int32 [{K}, 4]")
    size_arr = (C.c_int32 * (2 * K))(*sizes)
    need = int(L.pxt_points_from_depth_views_workspace_bytes(K, size_arr))
    if need <= 0:
        raise _lib.PxtError(f"{what}: planes of {list(zip(sizes[0::2], sizes[1::2]))} are not supported")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of the depth planes' device (a host pointer there is a memory fault,
    # not an error); the record may also be pinned host memory
    device = depth[0].device
    named = [(d, f"depth[{k}]") for k, d in enumerate(depth)] + [(p3d, "p3d"), (slot_valid, "slot_valid"),
                                                                  (workspace, "workspace")]
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != device:
            raise _lib.PxtError(f"{what}: {name} is on {t.device}, depth[0] on {device}")
    if not ((record.is_cuda and record.device == device) or record.is_pinned()):
        raise _lib.PxtError(f"{what}: record must be memory of the depth planes' device or pinned host memory")
    planes = (C.c_void_p * K)(*[d.data_ptr() for d in depth])
    vf = (C.c_float * len(views))(*[float(x) for x in views])
    _lib.check(L.pxt_points_from_depth_views(planes, size_arr, vf, K, float(min_alpha), int(erode), n_max, p3d.data_ptr(),
                                             slot_valid.data_ptr(), record.data_ptr(), workspace.data_ptr(),
                                             _stream(depth[0])), "pxt_points_from_depth_views")


def _pose_errors(vertices, rel_poses, want_adds, records, workspace):
    L = _lib.lib()
    _f32c(vertices, "vertices")
    _f32c(rel_poses, "rel_poses")
    _f32c(records, "records")
    if vertices.dim() != 2 or int(vertices.shape[1]) != 3 or rel_poses.dim() != 2 or int(rel_poses.shape[1]) != 12:
        raise _lib.PxtError(f"pose_errors: vertices {tuple(vertices.shape)} / rel_poses {tuple(rel_poses.shape)}, expected "
                            "[V, 3] / [F, 12]")
    V, F = int(vertices.shape[0]), int(rel_poses.shape[0])
    if tuple(records.shape) != (F, _lib.PXT_POSE_ERR_RECORD):
        raise _lib.PxtError(f"pose_errors: records is {tuple(records.shape)}, expected {(F, _lib.PXT_POSE_ERR_RECORD)}")
    need = int(L.pxt_pose_errors_workspace_bytes(F, V))
    if need <= 0:
        raise _lib.PxtError(f"pose_errors: {F} frames x {V} vertices is not supported (1..65535 frames, 1..2^20 vertices)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"pose_errors: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    for t, name in ((vertices, "vertices"), (rel_poses, "rel_poses"), (records, "records"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != vertices.device:
            raise _lib.PxtError(f"pose_errors: {name} is on {t.device}, the vertices on {vertices.device}")
    _lib.check(L.pxt_pose_errors(vertices.data_ptr(), V, rel_poses.data_ptr(), F, int(bool(want_adds)), records.data_ptr(),
                                 workspace.data_ptr(), _stream(vertices)), "pxt_pose_errors")


def _depth_agreement(depth_est, depth_gt, min_alpha, tq, records, workspace):
    L = _lib.lib()
    _f32c(depth_est, "depth_est")
    _f32c(depth_gt, "depth_gt")
    if depth_est.dim() != 4 or int(depth_est.shape[3]) != 4 or tuple(depth_gt.shape) != tuple(depth_est.shape):
        raise _lib.PxtError(f"depth_agreement: depth_est {tuple(depth_est.shape)} / depth_gt {tuple(depth_gt.shape)}, "
                            "expected two [P, H, W, 4] tensors of one shape")
    P, H, W = (int(x) for x in depth_est.shape[:3])
    if not (1 <= len(tq) <= _lib.PXT_DEPTH_AGREE_MAX_TAUS):
        raise _lib.PxtError(f"depth_agreement: {len(tq)} thresholds (1..{_lib.PXT_DEPTH_AGREE_MAX_TAUS})")
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_DEPTH_AGREE_RECORD):
        raise _lib.PxtError(f"depth_agreement: records is a contiguous int32 [{P}, {_lib.PXT_DEPTH_AGREE_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    need = int(L.pxt_depth_agreement_workspace_bytes(P, W, H))
    if need <= 0:
        raise _lib.PxtError(f"depth_agreement: {P} pairs of {W} x {H} are not supported (1..65535 pairs, 1..2^28 pixels)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"depth_agreement: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    for t, name in ((depth_est, "depth_est"), (depth_gt, "depth_gt"), (records, "records"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != depth_est.device:
            raise _lib.PxtError(f"depth_agreement: {name} is on {t.device}, depth_est on {depth_est.device}")
    tqs = (C.c_float * len(tq))(*[float(x) for x in tq])
    _lib.check(L.pxt_depth_agreement(depth_est.data_ptr(), depth_gt.data_ptr(), P, W, H, float(min_alpha), tqs, len(tq),
                                     records.data_ptr(), workspace.data_ptr(), _stream(depth_est)), "pxt_depth_agreement")


def _symmetric_pose_errors(vertices, syms, frames, records, workspace):
    L = _lib.lib()
    _f32c(vertices, "vertices")
    _f32c(syms, "syms")
    _f32c(frames, "frames")
    _f32c(records, "records")
    if (vertices.dim() != 2 or int(vertices.shape[1]) != 3 or syms.dim() != 2 or int(syms.shape[1]) != 12
            or frames.dim() != 2 or int(frames.shape[1]) != _lib.PXT_SYM_ERR_FRAME):
        raise _lib.PxtError(f"symmetric_pose_errors: vertices {tuple(vertices.shape)} / syms {tuple(syms.shape)} / frames "
                            f"{tuple(frames.shape)}, expected [V, 3] / [S, 12] / [F, {_lib.PXT_SYM_ERR_FRAME}]")
    V, S, F = int(vertices.shape[0]), int(syms.shape[0]), int(frames.shape[0])
    if tuple(records.shape) != (F, _lib.PXT_SYM_ERR_RECORD):
        raise _lib.PxtError(f"symmetric_pose_errors: records is {tuple(records.shape)}, expected "
                            f"{(F, _lib.PXT_SYM_ERR_RECORD)}")
    need = int(L.pxt_symmetric_pose_errors_workspace_bytes(F, S, V))
    if need <= 0:
        raise _lib.PxtError(f"symmetric_pose_errors: {F} frames x {S} symmetries x {V} vertices is not supported "
                            f"(1..65535 frames, 1..{_lib.PXT_SYM_ERR_MAX_SYMS} symmetries, 1..2^20 vertices)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"symmetric_pose_errors: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    for t, name in ((vertices, "vertices"), (syms, "syms"), (frames, "frames"), (records, "records"),
                    (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != vertices.device:
            raise _lib.PxtError(f"symmetric_pose_errors: {name} is on {t.device}, the vertices on {vertices.device}")
    _lib.check(L.pxt_symmetric_pose_errors(vertices.data_ptr(), V, syms.data_ptr(), S, frames.data_ptr(), F,
                                           records.data_ptr(), workspace.data_ptr(), _stream(vertices)),
               "pxt_symmetric_pose_errors")


def _sensor_vsd(depth_est, depth_gt, sensor, ray, shift, min_alpha, sensor_q, delta_q, tq, records, workspace):
    L = _lib.lib()
    _f32c(depth_est, "depth_est")
    _f32c(depth_gt, "depth_gt")
    if depth_est.dim() != 4 or int(depth_est.shape[3]) != 4 or tuple(depth_gt.shape) != tuple(depth_est.shape):
        raise _lib.PxtError(f"sensor_vsd: depth_est {tuple(depth_est.shape)} / depth_gt {tuple(depth_gt.shape)}, "
                            "expected two [P, H, W, 4] tensors of one shape")
    P, H, W = (int(x) for x in depth_est.shape[:3])
    if sensor.dtype not in (torch.uint16, torch.int16) or not sensor.is_contiguous() or tuple(sensor.shape) != (P, H, W):
        raise _lib.PxtError(f"sensor_vsd: sensor is a contiguous uint16 (or int16) [{P}, {H}, {W}] tensor "
                            f"(got {tuple(sensor.shape)}, {sensor.dtype})")
    if ray is not None:
        _f32c(ray, "ray")
        if tuple(ray.shape) != (H, W):
            raise _lib.PxtError(f"sensor_vsd: ray is {tuple(ray.shape)}, expected {(H, W)}")
    if len(shift) != 2 or any(abs(int(v)) > 32767 for v in shift):
        raise _lib.PxtError(f"sensor_vsd: shift is (shift_x, shift_y), each within +-32767 (got {list(shift)})")
    if not (1 <= len(tq) <= _lib.PXT_SENSOR_VSD_MAX_TAUS):
        raise _lib.PxtError(f"sensor_vsd: {len(tq)} thresholds (1..{_lib.PXT_SENSOR_VSD_MAX_TAUS})")
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_SENSOR_VSD_RECORD):
        raise _lib.PxtError(f"sensor_vsd: records is a contiguous int32 [{P}, {_lib.PXT_SENSOR_VSD_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    need = int(L.pxt_sensor_vsd_workspace_bytes(P, W, H))
    if need <= 0:
        raise _lib.PxtError(f"sensor_vsd: {P} pairs of {W} x {H} are not supported (1..65535 pairs, 1..2^28 pixels)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"sensor_vsd: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    named = [(depth_est, "depth_est"), (depth_gt, "depth_gt"), (sensor, "sensor"), (records, "records"),
             (workspace, "workspace")] + ([(ray, "ray")] if ray is not None else [])
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != depth_est.device:
            raise _lib.PxtError(f"sensor_vsd: {name} is on {t.device}, depth_est on {depth_est.device}")
    tqs = (C.c_float * len(tq))(*[float(x) for x in tq])
    _lib.check(L.pxt_sensor_vsd(depth_est.data_ptr(), depth_gt.data_ptr(), sensor.data_ptr(),
                                None if ray is None else ray.data_ptr(), P, W, H, int(shift[0]), int(shift[1]),
                                float(min_alpha), float(sensor_q), float(delta_q), tqs, len(tq), records.data_ptr(),
                                workspace.data_ptr(), _stream(depth_est)), "pxt_sensor_vsd")


def _depth_refine(p3d, point_masks, sensors, sensor_scales, cameras, ndist, poses, pose_is_lm_record, priors, num_iters,
                  pad, loss, loss_alpha, loss_scale, lambdas, max_residual, max_edge, grad_stop, dt_stop, dR_stop,
                  min_valid, records, logs, codes, workspace):
    L = _lib.lib()
    K = len(p3d)
    if not (1 <= K <= _lib.PXT_DEPTH_MAX_PROBLEMS):
        raise _lib.PxtError(f"depth_refine: {K} problems (1..{_lib.PXT_DEPTH_MAX_PROBLEMS})")
    if any(len(x) != K for x in (point_masks, sensors, sensor_scales, ndist, poses, records, logs, codes)) \
            or len(cameras) != 10 * K or len(priors) != 21 * K or len(lambdas) != 6:
        raise _lib.PxtError("depth_refine: per problem one mask slot, sensor image, scale, ndist, pose, record, log slot, "
                            "codes slot, 10 camera floats and 21 prior floats; 6 lambdas")
    if not (0 <= int(num_iters) <= _lib.PXT_DEPTH_MAX_ITERS):
        raise _lib.PxtError(f"depth_refine: num_iters {num_iters} (0..{_lib.PXT_DEPTH_MAX_ITERS})")
    _lib.require_gpu(workspace, "workspace")
    dev = workspace.device
    rows = int(num_iters)
    probs = (_lib.DepthProblem * K)()
    for k in range(K):
        pts = _f32c(p3d[k], "p3d")
        n = int(pts.shape[0])
        if tuple(pts.shape) != (n, 3) or not (1 <= n <= _lib.PXT_DEPTH_MAX_POINTS):
            raise _lib.PxtError(f"depth_refine: problem {k}: p3d {tuple(pts.shape)}, expected [N, 3] with 1 <= N <= "
                                f"{_lib.PXT_DEPTH_MAX_POINTS}")
        mk, sen, lg, cd = point_masks[k], sensors[k], logs[k], codes[k]
        if mk is not None and (mk.dtype != torch.uint8 or not mk.is_contiguous() or mk.numel() != n):
            raise _lib.PxtError("depth_refine: point masks are contiguous uint8 [n_points]")
        if sen.dtype not in (torch.uint16, torch.int16) or not sen.is_contiguous() or sen.dim() != 2 \
                or min(int(x) for x in sen.shape) < 4:
            raise _lib.PxtError(f"depth_refine: sensor {k} is a contiguous uint16 (or int16) [H, W] tensor, H, W >= 4 "
                                f"(got {tuple(sen.shape)}, {sen.dtype})")
        if lg is not None and (lg.dtype != torch.float32 or not lg.is_contiguous()
                               or tuple(lg.shape) != (rows, _lib.PXT_DEPTH_LOG_STRIDE)):
            raise _lib.PxtError(f"depth_refine: log {k} is a contiguous float32 [{rows}, {_lib.PXT_DEPTH_LOG_STRIDE}] tensor")
        if cd is not None and (cd.dtype != torch.uint8 or not cd.is_contiguous() or tuple(cd.shape) != (rows + 1, n)):
            raise _lib.PxtError(f"depth_refine: codes {k} is a contiguous uint8 [{rows + 1}, {n}] tensor")
        # what the kernel dereferences must be device memory of one device (a host pointer there is a memory fault,
        # not an error); the pose, the record and the log may also be pinned host memory
        for t, name in ((pts, "p3d"), (mk, "point_mask"), (sen, "sensor"), (cd, "codes")):
            if t is None:
                continue
            _lib.require_gpu(t, name)
            if t.device != dev:
                raise _lib.PxtError(f"depth_refine: {name} of problem {k} is on {t.device}, the workspace on {dev}")
        need = 16 if pose_is_lm_record else 12
        for t, name, count in ((poses[k], "pose", need), (records[k], "record", _lib.PXT_DEPTH_RECORD), (lg, "log", 0)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < count \
                    or not ((t.is_cuda and t.device == dev) or t.is_pinned()):
                raise _lib.PxtError(f"depth_refine: {name} {k} needs {count} contiguous float32 values in device or pinned "
                                    "memory")
        q = probs[k]
        q.p3d, q.point_mask, q.n_points = pts.data_ptr(), _lib.dptr(mk), n
        q.sensor, q.height, q.width = sen.data_ptr(), int(sen.shape[0]), int(sen.shape[1])
        q.sensor_scale = float(sensor_scales[k])
        q.cam[:] = [float(x) for x in cameras[10 * k:10 * k + 10]]
        q.ndist = int(ndist[k])
        q.pose, q.pose_is_lm_record = poses[k].data_ptr(), int(bool(pose_is_lm_record))
        q.prior[:] = [float(x) for x in priors[21 * k:21 * k + 21]]
        q.out, q.log, q.codes = records[k].data_ptr(), _lib.dptr(lg), _lib.dptr(cd)
    if workspace.numel() * workspace.element_size() < int(L.pxt_depth_refine_workspace_bytes(K)):
        raise _lib.PxtError("depth_refine: workspace smaller than pxt_depth_refine_workspace_bytes(K)")
    conf = _lib.DepthConf()
    conf.num_iters, conf.pad, conf.loss = int(num_iters), int(pad), int(loss)
    conf.loss_alpha, conf.loss_scale = float(loss_alpha), float(loss_scale)
    conf.lambda_[:] = [float(x) for x in lambdas]
    conf.max_residual, conf.max_edge = float(max_residual), float(max_edge)
    conf.grad_stop, conf.dt_stop, conf.dR_stop, conf.min_valid = float(grad_stop), float(dt_stop), float(dR_stop), int(min_valid)
    _lib.check(L.pxt_depth_refine(probs, K, C.byref(conf), workspace.data_ptr(), _stream(workspace)), "pxt_depth_refine")


def _occlusion_record(record, what):
    if record.dtype != torch.int32 or not record.is_contiguous() or record.numel() < _lib.PXT_OCCLUSION_RECORD \
            or not (record.is_cuda or record.is_pinned()):
        raise _lib.PxtError(f"{what}: record needs {_lib.PXT_OCCLUSION_RECORD} contiguous int32 words in device or pinned "
                            "memory")


def _occlusion_mask(depth, sensor, mask_in, shift, min_alpha, sensor_q, delta_q, radii, mask, occluder, record, workspace):
    L = _lib.lib()
    _f32c(depth, "depth")
    if depth.dim() != 3 or int(depth.shape[2]) != 4:
        raise _lib.PxtError(f"occlusion_mask: depth is {tuple(depth.shape)}, expected [H, W, 4]")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if sensor.dtype not in (torch.uint16, torch.int16) or not sensor.is_contiguous() or tuple(sensor.shape) != (H, W):
        raise _lib.PxtError(f"occlusion_mask: sensor is a contiguous uint16 (or int16) [{H}, {W}] tensor "
                            f"(got {tuple(sensor.shape)}, {sensor.dtype})")
    if mask_in.dtype != torch.uint8 or not mask_in.is_contiguous() or tuple(mask_in.shape) != (H, W):
        raise _lib.PxtError(f"occlusion_mask: mask_in is a contiguous uint8 [{H}, {W}] tensor")
    _mask_out(mask, H, W, depth, "occlusion_mask")
    _mask_out(occluder, H, W, depth, "occlusion_mask")
    if mask.data_ptr() == occluder.data_ptr():
        raise _lib.PxtError("occlusion_mask: mask and occluder are two tensors")
    if len(shift) != 2 or any(abs(int(v)) > 32767 for v in shift):
        raise _lib.PxtError(f"occlusion_mask: shift is (shift_x, shift_y), each within +-32767 (got {list(shift)})")
    if len(radii) != 2 or min(int(r) for r in radii) < 0 or int(radii[0]) + int(radii[1]) > _lib.PXT_OCCLUSION_MAX_RADIUS:
        raise _lib.PxtError(f"occlusion_mask: radii are (r_open, r_grow) >= 0 with r_open + r_grow <= "
                            f"{_lib.PXT_OCCLUSION_MAX_RADIUS} (got {list(radii)})")
    _occlusion_record(record, "occlusion_mask")
    need = int(L.pxt_occlusion_mask_workspace_bytes(W, H))
    if need <= 0:
        raise _lib.PxtError(f"occlusion_mask: {W} x {H} is not supported (1..2^28 pixels)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"occlusion_mask: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    for t, name in ((depth, "depth"), (sensor, "sensor"), (mask_in, "mask_in"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != depth.device:
            raise _lib.PxtError(f"occlusion_mask: {name} is on {t.device}, depth on {depth.device}")
    if record.is_cuda and record.device != depth.device:
        raise _lib.PxtError(f"occlusion_mask: record is on {record.device}, depth on {depth.device}")
    _lib.check(L.pxt_occlusion_mask(depth.data_ptr(), sensor.data_ptr(), mask_in.data_ptr(), W, H, int(shift[0]),
                                    int(shift[1]), float(min_alpha), float(sensor_q), float(delta_q), int(radii[0]),
                                    int(radii[1]), mask.data_ptr(), occluder.data_ptr(), record.data_ptr(),
                                    workspace.data_ptr(), _stream(depth)), "pxt_occlusion_mask")


def _occlusion_mask_views(depth, sensors, masks_in, shifts, min_alpha, quanta, radii, masks, occluders, records, workspace):
    L = _lib.lib()
    what = "occlusion_mask_views"
    K = len(depth)
    if not (1 <= K <= _lib.PXT_OCCLUSION_MAX_VIEWS):
        raise _lib.PxtError(f"{what}: 1..{_lib.PXT_OCCLUSION_MAX_VIEWS} views (got {K})")
    if not (len(sensors) == len(masks_in) == len(masks) == len(occluders) == K) or len(shifts) != 2 * K or len(quanta) != 2 * K:
        raise _lib.PxtError(f"{what}: sensors, masks_in, masks and occluders hold one tensor, shifts (shift_x, shift_y) "
                            f"and quanta (sensor_q, delta_q) two values per view ({K} views)")
    if len(radii) != 2 or min(int(r) for r in radii) < 0 or int(radii[0]) + int(radii[1]) > _lib.PXT_OCCLUSION_MAX_RADIUS:
        raise _lib.PxtError(f"{what}: radii are (r_open, r_grow) >= 0 with r_open + r_grow <= "
                            f"{_lib.PXT_OCCLUSION_MAX_RADIUS} (got {list(radii)})")
    if any(abs(int(v)) > 32767 for v in shifts):
        raise _lib.PxtError(f"{what}: every shift is within +-32767 (got {list(shifts)})")
    device = depth[0].device
    views = (_lib.OcclusionView * K)()
    sizes, spans = [], []
    for k in range(K):
        d, sen, mi, mo, oc = depth[k], sensors[k], masks_in[k], masks[k], occluders[k]
        _f32c(d, f"depth[{k}]")
        if d.dim() != 3 or int(d.shape[2]) != 4:
            raise _lib.PxtError(f"{what}: depth[{k}] is [H, W, 4] (got {tuple(d.shape)})")
        H, W = int(d.shape[0]), int(d.shape[1])
        if sen.dtype not in (torch.uint16, torch.int16) or not sen.is_contiguous() or tuple(sen.shape) != (H, W):
            raise _lib.PxtError(f"{what}: sensors[{k}] is a contiguous uint16 (or int16) [{H}, {W}] tensor "
                                f"(got {tuple(sen.shape)}, {sen.dtype})")
        if mi.dtype != torch.uint8 or not mi.is_contiguous() or tuple(mi.shape) != (H, W):
            raise _lib.PxtError(f"{what}: masks_in[{k}] is a contiguous uint8 [{H}, {W}] tensor")
        _mask_out(mo, H, W, d, what)
        _mask_out(oc, H, W, d, what)
        # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
        for t, name in ((d, "depth"), (sen, "sensors"), (mi, "masks_in")):
            _lib.require_gpu(t, f"{name}[{k}]")
            if t.device != device:
                raise _lib.PxtError(f"{what}: {name}[{k}] is on {t.device}, depth[0] on {device}")
        sizes += [W, H]
        spans += [(mo.data_ptr(), mo.data_ptr() + H * W, f"masks[{k}]"), (oc.data_ptr(), oc.data_ptr() + H * W, f"occluders[{k}]")]
        v = views[k]
        v.depth, v.sensor, v.mask_in, v.mask_out, v.occluder = d.data_ptr(), sen.data_ptr(), mi.data_ptr(), mo.data_ptr(), oc.data_ptr()
        v.width, v.height, v.shift_x, v.shift_y = W, H, int(shifts[2 * k]), int(shifts[2 * k + 1])
        v.sensor_q, v.delta_q = float(quanta[2 * k]), float(quanta[2 * k + 1])
    spans.sort()
    for (_lo, hi, a), (lo, _hi, b) in zip(spans, spans[1:]):
        if lo < hi:
            raise _lib.PxtError(f"{what}: {a} and {b} overlap; every view writes planes of its own")
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (K, _lib.PXT_OCCLUSION_RECORD) \
            or not ((records.is_cuda and records.device == device) or records.is_pinned()):
        raise _lib.PxtError(f"{what}: records is a contiguous int32 [{K}, {_lib.PXT_OCCLUSION_RECORD}] tensor on the depth "
                            "planes' device or in pinned memory")
    need = int(L.pxt_occlusion_mask_views_workspace_bytes(K, (C.c_int32 * (2 * K))(*sizes)))
    if need <= 0:
        raise _lib.PxtError(f"{what}: planes of {list(zip(sizes[0::2], sizes[1::2]))} are not supported (1..2^28 pixels)")
    _lib.require_gpu(workspace, "workspace")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or workspace.device != device:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {need} bytes on {device}")
    _lib.check(L.pxt_occlusion_mask_views(views, K, float(min_alpha), int(radii[0]), int(radii[1]), records.data_ptr(),
                                          workspace.data_ptr(), _stream(depth[0])), "pxt_occlusion_mask_views")


def _mask_exclude(mask_in, occluder, mask, record):
    L = _lib.lib()
    if mask_in.dtype != torch.uint8 or mask_in.dim() != 2 or not mask_in.is_contiguous():
        raise _lib.PxtError("mask_exclude: mask_in is a contiguous uint8 [H, W] tensor")
    H, W = int(mask_in.shape[0]), int(mask_in.shape[1])
    for t, name in ((occluder, "occluder"), (mask, "mask")):
        if t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (H, W):
            raise _lib.PxtError(f"mask_exclude: {name} is a contiguous uint8 [{H}, {W}] tensor (got {tuple(t.shape)}, "
                                f"{t.dtype})")
        _lib.require_gpu(t, name)
        if t.device != mask_in.device:
            raise _lib.PxtError(f"mask_exclude: {name} is on {t.device}, mask_in on {mask_in.device}")
    _lib.require_gpu(mask_in, "mask_in")
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise _lib.PxtError(f"mask_exclude: {W} x {H} is not supported (1..2^28 pixels)")
    if mask.data_ptr() == occluder.data_ptr():
        raise _lib.PxtError("mask_exclude: mask may be mask_in, not occluder")
    if record.dtype != torch.int32 or not record.is_contiguous() or record.numel() < 2 \
            or not (record.is_cuda or record.is_pinned()):
        raise _lib.PxtError("mask_exclude: record needs 2 contiguous int32 words in device or pinned memory")
    if record.is_cuda and record.device != mask_in.device:
        raise _lib.PxtError(f"mask_exclude: record is on {record.device}, mask_in on {mask_in.device}")
    _lib.check(L.pxt_mask_exclude(mask_in.data_ptr(), occluder.data_ptr(), W, H, mask.data_ptr(), record.data_ptr(),
                                  _stream(mask_in)), "pxt_mask_exclude")


def _points_visible(p3d, valid_in, pose, camera, ndist, occluder, valid, record):
    L = _lib.lib()
    _f32c(p3d, "p3d")
    n = int(p3d.shape[0])
    if tuple(p3d.shape) != (n, 3):
        raise _lib.PxtError(f"points_visible: p3d is {tuple(p3d.shape)}, expected [N, 3]")
    if occluder.dtype != torch.uint8 or occluder.dim() != 2 or not occluder.is_contiguous():
        raise _lib.PxtError("points_visible: occluder is a contiguous uint8 [H, W]")
    H, W = int(occluder.shape[0]), int(occluder.shape[1])
    if len(pose) != 12 or len(camera) != 10:
        raise _lib.PxtError("points_visible: pose holds 12 floats, camera 10")
    if (float(camera[0]), float(camera[1])) != (float(W), float(H)):
        raise _lib.PxtError(f"points_visible: the camera is {camera[0]:g} x {camera[1]:g}, the occluder plane {W} x {H}")
    for t, name in ((valid_in, "valid_in"), (valid, "valid")):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (n,)):
            raise _lib.PxtError(f"points_visible: {name} is a contiguous uint8 [{n}] tensor")
    _occlusion_record(record, "points_visible")
    _lib.require_gpu(occluder, "occluder")
    for t, name in ((p3d, "p3d"), (valid_in, "valid_in"), (valid, "valid")):
        if t is None:
            continue
        _lib.require_gpu(t, name)
        if t.device != occluder.device:
            raise _lib.PxtError(f"points_visible: {name} is on {t.device}, the occluder plane on {occluder.device}")
    if record.is_cuda and record.device != occluder.device:
        raise _lib.PxtError(f"points_visible: record is on {record.device}, the occluder plane on {occluder.device}")
    T = (C.c_float * 12)(*[float(x) for x in pose])
    cam = (C.c_float * 10)(*[float(x) for x in camera])
    _lib.check(L.pxt_points_visible(p3d.data_ptr() if n else None, _lib.dptr(valid_in) if n else None, n, T, cam,
                                    int(ndist), occluder.data_ptr(), W, H, valid.data_ptr() if n else None,
                                    record.data_ptr(), _stream(occluder)), "pxt_points_visible")


def _ngp_query(ctx, pos, dir, out):
    _f32c(pos, "pos")
    _f32c(dir, "dir")
    _f32c(out, "out")
    n = int(pos.shape[0])
    if tuple(pos.shape) != (n, 3) or tuple(dir.shape) != (n, 3) or tuple(out.shape) != (n, 4) or n < 1:
        raise _lib.PxtError(f"ngp_query: pos {tuple(pos.shape)} / dir {tuple(dir.shape)} / out {tuple(out.shape)}, expected "
                            "[n, 3] / [n, 3] / [n, 4], n >= 1")
    for t, name in ((pos, "pos"), (dir, "dir"), (out, "out")):
        _lib.require_gpu(t, name)
        if t.device != pos.device:
            raise _lib.PxtError(f"ngp_query: {name} is on {t.device}, pos on {pos.device}")
    _lib.check(_lib.lib().pxt_ngp_query(int(ctx), pos.data_ptr(), dir.data_ptr(), n, out.data_ptr(), _stream(pos)),
               "pxt_ngp_query")


def _iso_grid(values, grid, what):
    _f32c(values, "values")
    if values.dim() != 3 or len(grid) != 7:
        raise _lib.PxtError(f"{what}: values is [nz, ny, nx] (got {tuple(values.shape)}), grid holds iso, origin xyz, "
                            "spacing xyz")
    nz, ny, nx = (int(v) for v in values.shape)
    need = int(_lib.lib().pxt_iso_surface_workspace_bytes(nx, ny, nz)) if min(nx, ny, nz) >= 1 else -1
    if need <= 0:
        raise _lib.PxtError(f"{what}: a {nz} x {ny} x {nx} lattice is not supported (every extent >= 1, <= 2^27 points)")
    g = [float(v) for v in grid]
    return _lib.IsoGrid(nx, ny, nz, g[0], (C.c_float * 3)(*g[1:4]), (C.c_float * 3)(*g[4:7])), need


def _iso_workspace(workspace, need, values, what):
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {need} bytes")
    for t, name in ((values, "values"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != values.device:
            raise _lib.PxtError(f"{what}: {name} is on {t.device}, the values on {values.device}")


def _iso_surface_count(values, grid, workspace, counts):
    g, need = _iso_grid(values, grid, "iso_surface_count")
    _iso_workspace(workspace, need, values, "iso_surface_count")
    if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.numel() < 2 \
            or not ((counts.is_cuda and counts.device == values.device) or counts.is_pinned()):
        raise _lib.PxtError("iso_surface_count: counts needs 2 contiguous int32 words on the values' device or in pinned memory")
    _lib.check(_lib.lib().pxt_iso_surface_count(values.data_ptr(), C.byref(g), workspace.data_ptr(), counts.data_ptr(),
                                                _stream(values)), "pxt_iso_surface_count")


def _iso_surface_emit(values, grid, workspace, vertices, normals, triangles):
    g, need = _iso_grid(values, grid, "iso_surface_emit")
    _iso_workspace(workspace, need, values, "iso_surface_emit")
    _f32c(vertices, "vertices")
    n, m = int(vertices.shape[0]), int(triangles.shape[0])
    if tuple(vertices.shape) != (n, 3) or triangles.dtype != torch.int32 or not triangles.is_contiguous() \
            or tuple(triangles.shape) != (m, 3):
        raise _lib.PxtError(f"iso_surface_emit: vertices is float32 [n, 3], triangles contiguous int32 [m, 3] (got "
                            f"{tuple(vertices.shape)}, {tuple(triangles.shape)} {triangles.dtype})")
    if normals is not None and (_f32c(normals, "normals").shape != vertices.shape):
        raise _lib.PxtError(f"iso_surface_emit: normals is float32 {tuple(vertices.shape)}")
    for t, name in ((vertices, "vertices"), (normals, "normals"), (triangles, "triangles")):
        if t is None:
            continue
        _lib.require_gpu(t, name)
        if t.device != values.device:
            raise _lib.PxtError(f"iso_surface_emit: {name} is on {t.device}, the values on {values.device}")
    _lib.check(_lib.lib().pxt_iso_surface_emit(values.data_ptr(), C.byref(g), workspace.data_ptr(),
                                               vertices.data_ptr() if n else None, n,
                                               _lib.dptr(normals) if n else None, triangles.data_ptr() if m else None, m,
                                               _stream(values)), "pxt_iso_surface_emit")


def _max_pairwise_distance(points, out, workspace):
    L = _lib.lib()
    _f32c(points, "points")
    n = int(points.shape[0])
    if tuple(points.shape) != (n, 3):
        raise _lib.PxtError(f"max_pairwise_distance: points is {tuple(points.shape)}, expected [n, 3]")
    need = int(L.pxt_max_pairwise_distance_workspace_bytes(n))
    if need <= 0:
        raise _lib.PxtError(f"max_pairwise_distance: {n} points is not supported (1..2^22)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"max_pairwise_distance: workspace is a contiguous uint8 tensor of >= {need} bytes")
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < 4 \
            or not ((out.is_cuda and out.device == points.device) or out.is_pinned()):
        raise _lib.PxtError("max_pairwise_distance: out needs 4 contiguous int32 words on the points' device or in pinned "
                            "memory")
    for t, name in ((points, "points"), (workspace, "workspace")):
        _lib.require_gpu(t, name)
        if t.device != points.device:
            raise _lib.PxtError(f"max_pairwise_distance: {name} is on {t.device}, the points on {points.device}")
    _lib.check(L.pxt_max_pairwise_distance(points.data_ptr(), n, workspace.data_ptr(), out.data_ptr(), _stream(points)),
               "pxt_max_pairwise_distance")


def _mesh_raster(vertices, triangles, views, depth, triangle_ids, records, workspace):
    L = _lib.lib()
    _f32c(vertices, "vertices")
    _f32c(views, "views")
    _f32c(depth, "depth")
    if (vertices.dim() != 2 or int(vertices.shape[1]) != 3 or triangles.dim() != 2 or int(triangles.shape[1]) != 3
            or triangles.dtype != torch.int32 or not triangles.is_contiguous() or views.dim() != 2
            or int(views.shape[1]) != _lib.PXT_MESH_VIEW):
        raise _lib.PxtError(f"mesh_raster: vertices {tuple(vertices.shape)} / triangles {tuple(triangles.shape)} "
                            f"{triangles.dtype} / views {tuple(views.shape)}, expected float32 [V, 3] / contiguous int32 "
                            f"[T, 3] / float32 [P, {_lib.PXT_MESH_VIEW}]")
    V, T, P = int(vertices.shape[0]), int(triangles.shape[0]), int(views.shape[0])
    if depth.dim() != 4 or int(depth.shape[0]) != P or int(depth.shape[3]) != 4:
        raise _lib.PxtError(f"mesh_raster: depth is {tuple(depth.shape)}, expected [{P}, H, W, 4]")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if triangle_ids is not None and (triangle_ids.dtype != torch.int32 or not triangle_ids.is_contiguous()
                                     or tuple(triangle_ids.shape) != (P, H, W)):
        raise _lib.PxtError(f"mesh_raster: triangle_ids is a contiguous int32 [{P}, {H}, {W}] tensor (got "
                            f"{tuple(triangle_ids.shape)}, {triangle_ids.dtype})")
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_MESH_RASTER_RECORD):
        raise _lib.PxtError(f"mesh_raster: records is a contiguous int32 [{P}, {_lib.PXT_MESH_RASTER_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    need = int(L.pxt_mesh_raster_workspace_bytes(P, T, W, H)) if min(P, T, W, H) >= 1 else -1
    if need <= 0 or not (1 <= V <= 1 << 24):
        raise _lib.PxtError(f"mesh_raster: {P} views of {W} x {H}, {V} vertices, {T} triangles are not supported "
                            "(1..4096 views, 1..2^26 pixels, 1..2^24 vertices and triangles)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"mesh_raster: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    named = [(vertices, "vertices"), (triangles, "triangles"), (views, "views"), (depth, "depth"), (records, "records"),
             (workspace, "workspace")] + ([(triangle_ids, "triangle_ids")] if triangle_ids is not None else [])
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != vertices.device:
            raise _lib.PxtError(f"mesh_raster: {name} is on {t.device}, the vertices on {vertices.device}")
    _lib.check(L.pxt_mesh_raster(vertices.data_ptr(), V, triangles.data_ptr(), T, views.data_ptr(), P, W, H,
                                 depth.data_ptr(), _lib.dptr(triangle_ids), records.data_ptr(), workspace.data_ptr(),
                                 _stream(vertices)), "pxt_mesh_raster")


def _mesh_render_checked(what, vertices, triangles, attrs, check_attrs, views, width, height, rgba, rgb_u8, depth,
                         depth_nz, triangle_ids, records, workspace):
    """The checks mesh_render and mesh_render_textured share -> (V, T, P, W, H).  ``attrs``: [(tensor, name)] of the
    call's own inputs, ``check_attrs(V, T)`` their shapes."""
    L = _lib.lib()
    _f32c(vertices, "vertices")
    _f32c(views, "views")
    if (vertices.dim() != 2 or int(vertices.shape[1]) != 3 or triangles.dim() != 2 or int(triangles.shape[1]) != 3
            or triangles.dtype != torch.int32 or not triangles.is_contiguous() or views.dim() != 2
            or int(views.shape[1]) != _lib.PXT_MESH_VIEW):
        raise _lib.PxtError(f"{what}: vertices {tuple(vertices.shape)} / triangles {tuple(triangles.shape)} "
                            f"{triangles.dtype} / views {tuple(views.shape)}, expected float32 [V, 3] / contiguous int32 "
                            f"[T, 3] / float32 [P, {_lib.PXT_MESH_VIEW}]")
    V, T, P, W, H = int(vertices.shape[0]), int(triangles.shape[0]), int(views.shape[0]), int(width), int(height)
    check_attrs(V, T)
    outs = [(rgba, "rgba", torch.float32, (P, H, W, 4)), (rgb_u8, "rgb_u8", torch.uint8, (P, H, W, 3)),
            (depth, "depth", torch.float32, (P, H, W, 4)), (depth_nz, "depth_nz", torch.uint8, (P, H, W)),
            (triangle_ids, "triangle_ids", torch.int32, (P, H, W))]
    for t, name, dtype, shape in outs:
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape):
            raise _lib.PxtError(f"{what}: {name} is a contiguous {dtype} {list(shape)} tensor (got "
                                f"{tuple(t.shape)}, {t.dtype})")
    if all(t is None for t, *_ in outs):
        raise _lib.PxtError(f"{what}: no output was asked for")
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_MESH_RASTER_RECORD):
        raise _lib.PxtError(f"{what}: records is a contiguous int32 [{P}, {_lib.PXT_MESH_RASTER_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    need = int(L.pxt_mesh_raster_workspace_bytes(P, T, W, H)) if min(P, T, W, H) >= 1 else -1
    if need <= 0 or not (1 <= V <= 1 << 24):
        raise _lib.PxtError(f"{what}: {P} views of {W} x {H}, {V} vertices, {T} triangles are not supported "
                            "(1..4096 views, 1..2^26 pixels, 1..2^24 vertices and triangles)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {need} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    named = [(vertices, "vertices"), (triangles, "triangles"), *attrs, (views, "views"), (records, "records"),
             (workspace, "workspace")] + [(t, name) for t, name, *_ in outs if t is not None]
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != vertices.device:
            raise _lib.PxtError(f"{what}: {name} is on {t.device}, the vertices on {vertices.device}")
    return V, T, P, W, H


def _mesh_render(vertices, triangles, colors, views, width, height, rgba, rgb_u8, depth, depth_nz, triangle_ids,
                 records, workspace):
    _f32c(colors, "colors")

    def check(V, T):
        if tuple(colors.shape) != (V, 3):
            raise _lib.PxtError(f"mesh_render: colors is {tuple(colors.shape)}, expected float32 [{V}, 3]")

    V, T, P, W, H = _mesh_render_checked("mesh_render", vertices, triangles, [(colors, "colors")], check, views, width,
                                         height, rgba, rgb_u8, depth, depth_nz, triangle_ids, records, workspace)
    _lib.check(_lib.lib().pxt_mesh_render(
        vertices.data_ptr(), V, triangles.data_ptr(), T, colors.data_ptr(), views.data_ptr(), P, W, H, _lib.dptr(rgba),
        _lib.dptr(rgb_u8), _lib.dptr(depth), _lib.dptr(depth_nz), _lib.dptr(triangle_ids), records.data_ptr(),
        workspace.data_ptr(), _stream(vertices)), "pxt_mesh_render")


def _mesh_render_textured(vertices, triangles, uvs, triangle_uvs, texture, views, width, height, rgba, rgb_u8, depth,
                          depth_nz, triangle_ids, records, workspace):
    _f32c(uvs, "uvs")

    def check(V, T):
        if uvs.dim() != 2 or int(uvs.shape[1]) != 2 or not (1 <= int(uvs.shape[0]) <= 1 << 24):
            raise _lib.PxtError(f"mesh_render_textured: uvs is {tuple(uvs.shape)}, expected float32 [1..2^24, 2]")
        if triangle_uvs.dtype != torch.int32 or not triangle_uvs.is_contiguous() or tuple(triangle_uvs.shape) != (T, 3):
            raise _lib.PxtError(f"mesh_render_textured: triangle_uvs is a contiguous int32 [{T}, 3] tensor (got "
                                f"{tuple(triangle_uvs.shape)}, {triangle_uvs.dtype})")
        if (texture.dtype != torch.uint8 or not texture.is_contiguous() or texture.dim() != 3 or int(texture.shape[2]) != 4
                or not (1 <= int(texture.shape[0]) <= 16384 and 1 <= int(texture.shape[1]) <= 16384)):
            raise _lib.PxtError("mesh_render_textured: texture is a contiguous uint8 [1..16384, 1..16384, 4] tensor (got "
                                f"{tuple(texture.shape)}, {texture.dtype})")

    V, T, P, W, H = _mesh_render_checked(
        "mesh_render_textured", vertices, triangles, [(uvs, "uvs"), (triangle_uvs, "triangle_uvs"), (texture, "texture")],
        check, views, width, height, rgba, rgb_u8, depth, depth_nz, triangle_ids, records, workspace)
    _lib.check(_lib.lib().pxt_mesh_render_textured(
        vertices.data_ptr(), V, triangles.data_ptr(), T, uvs.data_ptr(), int(uvs.shape[0]), triangle_uvs.data_ptr(),
        texture.data_ptr(), int(texture.shape[1]), int(texture.shape[0]), views.data_ptr(), P, W, H, _lib.dptr(rgba),
        _lib.dptr(rgb_u8), _lib.dptr(depth), _lib.dptr(depth_nz), _lib.dptr(triangle_ids), records.data_ptr(),
        workspace.data_ptr(), _stream(vertices)), "pxt_mesh_render_textured")


def mesh_frame_planes(geometry, offsets, what="mesh_render_frame", max_views=_lib.PXT_MESH_FRAME_MAX_VIEWS):
    """The argument checks of mesh_render_frame that need no tensor: ``geometry`` = P x (width, height, supersample),
    ``offsets`` = P x (rgba, rgb_u8, depth, depth_nz) byte offsets or -1 -> (P, the bytes each of the four buffers
    must hold)."""
    geometry, offsets = [int(x) for x in geometry], [int(x) for x in offsets]
    P = len(geometry) // 3
    if not (1 <= P <= max_views) or len(geometry) != 3 * P or len(offsets) != 4 * P:
        raise _lib.PxtError(f"{what}: geometry holds (width, height, supersample) and offsets four byte offsets for "
                            f"each of 1..{max_views} views (got {len(geometry)} and {len(offsets)} "
                            "numbers)")
    need = [0, 0, 0, 0]
    spans = [[], [], [], []]
    names = ("rgba", "rgb_u8", "depth", "depth_nz")
    for p in range(P):
        W, H, S = geometry[3 * p:3 * p + 3]
        if S not in (1, 2, 4):
            raise _lib.PxtError(f"{what}: view {p}: supersample is 1, 2 or 4 (got {S})")
        if W < 1 or H < 1 or W * S * H * S > 1 << 26:
            raise _lib.PxtError(f"{what}: view {p}: {W} x {H} at supersample {S} is not supported (1..2^26 fine pixels)")
        off = offsets[4 * p:4 * p + 4]
        if all(o < 0 for o in off):
            raise _lib.PxtError(f"{what}: view {p} asks for no output")
        if S > 1 and (off[2] >= 0 or off[3] >= 0):
            raise _lib.PxtError(f"{what}: view {p}: depth and depth_nz exist for supersample 1 alone (got {S})")
        for k, (o, px, al) in enumerate(zip(off, (16, 3, 16, 1), (16, 4, 16, 4))):
            if o < 0:
                continue
            if o % al:
                raise _lib.PxtError(f"{what}: view {p}: the {names[k]} offset {o} is not a multiple of {al}")
            need[k] = max(need[k], o + W * H * px)
            spans[k].append((o, o + W * H * px))
    for k in range(4):
        sp = sorted(spans[k])
        if any(a[1] > b[0] for a, b in zip(sp, sp[1:])):
            raise _lib.PxtError(f"{what}: two views' {names[k]} planes overlap")
    return P, need


def _mesh_render_frame(vertices, triangles, colors, uvs, triangle_uvs, texture, views, geometry, offsets, rgba, rgb_u8,
                       depth, depth_nz, records, workspace):
    what = "mesh_render_frame"
    L = _lib.lib()
    _f32c(vertices, "vertices")
    _f32c(views, "views")
    if (vertices.dim() != 2 or int(vertices.shape[1]) != 3 or triangles.dim() != 2 or int(triangles.shape[1]) != 3
            or triangles.dtype != torch.int32 or not triangles.is_contiguous() or views.dim() != 2
            or int(views.shape[1]) != _lib.PXT_MESH_VIEW):
        raise _lib.PxtError(f"{what}: vertices {tuple(vertices.shape)} / triangles {tuple(triangles.shape)} "
                            f"{triangles.dtype} / views {tuple(views.shape)}, expected float32 [V, 3] / contiguous int32 "
                            f"[T, 3] / float32 [P, {_lib.PXT_MESH_VIEW}]")
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    P, need = mesh_frame_planes(geometry, offsets, what)
    if int(views.shape[0]) != P:
        raise _lib.PxtError(f"{what}: {int(views.shape[0])} views for {P} geometry entries")
    attrs = _mesh_shading_checked(what, V, T, colors, uvs, triangle_uvs, texture)
    outs, out_bytes = _mesh_frame_buffers(what, need, rgba, rgb_u8, depth, depth_nz)
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_MESH_RASTER_RECORD):
        raise _lib.PxtError(f"{what}: records is a contiguous int32 [{P}, {_lib.PXT_MESH_RASTER_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    geo = (C.c_int32 * (3 * P))(*[int(x) for x in geometry])
    off = (C.c_int64 * (4 * P))(*[int(x) for x in offsets])
    cap = (C.c_int64 * 4)(*out_bytes)
    bytes_needed = int(L.pxt_mesh_render_frame_workspace_bytes(P, T, geo)) if T >= 1 else -1
    if bytes_needed <= 0 or not (1 <= V <= 1 << 24):
        raise _lib.PxtError(f"{what}: {V} vertices, {T} triangles are not supported (1..2^24 vertices and triangles)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < bytes_needed:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {bytes_needed} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    named = [(vertices, "vertices"), (triangles, "triangles"), *attrs, (views, "views"), (records, "records"),
             (workspace, "workspace")] + [(t, name) for t, name, _ in outs if t is not None]
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != vertices.device:
            raise _lib.PxtError(f"{what}: {name} is on {t.device}, the vertices on {vertices.device}")
    _lib.check(L.pxt_mesh_render_frame(
        vertices.data_ptr(), V, triangles.data_ptr(), T, _lib.dptr(colors), _lib.dptr(uvs),
        0 if uvs is None else int(uvs.shape[0]), _lib.dptr(triangle_uvs), _lib.dptr(texture),
        0 if texture is None else int(texture.shape[1]), 0 if texture is None else int(texture.shape[0]), views.data_ptr(),
        P, geo, off, _lib.dptr(rgba), _lib.dptr(rgb_u8), _lib.dptr(depth), _lib.dptr(depth_nz), cap, records.data_ptr(),
        workspace.data_ptr(), _stream(vertices)), "pxt_mesh_render_frame")


def mesh_batch_planes(view_mesh, n_meshes, geometry, offsets, what="mesh_render_frame_batch"):
    """The argument checks of mesh_render_frame_batch that need no tensor: ``view_mesh`` = the mesh of each of the P
    views, ``n_meshes`` = M, ``geometry`` and ``offsets`` as ``mesh_frame_planes`` -> (P, the bytes each of the four
    buffers must hold)."""
    view_mesh, M = [int(x) for x in view_mesh], int(n_meshes)
    if not (1 <= M <= _lib.PXT_MESH_BATCH_MAX_MESHES):
        raise _lib.PxtError(f"{what}: 1..{_lib.PXT_MESH_BATCH_MAX_MESHES} meshes per call (got {M})")
    P, need = mesh_frame_planes(geometry, offsets, what, _lib.PXT_MESH_BATCH_MAX_VIEWS)
    if len(view_mesh) != P:
        raise _lib.PxtError(f"{what}: view_mesh names the mesh of each of the {P} views (got {len(view_mesh)} numbers)")
    bad = [(p, m) for p, m in enumerate(view_mesh) if not (0 <= m < M)]
    if bad:
        raise _lib.PxtError(f"{what}: view {bad[0][0]} names mesh {bad[0][1]} of {M}")
    return P, need


def _mesh_shading_checked(what, V, T, colors, uvs, triangle_uvs, texture):
    """One mesh's shading inputs -> the tensors the kernels dereference, named."""
    textured = uvs is not None or triangle_uvs is not None or texture is not None
    if (colors is not None) == textured:
        raise _lib.PxtError(f"{what}: a mesh is drawn with colors or with uvs + triangle_uvs + texture, one of the two")
    if not textured:
        _f32c(colors, "colors")
        if tuple(colors.shape) != (V, 3):
            raise _lib.PxtError(f"{what}: colors is {tuple(colors.shape)}, expected float32 [{V}, 3]")
        return [(colors, "colors")]
    if uvs is None or triangle_uvs is None or texture is None:
        raise _lib.PxtError(f"{what}: a textured mesh needs uvs, triangle_uvs and texture")
    _f32c(uvs, "uvs")
    if uvs.dim() != 2 or int(uvs.shape[1]) != 2 or not (1 <= int(uvs.shape[0]) <= 1 << 24):
        raise _lib.PxtError(f"{what}: uvs is {tuple(uvs.shape)}, expected float32 [1..2^24, 2]")
    if triangle_uvs.dtype != torch.int32 or not triangle_uvs.is_contiguous() or tuple(triangle_uvs.shape) != (T, 3):
        raise _lib.PxtError(f"{what}: triangle_uvs is a contiguous int32 [{T}, 3] tensor (got "
                            f"{tuple(triangle_uvs.shape)}, {triangle_uvs.dtype})")
    if (texture.dtype != torch.uint8 or not texture.is_contiguous() or texture.dim() != 3 or int(texture.shape[2]) != 4
            or not (1 <= int(texture.shape[0]) <= 16384 and 1 <= int(texture.shape[1]) <= 16384)):
        raise _lib.PxtError(f"{what}: texture is a contiguous uint8 [1..16384, 1..16384, 4] tensor (got "
                            f"{tuple(texture.shape)}, {texture.dtype})")
    return [(uvs, "uvs"), (triangle_uvs, "triangle_uvs"), (texture, "texture")]


def _mesh_frame_buffers(what, need, rgba, rgb_u8, depth, depth_nz):
    """The four flat output buffers hold the views' planes -> (the buffers named, their sizes in bytes)."""
    outs = [(rgba, "rgba", torch.float32), (rgb_u8, "rgb_u8", torch.uint8), (depth, "depth", torch.float32),
            (depth_nz, "depth_nz", torch.uint8)]
    out_bytes = []
    for (t, name, dtype), n in zip(outs, need):
        have = 0 if t is None else t.numel() * t.element_size()
        if t is not None and (t.dtype != dtype or not t.is_contiguous()):
            raise _lib.PxtError(f"{what}: {name} is a contiguous {dtype} buffer (got {t.dtype})")
        if have < n:
            raise _lib.PxtError(f"{what}: {name} holds {have} bytes, the views' planes need {n}")
        out_bytes.append(have)
    return outs, out_bytes


def mesh_scene_planes(view_scene, r_grow, occluder_offsets, geometry, what="mesh_render_scene_batch"):
    """The argument checks of mesh_render_scene_batch that need no tensor and no view floats: ``view_scene`` = the scene
    of each of the P views (-1: none), ``occluder_offsets`` = where each view's [H, W] uint8 plane starts in the flat
    occluder buffer (-1: none), ``geometry`` as ``mesh_frame_planes`` -> the bytes that buffer must hold."""
    P = len(geometry) // 3
    view_scene, offs, r_grow = [int(x) for x in view_scene], [int(x) for x in occluder_offsets], int(r_grow)
    if len(view_scene) != P or len(offs) != P:
        raise _lib.PxtError(f"{what}: view_scene and occluder_offsets hold one number per view ({P}; got {len(view_scene)}, "
                            f"{len(offs)})")
    if not (0 <= r_grow <= _lib.PXT_MESH_SCENE_MAX_GROW):
        raise _lib.PxtError(f"{what}: r_grow is 0..{_lib.PXT_MESH_SCENE_MAX_GROW} (got {r_grow})")
    first, spans = {}, []
    for p, (s, off) in enumerate(zip(view_scene, offs)):
        W, H, S = (int(x) for x in geometry[3 * p:3 * p + 3])
        if not (-1 <= s < P):
            raise _lib.PxtError(f"{what}: view {p} names scene {s}; a scene id is -1 (none) or 0..{P - 1}")
        if s < 0:
            if off >= 0:
                raise _lib.PxtError(f"{what}: view {p} asks for an occluder plane but is in no scene")
            continue
        if S != 1:
            raise _lib.PxtError(f"{what}: view {p} of scene {s} has supersample {S}; a scene's views have supersample 1")
        q = first.setdefault(s, p)
        if tuple(geometry[3 * q:3 * q + 2]) != tuple(geometry[3 * p:3 * p + 2]):
            raise _lib.PxtError(f"{what}: views {q} and {p} of scene {s} differ in size: a scene is one camera")
        if off >= 0:
            if off % 4:
                raise _lib.PxtError(f"{what}: view {p}'s occluder plane starts at byte {off}, not a multiple of 4")
            spans.append((off, off + W * H, p))
    spans.sort()
    for (a0, a1, p), (b0, b1, q) in zip(spans, spans[1:]):
        if b0 < a1:
            raise _lib.PxtError(f"{what}: the occluder planes of views {p} and {q} overlap")
    return max([e for _, e, _ in spans], default=0)


def _mesh_render_frame_batch(vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views, geometry, offsets,
                             rgba, rgb_u8, depth, depth_nz, records, workspace):
    _mesh_batch_call("mesh_render_frame_batch", vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views,
                     geometry, offsets, rgba, rgb_u8, depth, depth_nz, records, workspace, None)


def _mesh_render_scene_batch(vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views, geometry, offsets,
                             view_scene, r_grow, occluder_offsets, rgba, rgb_u8, depth, depth_nz, occluder, records,
                             workspace):
    _mesh_batch_call("mesh_render_scene_batch", vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views,
                     geometry, offsets, rgba, rgb_u8, depth, depth_nz, records, workspace,
                     (view_scene, r_grow, occluder_offsets, occluder))


def _mesh_render_frame_batch_posed(vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views, geometry,
                                   offsets, pose_records, radii, rgba, rgb_u8, depth, depth_nz, records, workspace,
                                   views_out):
    _mesh_batch_call("mesh_render_frame_batch_posed", vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh,
                     views, geometry, offsets, rgba, rgb_u8, depth, depth_nz, records, workspace, None,
                     (pose_records, radii, views_out))


def mesh_view_poses(pose_records, radii, views_out, P, device, what="mesh_render_frame_batch_posed"):
    """The checks of mesh_render_frame_batch_posed's own arguments -> the ``pxt_mesh_view_pose`` array.  A record or
    ``views_out`` is memory the kernel dereferences: of ``device``, or pinned host memory."""
    def reachable(t, name):
        if not (t.is_cuda and t.device == device) and not (not t.is_cuda and t.is_pinned()):
            raise _lib.PxtError(f"{what}: {name} is memory of {device} or pinned host memory (got {t.device}, unpinned)")
    if len(pose_records) != P or len(radii) != P:
        raise _lib.PxtError(f"{what}: pose_records and radii hold one entry per view ({P}; got {len(pose_records)}, "
                            f"{len(radii)})")
    table = (_lib.MeshViewPose * P)()
    for p, (rec, radius) in enumerate(zip(pose_records, radii)):
        if rec is None:
            continue
        _f32c(rec, f"pose_records[{p}]")
        if rec.numel() < 16:
            raise _lib.PxtError(f"{what}: pose_records[{p}] holds {rec.numel()} floats, an LM output record has >= 16")
        reachable(rec, f"pose_records[{p}]")
        radius = float(radius)
        if not (math.isfinite(radius) and radius >= 0.0):
            raise _lib.PxtError(f"{what}: view {p}'s radius is finite and >= 0 (got {radius})")
        table[p].pose_record, table[p].radius = rec.data_ptr(), radius
    if views_out is not None:
        _f32c(views_out, "views_out")
        if tuple(views_out.shape) != (P, _lib.PXT_MESH_VIEW_OUT):
            raise _lib.PxtError(f"{what}: views_out is float32 [{P}, {_lib.PXT_MESH_VIEW_OUT}] (got {tuple(views_out.shape)})")
        reachable(views_out, "views_out")
    return table


def _mesh_batch_call(what, vertices, triangles, colors, uvs, triangle_uvs, texture, view_mesh, views, geometry, offsets,
                     rgba, rgb_u8, depth, depth_nz, records, workspace, scene, posed=None):
    """The batch ops: ``scene`` = (view_scene, r_grow, occluder_offsets, occluder) for mesh_render_scene_batch,
    ``posed`` = (pose_records, radii, views_out) for mesh_render_frame_batch_posed."""
    L = _lib.lib()
    M = len(vertices)
    if not all(len(x) == M for x in (triangles, colors, uvs, triangle_uvs, texture)):
        raise _lib.PxtError(f"{what}: vertices, triangles, colors, uvs, triangle_uvs and texture hold one entry per mesh "
                            f"(got {[len(x) for x in (vertices, triangles, colors, uvs, triangle_uvs, texture)]})")
    P, need = mesh_batch_planes(view_mesh, M, geometry, offsets, what)
    if (views.is_cuda or views.dtype != torch.float32 or not views.is_contiguous()
            or tuple(views.shape) != (P, _lib.PXT_MESH_VIEW)):
        raise _lib.PxtError(f"{what}: views is a contiguous float32 CPU tensor [{P}, {_lib.PXT_MESH_VIEW}] (got "
                            f"{tuple(views.shape)}, {views.dtype}, {views.device})")
    named, descs, counts = [], (_lib.MeshDesc * M)(), []
    for m in range(M):
        v, t = vertices[m], triangles[m]
        _f32c(v, f"vertices[{m}]")
        if (v.dim() != 2 or int(v.shape[1]) != 3 or t.dim() != 2 or int(t.shape[1]) != 3 or t.dtype != torch.int32
                or not t.is_contiguous()):
            raise _lib.PxtError(f"{what}: mesh {m}: vertices {tuple(v.shape)} / triangles {tuple(t.shape)} {t.dtype}, "
                                "expected float32 [V, 3] / contiguous int32 [T, 3]")
        V, T = int(v.shape[0]), int(t.shape[0])
        if not (1 <= V <= 1 << 24 and 1 <= T <= 1 << 24):
            raise _lib.PxtError(f"{what}: mesh {m}: {V} vertices, {T} triangles are not supported (1..2^24 vertices and "
                                "triangles)")
        attrs = _mesh_shading_checked(f"{what}: mesh {m}", V, T, colors[m], uvs[m], triangle_uvs[m], texture[m])
        named += [(v, f"vertices[{m}]"), (t, f"triangles[{m}]")] + [(a, f"{n}[{m}]") for a, n in attrs]
        d = descs[m]
        d.vertices, d.triangles, d.n_vertices, d.n_triangles = v.data_ptr(), t.data_ptr(), V, T
        d.colors, d.uvs = _lib.dptr(colors[m]), _lib.dptr(uvs[m])
        d.triangle_uvs, d.texture = _lib.dptr(triangle_uvs[m]), _lib.dptr(texture[m])
        d.n_uvs = 0 if uvs[m] is None else int(uvs[m].shape[0])
        d.tex_width = 0 if texture[m] is None else int(texture[m].shape[1])
        d.tex_height = 0 if texture[m] is None else int(texture[m].shape[0])
        counts.append(T)
    outs, out_bytes = _mesh_frame_buffers(what, need, rgba, rgb_u8, depth, depth_nz)
    if records.dtype != torch.int32 or not records.is_contiguous() or tuple(records.shape) != (P, _lib.PXT_MESH_RASTER_RECORD):
        raise _lib.PxtError(f"{what}: records is a contiguous int32 [{P}, {_lib.PXT_MESH_RASTER_RECORD}] tensor "
                            f"(got {tuple(records.shape)}, {records.dtype})")
    geo = (C.c_int32 * (3 * P))(*[int(x) for x in geometry])
    off = (C.c_int64 * (4 * P))(*[int(x) for x in offsets])
    cap = (C.c_int64 * 4)(*out_bytes)
    vm = (C.c_int32 * P)(*[int(x) for x in view_mesh])
    occluder = None
    if scene is not None:
        view_scene, r_grow, occluder_offsets, occluder = scene
        occ_need = mesh_scene_planes(view_scene, r_grow, occluder_offsets, geometry, what)
        scenes = {}
        for p, s in enumerate(view_scene):
            q = scenes.setdefault(int(s), p)
            if int(s) >= 0 and not torch.equal(views[p, 12:16].view(torch.int32), views[q, 12:16].view(torch.int32)):
                raise _lib.PxtError(f"{what}: views {q} and {p} of scene {int(s)} differ in fx fy cx cy: a scene is one camera")
        occ_have = 0 if occluder is None else occluder.numel()
        if occluder is not None and (occluder.dtype != torch.uint8 or not occluder.is_contiguous()):
            raise _lib.PxtError(f"{what}: occluder is a contiguous uint8 buffer (got {occluder.dtype})")
        if occ_have < occ_need:
            raise _lib.PxtError(f"{what}: occluder holds {occ_have} bytes, the views' planes need {occ_need}")
        if occluder is not None:
            named.append((occluder, "occluder"))
    size_fn = L.pxt_mesh_render_frame_batch_workspace_bytes if scene is None else L.pxt_mesh_render_scene_batch_workspace_bytes
    bytes_needed = int(size_fn(M, (C.c_int32 * M)(*counts), P, vm, geo))
    if bytes_needed <= 0:
        raise _lib.PxtError(f"{what}: the views {list(geometry)} are not supported")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < bytes_needed:
        raise _lib.PxtError(f"{what}: workspace is a contiguous uint8 tensor of >= {bytes_needed} bytes")
    # what the kernels dereference must be memory of one device (a host pointer there is a memory fault, not an error)
    named += [(records, "records"), (workspace, "workspace")] + [(t, name) for t, name, _ in outs if t is not None]
    device = vertices[0].device
    for t, name in named:
        _lib.require_gpu(t, name)
        if t.device != device:
            raise _lib.PxtError(f"{what}: {name} is on {t.device}, vertices[0] on {device}")
    if posed is not None:
        pose_records, radii, views_out = posed
        table = mesh_view_poses(pose_records, radii, views_out, P, device, what)
        _lib.check(L.pxt_mesh_render_frame_batch_posed(
            descs, M, vm, views.data_ptr(), P, geo, off, _lib.dptr(rgba), _lib.dptr(rgb_u8), _lib.dptr(depth),
            _lib.dptr(depth_nz), cap, records.data_ptr(), workspace.data_ptr(), table, _lib.dptr(views_out),
            _stream(vertices[0])), "pxt_mesh_render_frame_batch_posed")
        return
    if scene is None:
        _lib.check(L.pxt_mesh_render_frame_batch(
            descs, M, vm, views.data_ptr(), P, geo, off, _lib.dptr(rgba), _lib.dptr(rgb_u8), _lib.dptr(depth),
            _lib.dptr(depth_nz), cap, records.data_ptr(), workspace.data_ptr(), _stream(vertices[0])),
            "pxt_mesh_render_frame_batch")
        return
    _lib.check(L.pxt_mesh_render_scene_batch(
        descs, M, vm, views.data_ptr(), P, geo, off, _lib.dptr(rgba), _lib.dptr(rgb_u8), _lib.dptr(depth),
        _lib.dptr(depth_nz), cap, (C.c_int32 * P)(*[int(x) for x in view_scene]), int(r_grow), _lib.dptr(occluder),
        occ_have, (C.c_int64 * P)(*[int(x) for x in occluder_offsets]), records.data_ptr(), workspace.data_ptr(),
        _stream(vertices[0])), "pxt_mesh_render_scene_batch")


_IMPLS = {
    "mesh_render_frame_batch": _mesh_render_frame_batch,
    "mesh_render_frame_batch_posed": _mesh_render_frame_batch_posed,
    "mesh_render_scene_batch": _mesh_render_scene_batch,
    "mask_exclude": _mask_exclude,
    "mesh_raster": _mesh_raster,
    "mesh_render_frame": _mesh_render_frame,
    "mesh_render": _mesh_render,
    "mesh_render_textured": _mesh_render_textured,
    "ngp_query": _ngp_query,
    "iso_surface_count": _iso_surface_count,
    "iso_surface_emit": _iso_surface_emit,
    "max_pairwise_distance": _max_pairwise_distance,
    "occlusion_mask": _occlusion_mask,
    "occlusion_mask_views": _occlusion_mask_views,
    "points_visible": _points_visible,
    "depth_refine": _depth_refine,
    "sensor_vsd": _sensor_vsd,
    "symmetric_pose_errors": _symmetric_pose_errors,
    "depth_agreement": _depth_agreement,
    "pose_errors": _pose_errors,
    "points_from_depth": _points_from_depth,
    "points_from_depth_views": _points_from_depth_views,
    "lm_refine": _lm_refine,
    "lm_refine_batch": _lm_refine_batch,
    "lm_information": _lm_information,
    "lm_point_report": _lm_point_report,
    "sample_sparse": _sample_sparse,
    "score_pose_hypotheses": _score_pose_hypotheses,
    "unet_forward_batch": _unet_forward_batch,
    "conv3x3_nhwc_f16": _conv3x3,
    "ngp_render": _ngp_render,
    "ngp_render_both": _ngp_render_both,
    "ngp_render_both_from_pose": _ngp_render_both_from_pose,
    "ngp_render_frame": _ngp_render_frame,
    "ngp_render_frame_batch": _ngp_render_frame_batch,
    "depth_mask": _depth_mask,
    "depth_mask_plane": _depth_mask_plane,
    "rgba_to_u8": _rgba_to_u8,
    "resize_linear": _resize_linear,
    "resize_activity": _resize_activity,
}
for _name, _fn in _IMPLS.items():
    _DEF.impl(_name, _fn, "CUDA")  # CUDA dispatch key == HIP device on torch-ROCm; nothing for CPU

ops = getattr(torch.ops, _NS)


def op_names() -> List[str]:
    return sorted(SCHEMAS)
