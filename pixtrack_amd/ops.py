"""``torch.ops.pixtrack.*``: the C-ABI entry points of libpixtrack_hip.so (include/pixtrack_hip.h)
registered as ``torch.library`` custom ops on the ROCm device (dispatch key CUDA == HIP on a
ROCm build of torch).  This is the seam SURVEY.md 8(b) / BASELINE north_star ask for: Python host
code hands ``torch.Tensor``s to the ops, the op bodies are the only place where ctypes touches the
hot path (pointers, sizes, the current HIP stream).

Reference call sites the ops stand in for:
  lm_refine            pixloc BaseRefiner.refine_pose_using_features -> opt.run per level
                       (pixtrack/localization/pixloc_pose_refiners.py:255-262)
  lm_refine_batch      (no reference counterpart) K such refinements, the objects of lock-step tracking, in one launch
  lm_information       (no reference counterpart) the LM's normal equations at a given pose, K problems per launch
  lm_point_report      (opt-in) the per-point terms of one LM iteration at a given pose, K problems per launch: what
                       DebugTracker keeps of a refinement's points at debug >= 2 (pixtrack/localization/tracker.py:26-30)
  sample_sparse        PoseTrackerRefiner.interp_sparse_observations (:327-368, interpolator :351)
  score_pose_hypotheses  (no reference counterpart) M pose hypotheses scored in one launch (relocalizer.py)
  unet_forward_batch   self.model({"image": ...}) (pixtrack/localization/feature_extractor.py:48)
  ngp_render[_both]    testbed.render(w, h, spp, True) (pixtrack/visualization/run_vis_on_poses.py:51)
  ngp_render_both_from_pose, ngp_render_frame[_batch]  the same renders with the camera derived on the device from an
                       lm_refine record, with the 8-bit planes the tracker consumes written by the last kernel, and K
                       of those for K contexts in one chain
  ngp_query            (no reference counterpart) the network's density and colour at given points (parity tests, mesh extraction)
  depth_mask[_plane]   get_mask morphology (pixtrack/pose_trackers/pixloc_tracker_r9.py:207-214), from the float Depth
                       image or from its nonzero plane
  rgba_to_u8           get_nerf_image's alpha threshold / *255 / uint8 (run_vis_on_poses.py:52-54)
  resize_linear        pixloc resize(image, size, max, "linear") (feature_extractor.py:45)
  resize_activity      (no reference counterpart) which pixels of a resized image can be non-zero: the mask the UNet's
                       constant-tile skipping reads for images above the extractor's size limit
  conv3x3_nhwc_f16     one convolution layer of that model on its own (tests, microbenchmarks)
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
  iso_surface_count, iso_surface_emit, max_pairwise_distance  (opt-in, no reference counterpart) a mesh from a lattice
                       of densities in two passes, and its diameter (mesh.py)
  mesh_raster, mesh_render[_textured]  (opt-in, no reference counterpart) depth, triangle ids and colour of a triangle
                       mesh from P views (mesh_render.py, mesh_evaluation.py)
  mesh_render_frame[_batch]  (opt-in) a tracker frame's views of one mesh, or of up to 16 meshes, in one call: a mesh
                       template in the NeRF's place (mesh_template.py)
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


# ------------------------------------------------------------------------- argument checks
# The vocabulary every op body below checks its arguments with: plain functions that raise PxtError
# with "<op>: <argument> is <expected> (got ...)".  Inside a body the order is: lengths and counts, then dtype / shape /
# contiguity, then the workspace's size, then devices.
_SENSOR_DTYPES = (torch.uint16, torch.int16)  # raw depth counts; int16 holds the same bits
_ANY3 = (None, None, None)


def _dense(op, t, name, dtype=torch.float32, shape=None, where=""):
    """``t`` is a contiguous tensor of ``dtype`` (one, or a tuple of them) and of ``shape``, where an entry of None
    stands for any extent (the pattern still fixes the rank) -> t.  ``where`` (a string, or a tuple of parts) follows
    the name in the message.  The passing path is kept short: it runs dozens of times per launch on a frame's
    critical path."""
    if (t.dtype == dtype or (dtype.__class__ is tuple and t.dtype in dtype)) and t.is_contiguous():
        if shape is None:
            return t
        have = t.shape
        if len(have) == len(shape):
            for d, s in zip(have, shape):
                if s is not None and d != s:
                    break
            else:
                return t
    dtypes = " or ".join(str(d)[6:] for d in (dtype if dtype.__class__ is tuple else (dtype,)))
    want = "" if shape is None else " [" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
    where = "".join(str(w) for w in where) if where.__class__ is tuple else where
    raise _lib.PxtError(f"{op}: {name}{where} is a contiguous {dtypes}{want} tensor (got {tuple(t.shape)}, {t.dtype}, "
                        f"contiguous={t.is_contiguous()})")


def _point_mask(op, t, n, name="point_mask"):
    """A point mask is None or contiguous uint8 with one byte per point: the kernels read ``n`` bytes of it."""
    if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != n):
        raise _lib.PxtError(f"{op}: {name} is contiguous uint8 [n_points = {n}] (got {tuple(t.shape)}, {t.dtype})")


def _sensor(op, t, name, shape):
    return _dense(op, t, name, _SENSOR_DTYPES, shape)


def _shifts(op, shift, pairs=1):
    if len(shift) != 2 * pairs or any(abs(int(v)) > 32767 for v in shift):
        raise _lib.PxtError(f"{op}: shift is (shift_x, shift_y){' per view' if pairs > 1 else ''}, each within +-32767 "
                            f"(got {list(shift)})")


def _radii(op, radii):
    if len(radii) != 2 or min(int(r) for r in radii) < 0 or int(radii[0]) + int(radii[1]) > _lib.PXT_OCCLUSION_MAX_RADIUS:
        raise _lib.PxtError(f"{op}: radii are (r_open, r_grow) >= 0 with r_open + r_grow <= "
                            f"{_lib.PXT_OCCLUSION_MAX_RADIUS} (got {list(radii)})")


def _record(op, t, name, dtype, count, device, shape=None):
    """A record the host reads: ``count`` contiguous words of ``dtype`` at least (or exactly ``shape``), in memory of
    ``device`` or in pinned host memory - a kernel on ``device`` stores to it -> its address."""
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < count or (shape is not None and tuple(t.shape) != shape) \
            or not ((t.is_cuda and t.device == device) or t.is_pinned()):
        size = f"{count} contiguous {str(dtype)[6:]} words" if shape is None else f"a contiguous {str(dtype)[6:]} {list(shape)}"
        raise _lib.PxtError(f"{op}: {name} needs {size} in memory of {device} or pinned host memory (got "
                            f"{tuple(t.shape)}, {t.dtype}, {t.device})")
    return t.data_ptr()


def _workspace(op, workspace, need, unsupported, any_dtype=""):
    """``need`` = what the op's size query answered; <= 0 says that it does not support the problem.  Two forms: a
    contiguous uint8 tensor of that many bytes, or (``any_dtype`` = what to call it) a tensor of any dtype with that
    many - all the LM and depth-refinement ops ever asked."""
    if need <= 0:
        raise _lib.PxtError(f"{op}: {unsupported}")
    if any_dtype:
        if workspace.numel() * workspace.element_size() < need:
            raise _lib.PxtError(f"{op}: {any_dtype} holds {workspace.numel() * workspace.element_size()} bytes, {need} needed")
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.PxtError(f"{op}: workspace is a contiguous uint8 tensor of >= {need} bytes (got {workspace.numel()}, "
                            f"{workspace.dtype})")


def _one_device(op, anchor, named, where=""):
    """Every tensor of ``named`` = (tensor or None, name) pairs lives on the ROCm device of ``anchor``.  The
    dispatcher only guarantees that SOME argument is a device tensor, and a kernel dereferences them all: a host
    pointer or another device's there is a memory fault, not an error."""
    index = anchor.get_device()  # (-1: host memory; comparing indices is the cheap way to pass)
    for t, name in named:
        if t is None or (t.get_device() == index and index >= 0):
            continue
        _lib.require_gpu(t, name)
        if t.device != anchor.device:
            raise _lib.PxtError(f"{op}: {name}{where} is on {t.device}, not on {anchor.device}")


# ------------------------------------------------------------------------------------------- LM
_LM_HEADER = 16 + _lib.PXT_MAX_LEVELS  # the floats of an LM output record ahead of its iteration log


def _lm_conf(pad, loss, loss_alpha, loss_scale, min_valid=0, num_iters=0, grad_stop=0.0, dt_stop=0.0, dR_stop=0.0,
             n_workgroups=0, spin_limit=0, lm_path=0):
    conf = _lib.LmConf()
    conf.num_iters, conf.pad, conf.loss = int(num_iters), int(pad), int(loss)
    conf.loss_alpha, conf.loss_scale = float(loss_alpha), float(loss_scale)
    conf.grad_stop, conf.dt_stop, conf.dR_stop = float(grad_stop), float(dt_stop), float(dR_stop)
    conf.min_valid, conf.n_workgroups, conf.spin_limit = int(min_valid), int(n_workgroups), int(spin_limit)
    conf.path = int(lm_path)
    return conf


def _lm_level(op, lv, where, fmap, table, n, channels, camera, ndist, lambdas=None, field="fref"):
    """One level: the query map [h, w, cstride] and a table [n, cstride] of per-point records - the reference
    records, or sample_sparse's output - checked and written into the level record ``lv`` (pxt_lm_level,
    pxt_sample_level, pxt_reloc_map; ``field``: where the table's pointer goes, None for a record without one)."""
    _dense(op, fmap, "fmap", torch.float32, _ANY3, where)
    h, w, cs = fmap.shape
    if table.shape != (n, cs) or table.dtype != torch.float32 or not table.is_contiguous():  # (per level, K x levels per
        _dense(op, table, field or "fref", torch.float32, (n, cs), where)                    # launch: refusing is _dense's)
    lv.fmap, lv.h, lv.w, lv.C, lv.cstride = fmap.data_ptr(), h, w, int(channels), cs
    if field is not None:
        setattr(lv, field, table.data_ptr())
    lv.cam[:] = camera
    lv.ndist = int(ndist)
    if lambdas is not None:
        lv.lambda_[:] = lambdas


def _lm_camera(op, conv27, slots, cam_out, device):
    """pxt_lm_camera: the kernel's epilogue also derives the next render's camera and stores it in up to two renderer
    slots (0: none) and in ``cam_out`` (13 floats the host reads, or None)."""
    cam = _lib.LmCamera()
    cam.conv27[:] = [float(x) for x in conv27]
    for k in range(2):
        cam.cam_slot[k] = (int(slots[k]) or None) if k < len(slots) else None
    cam.cam_out13 = None if cam_out is None else _record(op, cam_out, "cam_out", torch.float32, 13, device)
    return cam


def _lm_record(op, record, name, n_levels, num_iters, want_log, device):
    """An LM output record: the header, then the iteration log when wanted -> the addresses of the two."""
    log = n_levels * int(num_iters) * _lib.PXT_LM_LOG_STRIDE if want_log else 0
    out = _record(op, record, name, torch.float32, _LM_HEADER + log, device)
    return out, out + 4 * _LM_HEADER if want_log else None


def _lm_refine(p3d, point_mask, fmaps, frefs, channels, cameras, ndist, lambdas, T_init, num_iters, pad, loss,
               loss_alpha, loss_scale, grad_stop, dt_stop, dR_stop, min_valid, n_workgroups, record, workspace,
               want_log, spin_limit=0, cam_conv=None, cam_slots=None, cam_out=None, lm_path=0, guard_level=-1,
               guard_flags=None, guard_geo=None):
    """``guard_level`` (index in execution order), ``guard_flags`` (uint8 device tensor) and ``guard_geo`` = [tile_rows,
    tiles_per_row, tile_x0, tile_y0]: that level's map holds data only in the tiles whose flag is 1
    (pxt_lm_tile_guard, pxt_lm_refine_guarded); a launch that reads another tile ends with status PXT_E_GUARD."""
    op = "lm_refine"
    n_levels = len(fmaps)
    if not (1 <= n_levels <= _lib.PXT_MAX_LEVELS) or len(frefs) != n_levels or len(channels) != n_levels:
        raise _lib.PxtError(f"{op}: {n_levels} levels (1..{_lib.PXT_MAX_LEVELS}), {len(frefs)} frefs, {len(channels)} channels")
    if len(cameras) != 10 * n_levels or len(lambdas) != 6 * n_levels or len(ndist) != n_levels or len(T_init) != 12:
        raise _lib.PxtError(f"{op}: cameras need 10, lambdas 6 floats per level, T_init 12 floats")
    n = int(_dense(op, p3d, "p3d").shape[0])
    arr = (_lib.LmLevel * n_levels)()
    for i in range(n_levels):
        _lm_level(op, arr[i], (" of level ", i), fmaps[i], frefs[i], n, channels[i], cameras[10 * i:10 * i + 10], ndist[i],
                  lambdas[6 * i:6 * i + 6])
    guard = None
    if guard_flags is not None:
        if guard_geo is None or len(guard_geo) != 4:
            raise _lib.PxtError(f"{op}: guard_geo holds tile_rows, tiles_per_row, tile_x0, tile_y0")
        gl, flags = int(guard_level), guard_flags
        tile_rows, tiles_per_row, tile_x0, tile_y0 = (int(x) for x in guard_geo)
        if not (0 <= gl < n_levels) or flags.dtype != torch.uint8 or not flags.is_cuda or not flags.is_contiguous():
            raise _lib.PxtError(f"{op}: tile_guard names a level and a contiguous uint8 device tensor of flags")
        rows = (tile_y0 + arr[gl].h - 1) // max(tile_rows, 1) + 1
        if tile_rows < 1 or flags.numel() < rows * tiles_per_row:
            raise _lib.PxtError(f"{op}: tile_guard needs {rows} x {tiles_per_row} flags, got {flags.numel()}")
        guard = _lib.LmTileGuard(gl, flags.data_ptr(), tile_rows, tiles_per_row, tile_x0, tile_y0)
    conf = _lm_conf(pad, loss, loss_alpha, loss_scale, min_valid, num_iters, grad_stop, dt_stop, dR_stop, n_workgroups,
                    spin_limit, lm_path)
    out, log = _lm_record(op, record, "record", n_levels, num_iters, want_log, p3d.device)
    _point_mask(op, point_mask, n)
    cam = None
    if cam_conv is not None:  # the kernel's epilogue also derives the next render's camera
        slots = cam_slots or []
        if len(cam_conv) != 27:
            raise _lib.PxtError(f"{op}: cam_conv holds 27 doubles (Testbed.pose_conversion)")
        if len(slots) > 2 or (not slots and cam_out is None):
            raise _lib.PxtError(f"{op}: at most two camera slots; at least one slot or cam_out")
        cam = _lm_camera(op, cam_conv, slots, cam_out, p3d.device)
    T0 = (C.c_float * 12)(*[float(x) for x in T_init])
    # (pxt_lm_refine and pxt_lm_refine_cam are this entry with no camera and no guard)
    _lib.check(_lib.lib().pxt_lm_refine_guarded(
        p3d.data_ptr(), _lib.dptr(point_mask), n, arr, n_levels, T0, C.byref(conf), out, log, workspace.data_ptr(),
        None if cam is None else C.byref(cam), None if guard is None else C.byref(guard), _stream(p3d)),
        "pxt_lm_refine_guarded")


def _lm_refine_batch(p3d, point_masks, n_levels, fmaps, frefs, channels, cameras, ndist, lambdas, T_init, num_iters, pad,
                     loss, loss_alpha, loss_scale, grad_stop, dt_stop, dR_stop, min_valid, n_workgroups, records,
                     workspaces, batch_workspace, want_log, spin_limit=0, cam_conv=None, cam_slots=None, cam_outs=None,
                     lm_path=0, cam_enabled=None):
    op = "lm_refine_batch"
    L = _lib.lib()
    K = len(p3d)
    n_levels = [int(x) for x in n_levels]
    nl_tot = sum(n_levels)
    if not (1 <= K <= _lib.PXT_LM_MAX_BATCH) or len(n_levels) != K or len(records) != K or len(workspaces) != K \
            or len(point_masks) != K or len(T_init) != 12 * K:
        raise _lib.PxtError(f"{op}: {K} problems (1..{_lib.PXT_LM_MAX_BATCH}) need one record, workspace, mask slot "
                            "and 12 pose floats each")
    if len(fmaps) != nl_tot or len(frefs) != nl_tot or len(channels) != nl_tot or len(cameras) != 10 * nl_tot \
            or len(lambdas) != 6 * nl_tot or len(ndist) != nl_tot:
        raise _lib.PxtError(f"{op}: per level one fmap, fref, channel count, ndist, 10 camera and 6 lambda floats")
    conf = _lm_conf(pad, loss, loss_alpha, loss_scale, min_valid, num_iters, grad_stop, dt_stop, dR_stop, n_workgroups,
                    spin_limit, lm_path)
    if cam_conv is not None and (len(cam_conv) != 27 * K or len(cam_slots or []) != 2 * K
                                 or (cam_outs is not None and len(cam_outs) != K)):
        raise _lib.PxtError(f"{op}: cam_conv holds 27 doubles, cam_slots 2 pointers (0 = none) per problem")
    device = p3d[0].device
    probs = (_lib.LmProblem * K)()
    keep = []  # ctypes records the problem array points to
    li = 0
    for k in range(K):
        where, nl, mk = f" of problem {k}", n_levels[k], point_masks[k]
        n = int(_dense(op, p3d[k], "p3d" + where).shape[0])
        if not (1 <= nl <= _lib.PXT_MAX_LEVELS):
            raise _lib.PxtError(f"{op}: problem {k} has {nl} levels")
        arr = (_lib.LmLevel * nl)()
        for i in range(nl):
            _lm_level(op, arr[i], (where, " level ", i), fmaps[li], frefs[li], n, channels[li], cameras[10 * li:10 * li + 10],
                      ndist[li], lambdas[6 * li:6 * li + 6])
            li += 1
        q = probs[k]
        q.out, q.log = _lm_record(op, records[k], f"record {k}", nl, num_iters, want_log, device)
        _point_mask(op, mk, n, "point_mask" + where)
        T0 = (C.c_float * 12)(*[float(x) for x in T_init[12 * k:12 * k + 12]])
        q.p3d, q.point_mask, q.n_points = p3d[k].data_ptr(), _lib.dptr(mk), n
        q.levels_host, q.n_levels, q.T_init_host = arr, nl, T0
        q.workspace = workspaces[k].data_ptr()
        cam = None
        if cam_conv is not None and (cam_enabled is None or cam_enabled[k]):
            cam = _lm_camera(op, cam_conv[27 * k:27 * k + 27], cam_slots[2 * k:2 * k + 2],
                             None if cam_outs is None else cam_outs[k], device)
            q.cam_host = C.pointer(cam)
        keep.append((arr, T0, cam))
    # (K is in range: the size query cannot answer "not supported" here, nor in the two bodies below that pass any_dtype)
    _workspace(op, batch_workspace, int(L.pxt_lm_batch_workspace_bytes(K)), f"{K} problems are not supported",
               any_dtype="batch_workspace")
    _lib.check(L.pxt_lm_refine_batch(probs, K, C.byref(conf), batch_workspace.data_ptr(), _stream(p3d[0])),
               "pxt_lm_refine_batch")


def _lm_evaluate(op, problems, conf, records, workspace, *, entry, workspace_bytes, Problem, max_problems, record_name,
                 record_field, n_record, own=None, extras=(), extra_names=""):
    """The K (points, level, pose) problems of lm_information / lm_point_report: checked, packed and launched through
    ``entry``.  ``problems`` = the ops' common per-problem arguments in schema order (p3d ... pose_is_lm_record),
    ``conf`` = (pad, loss, loss_alpha, loss_scale, min_valid); problem k's record goes into ``record_field``.
    ``own(q, k, n)`` checks and sets what only ``op`` has (one list per problem in ``extras``) and returns the
    (tensor, name) pairs the kernel dereferences besides."""
    p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record = problems
    K = len(p3d)
    if not (1 <= K <= max_problems):
        raise _lib.PxtError(f"{op}: {K} problems (1..{max_problems})")
    if any(len(x) != K for x in (point_masks, fmaps, frefs, channels, ndist, poses, records, *extras)) \
            or len(cameras) != 10 * K:
        raise _lib.PxtError(f"{op}: per problem one mask slot, map, reference table, channel count, ndist, pose, "
                            f"{extra_names}{record_name} and 10 camera floats")
    _one_device(op, workspace, [(workspace, "workspace")])
    probs = (Problem * K)()
    for k in range(K):
        where, q, mk = f" of problem {k}", probs[k], point_masks[k]
        n = int(_dense(op, p3d[k], "p3d" + where, shape=(None, 3)).shape[0])
        _lm_level(op, q.level, where, fmaps[k], frefs[k], n, channels[k], cameras[10 * k:10 * k + 10], ndist[k])
        _point_mask(op, mk, n, "point_mask" + where)
        more = own(q, k, n) if own is not None else ()
        # (the pose and the record may also be pinned host memory)
        _one_device(op, workspace, [(p3d[k], "p3d"), (fmaps[k], "fmap"), (frefs[k], "fref"), (mk, "point_mask"), *more], where)
        q.pose = _record(op, poses[k], f"pose {k}", torch.float32, 16 if pose_is_lm_record else 12, workspace.device)
        setattr(q, record_field, _record(op, records[k], f"{record_name} {k}", torch.float32, n_record, workspace.device))
        q.p3d, q.point_mask, q.n_points = p3d[k].data_ptr(), _lib.dptr(mk), n
        q.pose_is_lm_record = int(bool(pose_is_lm_record))
    _workspace(op, workspace, int(workspace_bytes(K)), f"{K} problems are not supported", any_dtype="workspace")
    _lib.check(entry(probs, K, C.byref(_lm_conf(*conf)), workspace.data_ptr(), _stream(workspace)), entry.__name__)


def _lm_information(p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record, pad, loss,
                    loss_alpha, loss_scale, min_valid, records, workspace):
    L = _lib.lib()
    _lm_evaluate("lm_information", (p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record),
                 (pad, loss, loss_alpha, loss_scale, min_valid), records, workspace, entry=L.pxt_lm_information,
                 workspace_bytes=L.pxt_lm_information_workspace_bytes, Problem=_lib.LmInfoProblem,
                 max_problems=_lib.PXT_LM_INFO_MAX_PROBLEMS, record_name="record", record_field="out",
                 n_record=_lib.PXT_LM_INFO_RECORD)


def _lm_point_report(p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record, pad, loss,
                     loss_alpha, loss_scale, min_valid, inlier_weights, points, summaries, workspace):
    def own(q, k, n):
        out = points[k]
        if out is not None:
            _dense("lm_point_report", out, f"points of problem {k}", shape=(n, _lib.PXT_LM_POINT_RECORD))
        q.inlier_weight, q.points = float(inlier_weights[k]), _lib.dptr(out)
        return ((out, "points"),)

    L = _lib.lib()
    _lm_evaluate("lm_point_report", (p3d, point_masks, fmaps, frefs, channels, cameras, ndist, poses, pose_is_lm_record),
                 (pad, loss, loss_alpha, loss_scale, min_valid), summaries, workspace, entry=L.pxt_lm_point_report,
                 workspace_bytes=L.pxt_lm_point_report_workspace_bytes, Problem=_lib.LmReportProblem,
                 max_problems=_lib.PXT_LM_REPORT_MAX_PROBLEMS, record_name="summary", record_field="summary",
                 n_record=_lib.PXT_LM_REPORT_SUMMARY, own=own, extras=(inlier_weights, points),
                 extra_names="inlier weight, points slot, ")


# ------------------------------------------------------------------------------------ sampling
def _sample_sparse(p3d, T, fmaps, channels, cameras, ndist, pad, normalize, outs, valid, windows=None):
    op = "sample_sparse"
    n_levels = len(fmaps)
    if len(outs) != n_levels or len(cameras) != 10 * n_levels or len(T) != 12:
        raise _lib.PxtError(f"{op}: one out tensor and 10 camera floats per level, T of 12 floats")
    if windows is not None and len(windows) != 4 * n_levels:
        raise _lib.PxtError(f"{op}: windows holds (x0, y0, full_w, full_h) per level")
    n = int(_dense(op, p3d, "p3d").shape[0])
    arr = (_lib.SampleLevel * n_levels)()
    for i in range(n_levels):
        _lm_level(op, arr[i], (" of level ", i), fmaps[i], outs[i], n, channels[i], cameras[10 * i:10 * i + 10], ndist[i],
                  field="out")
        if windows is not None:  # (x0, y0, full_w, full_h) per level: the map is a window of the full level
            arr[i].x0, arr[i].y0, arr[i].full_w, arr[i].full_h = (int(x) for x in windows[4 * i:4 * i + 4])
    if valid.dtype != torch.uint8 or valid.numel() != n:
        raise _lib.PxtError(f"{op}: valid must be uint8 [n_points]")
    T12 = (C.c_float * 12)(*[float(x) for x in T])
    _lib.check(_lib.lib().pxt_sample_sparse(p3d.data_ptr(), n, T12, arr, n_levels, int(pad), int(bool(normalize)),
                                            valid.data_ptr(), _stream(p3d)), "pxt_sample_sparse")


# ------------------------------------------------------------------------------ relocalisation
def _score_pose_hypotheses(fmap, channels, camera, ndist, p3d, fref, valid, poses, ranges, pad, loss, loss_alpha, loss_scale,
                           out):
    op = "score_pose_hypotheses"
    if len(camera) != 10:
        raise _lib.PxtError(f"{op}: camera holds 10 floats")
    n = int(_dense(op, p3d, "p3d", shape=(None, 3)).shape[0])
    mp = _lib.RelocMap()
    _lm_level(op, mp, "", fmap, fref, n, channels, camera, ndist, field=None)
    _point_mask(op, valid, n, "valid")
    M = int(_dense(op, poses, "poses", shape=(None, 12)).shape[0])
    if M < 1:
        raise _lib.PxtError(f"{op}: poses is {tuple(poses.shape)}, expected [M >= 1, 12]")
    _dense(op, ranges, "ranges", torch.int32, (M, 2))
    if _dense(op, out, "out").numel() != 4 * M:
        raise _lib.PxtError(f"{op}: out holds 4 floats per hypothesis")
    _one_device(op, fmap, [(fmap, "fmap"), (p3d, "p3d"), (fref, "fref"), (valid, "valid"), (poses, "poses"),
                           (ranges, "ranges"), (out, "out")])
    bank = _lib.RelocBank(p3d.data_ptr(), fref.data_ptr(), _lib.dptr(valid), n)
    conf = _lm_conf(pad, loss, loss_alpha, loss_scale)
    _lib.check(_lib.lib().pxt_score_pose_hypotheses(C.byref(mp), C.byref(bank), poses.data_ptr(), ranges.data_ptr(), M,
                                                    C.byref(conf), out.data_ptr(), _stream(fmap)),
               "pxt_score_pose_hypotheses")


# ---------------------------------------------------------------------------------------- UNet
def _unet_points(images, n, sample_p3d, sample_pose_camera, sample_ints):
    points = None
    if sample_p3d is not None:
        if n > 2 or sample_pose_camera is None or sample_ints is None or len(sample_pose_camera) != 22 or len(sample_ints) < 6:
            raise _lib.PxtError("unet_forward_batch: sample points go with one image or a pair, 22 floats (pose, camera) "
                                "and 6 ints (ndist, pad, x0, y0, full_w, full_h)")
        _dense("unet_forward_batch", sample_p3d, "sample_p3d", shape=(None, 3))
        _one_device("unet_forward_batch", images[0], [(sample_p3d, "sample_p3d")])
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
        _dense("unet_forward_batch", o, "out map")
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


def _ngp_render(ctx, view, width, height, spp, mode, out, stats):
    _dense("ngp_render", out, "out", shape=(height, width, 4))
    v = _view(view, width, height, spp, mode)
    _lib.check(_lib.lib().pxt_ngp_render(ctx, C.byref(v), out.data_ptr(), _lib.dptr(stats), _stream(out)),
               "pxt_ngp_render")


def _ngp_render_both(ctx, view, width, height, spp, rgba, depth, stats):
    _dense("ngp_render_both", rgba, "rgba", shape=(height, width, 4))
    _dense("ngp_render_both", depth, "depth", shape=(height, width, 4))
    v = _view(view, width, height, spp, 0)
    _lib.check(_lib.lib().pxt_ngp_render_both(ctx, C.byref(v), rgba.data_ptr(), depth.data_ptr(), _lib.dptr(stats),
                                              _stream(rgba)), "pxt_ngp_render_both")


def _ngp_render_both_from_pose(ctx, view, pose_record, conv, width, height, spp, mode, rgba, depth, cam_out, stats):
    """pxt_ngp_render_both with the camera derived ON THE DEVICE from `pose_record` (pinned float32, >= 12 floats:
    the record pxt_lm_refine writes), so that the render can be enqueued behind the LM launch.  `cam_out`: pinned
    float32 [>= 13], receives the camera + a completion word.  `depth` given: Shade + Depth in one march (`mode`
    ignored); None: one render in `mode` (0 Shade, 1 Depth) into `rgba`."""
    _dense("ngp_render_both_from_pose", rgba, "rgba", shape=(height, width, 4))
    if depth is not None:
        _dense("ngp_render_both_from_pose", depth, "depth", shape=(height, width, 4))
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
            _dense("ngp_render_frame", t, what, shape=(height, width, 4))
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
                _dense("ngp_render_frame_batch", df, "depth_float", shape=(h, w, 4))
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
    _dense("depth_mask", depth_rgba, "depth_rgba")
    H, W = int(depth_rgba.shape[0]), int(depth_rgba.shape[1])
    _mask_out(mask, H, W, depth_rgba, "depth_mask")
    if scratch.numel() < 2 * H * W:
        raise _lib.PxtError("depth_mask: scratch holds 2*H*W bytes")
    _lib.check(_lib.lib().pxt_depth_mask(depth_rgba.data_ptr(), H, W, int(n_erode), int(n_dilate), mask.data_ptr(),
                                         scratch.data_ptr(), _stream(depth_rgba)), "pxt_depth_mask")


def _rgba_to_u8(rgba, alpha_thresh, out):
    _dense("rgba_to_u8", rgba, "rgba")
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3):
        raise _lib.PxtError("rgba_to_u8: out is uint8 [H, W, 3]")
    _lib.check(_lib.lib().pxt_rgba_to_u8(rgba.data_ptr(), H, W, float(alpha_thresh), out.data_ptr(), _stream(rgba)),
               "pxt_rgba_to_u8")


def _resize_linear(src, dst):
    _dense("resize_linear", src, "src")
    _dense("resize_linear", dst, "dst")
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
    op = "points_from_depth"
    L = _lib.lib()
    _dense(op, depth, "depth", shape=(None, None, 4))
    H, W, n_max = int(depth.shape[0]), int(depth.shape[1]), int(n_max)
    if len(xform) != 12:
        raise _lib.PxtError(f"{op}: xform holds 12 floats ([M | b], 3 x 4 row-major)")
    if int(erode) not in (0, 1, 2) or n_max < 1:
        raise _lib.PxtError(f"{op}: erode is 0, 1 or 2 and n_max >= 1")
    _dense(op, p3d, "p3d", shape=(n_max, 3))
    _point_mask(op, slot_valid, n_max, "slot_valid")  # (one byte per slot in any shape; the schema rules None out)
    rec = _record(op, record, "record", torch.int32, 4, depth.device)
    _workspace(op, workspace, int(L.pxt_points_from_depth_workspace_bytes(W, H)), f"a {W} x {H} image is not supported")
    _one_device(op, depth, [(depth, "depth"), (p3d, "p3d"), (slot_valid, "slot_valid"), (workspace, "workspace")])
    xf = (C.c_float * 12)(*[float(x) for x in xform])
    _lib.check(L.pxt_points_from_depth(depth.data_ptr(), W, H, xf, float(focal), float(depth_scale), float(min_alpha),
                                       int(erode), n_max, p3d.data_ptr(), slot_valid.data_ptr(), rec,
                                       workspace.data_ptr(), _stream(depth)), "pxt_points_from_depth")


def _points_from_depth_views(depth, views, min_alpha, erode, n_max, p3d, slot_valid, record, workspace):
    op = "points_from_depth_views"
    L = _lib.lib()
    K, n_max = len(depth), int(n_max)
    if not (1 <= K <= _lib.PXT_POINTS_MAX_VIEWS):
        raise _lib.PxtError(f"{op}: 1..{_lib.PXT_POINTS_MAX_VIEWS} depth planes (got {K})")
    sizes = []
    for k, d in enumerate(depth):
        _dense(op, d, f"depth[{k}]", shape=(None, None, 4))
        sizes += [int(d.shape[1]), int(d.shape[0])]
    if len(views) != K * _lib.PXT_MESH_VIEW:
        raise _lib.PxtError(f"{op}: views holds {_lib.PXT_MESH_VIEW} floats per plane ({K * _lib.PXT_MESH_VIEW}; got "
                            f"{len(views)})")
    if int(erode) not in (0, 1, 2) or n_max < 1:
        raise _lib.PxtError(f"{op}: erode is 0, 1 or 2 and n_max >= 1")
    _dense(op, p3d, "p3d", shape=(K, n_max, 3))
    _dense(op, slot_valid, "slot_valid", torch.uint8, (K, n_max))
    rec = _record(op, record, "record", torch.int32, 0, depth[0].device, shape=(K, 4))
    size_arr = (C.c_int32 * (2 * K))(*sizes)
    _workspace(op, workspace, int(L.pxt_points_from_depth_views_workspace_bytes(K, size_arr)),
               f"planes of {list(zip(sizes[0::2], sizes[1::2]))} are not supported")
    _one_device(op, depth[0], [(d, f"depth[{k}]") for k, d in enumerate(depth)]
                + [(p3d, "p3d"), (slot_valid, "slot_valid"), (workspace, "workspace")])
    planes = (C.c_void_p * K)(*[d.data_ptr() for d in depth])
    vf = (C.c_float * len(views))(*[float(x) for x in views])
    _lib.check(L.pxt_points_from_depth_views(planes, size_arr, vf, K, float(min_alpha), int(erode), n_max, p3d.data_ptr(),
                                             slot_valid.data_ptr(), rec, workspace.data_ptr(), _stream(depth[0])),
               "pxt_points_from_depth_views")


def _pose_errors(vertices, rel_poses, want_adds, records, workspace):
    op = "pose_errors"
    L = _lib.lib()
    V = int(_dense(op, vertices, "vertices", shape=(None, 3)).shape[0])
    F = int(_dense(op, rel_poses, "rel_poses", shape=(None, 12)).shape[0])
    _dense(op, records, "records", shape=(F, _lib.PXT_POSE_ERR_RECORD))
    _workspace(op, workspace, int(L.pxt_pose_errors_workspace_bytes(F, V)),
               f"{F} frames x {V} vertices is not supported (1..65535 frames, 1..2^20 vertices)")
    _one_device(op, vertices, [(vertices, "vertices"), (rel_poses, "rel_poses"), (records, "records"),
                               (workspace, "workspace")])
    _lib.check(L.pxt_pose_errors(vertices.data_ptr(), V, rel_poses.data_ptr(), F, int(bool(want_adds)), records.data_ptr(),
                                 workspace.data_ptr(), _stream(vertices)), "pxt_pose_errors")


def _depth_pairs(op, depth_est, depth_gt):
    """The P pairs of Depth renders depth_agreement and sensor_vsd compare -> (P, H, W)."""
    _dense(op, depth_est, "depth_est", shape=(None, None, None, 4))
    _dense(op, depth_gt, "depth_gt", shape=tuple(depth_est.shape))
    return (int(x) for x in depth_est.shape[:3])


def _depth_agreement(depth_est, depth_gt, min_alpha, tq, records, workspace):
    op = "depth_agreement"
    L = _lib.lib()
    P, H, W = _depth_pairs(op, depth_est, depth_gt)
    if not (1 <= len(tq) <= _lib.PXT_DEPTH_AGREE_MAX_TAUS):
        raise _lib.PxtError(f"{op}: {len(tq)} thresholds (1..{_lib.PXT_DEPTH_AGREE_MAX_TAUS})")
    _dense(op, records, "records", torch.int32, (P, _lib.PXT_DEPTH_AGREE_RECORD))
    _workspace(op, workspace, int(L.pxt_depth_agreement_workspace_bytes(P, W, H)),
               f"{P} pairs of {W} x {H} are not supported (1..65535 pairs, 1..2^28 pixels)")
    _one_device(op, depth_est, [(depth_est, "depth_est"), (depth_gt, "depth_gt"), (records, "records"),
                                (workspace, "workspace")])
    tqs = (C.c_float * len(tq))(*[float(x) for x in tq])
    _lib.check(L.pxt_depth_agreement(depth_est.data_ptr(), depth_gt.data_ptr(), P, W, H, float(min_alpha), tqs, len(tq),
                                     records.data_ptr(), workspace.data_ptr(), _stream(depth_est)), "pxt_depth_agreement")


def _symmetric_pose_errors(vertices, syms, frames, records, workspace):
    op = "symmetric_pose_errors"
    L = _lib.lib()
    V = int(_dense(op, vertices, "vertices", shape=(None, 3)).shape[0])
    S = int(_dense(op, syms, "syms", shape=(None, 12)).shape[0])
    F = int(_dense(op, frames, "frames", shape=(None, _lib.PXT_SYM_ERR_FRAME)).shape[0])
    _dense(op, records, "records", shape=(F, _lib.PXT_SYM_ERR_RECORD))
    _workspace(op, workspace, int(L.pxt_symmetric_pose_errors_workspace_bytes(F, S, V)),
               f"{F} frames x {S} symmetries x {V} vertices is not supported (1..65535 frames, "
               f"1..{_lib.PXT_SYM_ERR_MAX_SYMS} symmetries, 1..2^20 vertices)")
    _one_device(op, vertices, [(vertices, "vertices"), (syms, "syms"), (frames, "frames"), (records, "records"),
                               (workspace, "workspace")])
    _lib.check(L.pxt_symmetric_pose_errors(vertices.data_ptr(), V, syms.data_ptr(), S, frames.data_ptr(), F,
                                           records.data_ptr(), workspace.data_ptr(), _stream(vertices)),
               "pxt_symmetric_pose_errors")


def _sensor_vsd(depth_est, depth_gt, sensor, ray, shift, min_alpha, sensor_q, delta_q, tq, records, workspace):
    op = "sensor_vsd"
    L = _lib.lib()
    P, H, W = _depth_pairs(op, depth_est, depth_gt)
    _sensor(op, sensor, "sensor", (P, H, W))
    if ray is not None:
        _dense(op, ray, "ray", shape=(H, W))
    _shifts(op, shift)
    if not (1 <= len(tq) <= _lib.PXT_SENSOR_VSD_MAX_TAUS):
        raise _lib.PxtError(f"{op}: {len(tq)} thresholds (1..{_lib.PXT_SENSOR_VSD_MAX_TAUS})")
    _dense(op, records, "records", torch.int32, (P, _lib.PXT_SENSOR_VSD_RECORD))
    _workspace(op, workspace, int(L.pxt_sensor_vsd_workspace_bytes(P, W, H)),
               f"{P} pairs of {W} x {H} are not supported (1..65535 pairs, 1..2^28 pixels)")
    _one_device(op, depth_est, [(depth_est, "depth_est"), (depth_gt, "depth_gt"), (sensor, "sensor"), (records, "records"),
                                (workspace, "workspace"), (ray, "ray")])
    tqs = (C.c_float * len(tq))(*[float(x) for x in tq])
    _lib.check(L.pxt_sensor_vsd(depth_est.data_ptr(), depth_gt.data_ptr(), sensor.data_ptr(), _lib.dptr(ray), P, W, H,
                                int(shift[0]), int(shift[1]), float(min_alpha), float(sensor_q), float(delta_q), tqs,
                                len(tq), records.data_ptr(), workspace.data_ptr(), _stream(depth_est)), "pxt_sensor_vsd")


def _depth_refine(p3d, point_masks, sensors, sensor_scales, cameras, ndist, poses, pose_is_lm_record, priors, num_iters,
                  pad, loss, loss_alpha, loss_scale, lambdas, max_residual, max_edge, grad_stop, dt_stop, dR_stop,
                  min_valid, records, logs, codes, workspace):
    op = "depth_refine"
    L = _lib.lib()
    K = len(p3d)
    if not (1 <= K <= _lib.PXT_DEPTH_MAX_PROBLEMS):
        raise _lib.PxtError(f"{op}: {K} problems (1..{_lib.PXT_DEPTH_MAX_PROBLEMS})")
    if any(len(x) != K for x in (point_masks, sensors, sensor_scales, ndist, poses, records, logs, codes)) \
            or len(cameras) != 10 * K or len(priors) != 21 * K or len(lambdas) != 6:
        raise _lib.PxtError(f"{op}: per problem one mask slot, sensor image, scale, ndist, pose, record, log slot, "
                            "codes slot, 10 camera floats and 21 prior floats; 6 lambdas")
    if not (0 <= int(num_iters) <= _lib.PXT_DEPTH_MAX_ITERS):
        raise _lib.PxtError(f"{op}: num_iters {num_iters} (0..{_lib.PXT_DEPTH_MAX_ITERS})")
    _one_device(op, workspace, [(workspace, "workspace")])
    dev = workspace.device
    rows = int(num_iters)
    probs = (_lib.DepthProblem * K)()
    for k in range(K):
        where, mk, sen, lg, cd = f" of problem {k}", point_masks[k], sensors[k], logs[k], codes[k]
        n = int(_dense(op, p3d[k], "p3d" + where, shape=(None, 3)).shape[0])
        if not (1 <= n <= _lib.PXT_DEPTH_MAX_POINTS):
            raise _lib.PxtError(f"{op}: problem {k}: {n} points (1..{_lib.PXT_DEPTH_MAX_POINTS})")
        _point_mask(op, mk, n, "point_mask" + where)
        if min(int(x) for x in _sensor(op, sen, "sensor" + where, (None, None)).shape) < 4:
            raise _lib.PxtError(f"{op}: sensor {k} is {tuple(sen.shape)}; H, W >= 4")
        if cd is not None:
            _dense(op, cd, "codes" + where, torch.uint8, (rows + 1, n))
        # (the pose, the record and the log may also be pinned host memory)
        _one_device(op, workspace, [(p3d[k], "p3d"), (mk, "point_mask"), (sen, "sensor"), (cd, "codes")], where)
        q = probs[k]
        q.pose = _record(op, poses[k], f"pose {k}", torch.float32, 16 if pose_is_lm_record else 12, dev)
        q.out = _record(op, records[k], f"record {k}", torch.float32, _lib.PXT_DEPTH_RECORD, dev)
        q.log = None if lg is None else _record(op, lg, f"log {k}", torch.float32, 0, dev,
                                                shape=(rows, _lib.PXT_DEPTH_LOG_STRIDE))
        q.p3d, q.point_mask, q.n_points = p3d[k].data_ptr(), _lib.dptr(mk), n
        q.sensor, q.height, q.width = sen.data_ptr(), int(sen.shape[0]), int(sen.shape[1])
        q.sensor_scale = float(sensor_scales[k])
        q.cam[:] = [float(x) for x in cameras[10 * k:10 * k + 10]]
        q.ndist = int(ndist[k])
        q.pose_is_lm_record = int(bool(pose_is_lm_record))
        q.prior[:] = [float(x) for x in priors[21 * k:21 * k + 21]]
        q.codes = _lib.dptr(cd)
    _workspace(op, workspace, int(L.pxt_depth_refine_workspace_bytes(K)), f"{K} problems are not supported", any_dtype="workspace")
    conf = _lib.DepthConf()
    conf.num_iters, conf.pad, conf.loss = int(num_iters), int(pad), int(loss)
    conf.loss_alpha, conf.loss_scale = float(loss_alpha), float(loss_scale)
    conf.lambda_[:] = [float(x) for x in lambdas]
    conf.max_residual, conf.max_edge = float(max_residual), float(max_edge)
    conf.grad_stop, conf.dt_stop, conf.dR_stop, conf.min_valid = float(grad_stop), float(dt_stop), float(dR_stop), int(min_valid)
    _lib.check(L.pxt_depth_refine(probs, K, C.byref(conf), workspace.data_ptr(), _stream(workspace)), "pxt_depth_refine")


def _occlusion_pair(op, where, depth, sensor, mask_in, mask, occluder):
    """One image pair of the occlusion ops: the Depth render [H, W, 4], the sensor image and the plain mask of its
    size, and the two planes the kernels write -> (H, W)."""
    _dense(op, depth, "depth" + where, shape=(None, None, 4))
    H, W = int(depth.shape[0]), int(depth.shape[1])
    _sensor(op, sensor, "sensor" + where, (H, W))
    _dense(op, mask_in, "mask_in" + where, torch.uint8, (H, W))
    _mask_out(mask, H, W, depth, op)
    _mask_out(occluder, H, W, depth, op)
    return H, W


def _occlusion_mask(depth, sensor, mask_in, shift, min_alpha, sensor_q, delta_q, radii, mask, occluder, record, workspace):
    op = "occlusion_mask"
    L = _lib.lib()
    H, W = _occlusion_pair(op, "", depth, sensor, mask_in, mask, occluder)
    if mask.data_ptr() == occluder.data_ptr():
        raise _lib.PxtError(f"{op}: mask and occluder are two tensors")
    _shifts(op, shift)
    _radii(op, radii)
    rec = _record(op, record, "record", torch.int32, _lib.PXT_OCCLUSION_RECORD, depth.device)
    _workspace(op, workspace, int(L.pxt_occlusion_mask_workspace_bytes(W, H)), f"{W} x {H} is not supported (1..2^28 pixels)")
    _one_device(op, depth, [(depth, "depth"), (sensor, "sensor"), (mask_in, "mask_in"), (workspace, "workspace")])
    _lib.check(L.pxt_occlusion_mask(depth.data_ptr(), sensor.data_ptr(), mask_in.data_ptr(), W, H, int(shift[0]),
                                    int(shift[1]), float(min_alpha), float(sensor_q), float(delta_q), int(radii[0]),
                                    int(radii[1]), mask.data_ptr(), occluder.data_ptr(), rec, workspace.data_ptr(),
                                    _stream(depth)), "pxt_occlusion_mask")


def _occlusion_mask_views(depth, sensors, masks_in, shifts, min_alpha, quanta, radii, masks, occluders, records, workspace):
    op = "occlusion_mask_views"
    L = _lib.lib()
    K = len(depth)
    if not (1 <= K <= _lib.PXT_OCCLUSION_MAX_VIEWS):
        raise _lib.PxtError(f"{op}: 1..{_lib.PXT_OCCLUSION_MAX_VIEWS} views (got {K})")
    if not (len(sensors) == len(masks_in) == len(masks) == len(occluders) == K) or len(quanta) != 2 * K:
        raise _lib.PxtError(f"{op}: sensors, masks_in, masks and occluders hold one tensor and quanta (sensor_q, delta_q) "
                            f"two values per view ({K} views)")
    _radii(op, radii)
    _shifts(op, shifts, K)
    views = (_lib.OcclusionView * K)()
    sizes, spans, named = [], [], [(workspace, "workspace")]
    for k in range(K):
        d, sen, mi, mo, oc = depth[k], sensors[k], masks_in[k], masks[k], occluders[k]
        H, W = _occlusion_pair(op, f"[{k}]", d, sen, mi, mo, oc)
        named += [(d, f"depth[{k}]"), (sen, f"sensors[{k}]"), (mi, f"masks_in[{k}]")]
        sizes += [W, H]
        spans += [(mo.data_ptr(), mo.data_ptr() + H * W, f"masks[{k}]"), (oc.data_ptr(), oc.data_ptr() + H * W, f"occluders[{k}]")]
        v = views[k]
        v.depth, v.sensor, v.mask_in, v.mask_out, v.occluder = d.data_ptr(), sen.data_ptr(), mi.data_ptr(), mo.data_ptr(), oc.data_ptr()
        v.width, v.height, v.shift_x, v.shift_y = W, H, int(shifts[2 * k]), int(shifts[2 * k + 1])
        v.sensor_q, v.delta_q = float(quanta[2 * k]), float(quanta[2 * k + 1])
    spans.sort()
    for (_lo, hi, a), (lo, _hi, b) in zip(spans, spans[1:]):
        if lo < hi:
            raise _lib.PxtError(f"{op}: {a} and {b} overlap; every view writes planes of its own")
    rec = _record(op, records, "records", torch.int32, 0, depth[0].device, shape=(K, _lib.PXT_OCCLUSION_RECORD))
    _workspace(op, workspace, int(L.pxt_occlusion_mask_views_workspace_bytes(K, (C.c_int32 * (2 * K))(*sizes))),
               f"planes of {list(zip(sizes[0::2], sizes[1::2]))} are not supported (1..2^28 pixels)")
    _one_device(op, depth[0], named)
    _lib.check(L.pxt_occlusion_mask_views(views, K, float(min_alpha), int(radii[0]), int(radii[1]), rec,
                                          workspace.data_ptr(), _stream(depth[0])), "pxt_occlusion_mask_views")


def _mask_exclude(mask_in, occluder, mask, record):
    op = "mask_exclude"
    _dense(op, mask_in, "mask_in", torch.uint8, (None, None))
    H, W = int(mask_in.shape[0]), int(mask_in.shape[1])
    _dense(op, occluder, "occluder", torch.uint8, (H, W))
    _dense(op, mask, "mask", torch.uint8, (H, W))
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise _lib.PxtError(f"{op}: {W} x {H} is not supported (1..2^28 pixels)")
    if mask.data_ptr() == occluder.data_ptr():
        raise _lib.PxtError(f"{op}: mask may be mask_in, not occluder")
    rec = _record(op, record, "record", torch.int32, 2, mask_in.device)
    _one_device(op, mask_in, [(mask_in, "mask_in"), (occluder, "occluder"), (mask, "mask")])
    _lib.check(_lib.lib().pxt_mask_exclude(mask_in.data_ptr(), occluder.data_ptr(), W, H, mask.data_ptr(), rec,
                                           _stream(mask_in)), "pxt_mask_exclude")


def _points_visible(p3d, valid_in, pose, camera, ndist, occluder, valid, record):
    op = "points_visible"
    n = int(_dense(op, p3d, "p3d", shape=(None, 3)).shape[0])
    _dense(op, occluder, "occluder", torch.uint8, (None, None))
    H, W = int(occluder.shape[0]), int(occluder.shape[1])
    if len(pose) != 12 or len(camera) != 10:
        raise _lib.PxtError(f"{op}: pose holds 12 floats, camera 10")
    if (float(camera[0]), float(camera[1])) != (float(W), float(H)):
        raise _lib.PxtError(f"{op}: the camera is {camera[0]:g} x {camera[1]:g}, the occluder plane {W} x {H}")
    for t, name in ((valid_in, "valid_in"), (valid, "valid")):
        if t is not None:
            _dense(op, t, name, torch.uint8, (n,))
    rec = _record(op, record, "record", torch.int32, _lib.PXT_OCCLUSION_RECORD, occluder.device)
    _one_device(op, occluder, [(occluder, "occluder"), (p3d, "p3d"), (valid_in, "valid_in"), (valid, "valid")])
    T = (C.c_float * 12)(*[float(x) for x in pose])
    cam = (C.c_float * 10)(*[float(x) for x in camera])
    _lib.check(_lib.lib().pxt_points_visible(p3d.data_ptr() if n else None, _lib.dptr(valid_in) if n else None, n, T, cam,
                                             int(ndist), occluder.data_ptr(), W, H, valid.data_ptr() if n else None, rec,
                                             _stream(occluder)), "pxt_points_visible")


def _ngp_query(ctx, pos, dir, out):
    op = "ngp_query"
    n = int(_dense(op, pos, "pos", shape=(None, 3)).shape[0])
    _dense(op, dir, "dir", shape=(n, 3))
    _dense(op, out, "out", shape=(n, 4))
    if n < 1:
        raise _lib.PxtError(f"{op}: no point to query")
    _one_device(op, pos, [(pos, "pos"), (dir, "dir"), (out, "out")])
    _lib.check(_lib.lib().pxt_ngp_query(int(ctx), pos.data_ptr(), dir.data_ptr(), n, out.data_ptr(), _stream(pos)),
               "pxt_ngp_query")


def _iso_grid(op, values, grid, workspace):
    """What iso_surface_count and iso_surface_emit check alike: the lattice, its grid record and the workspace the
    pair shares -> pxt_iso_grid."""
    _dense(op, values, "values", shape=(None, None, None))
    if len(grid) != 7:
        raise _lib.PxtError(f"{op}: grid holds iso, origin xyz, spacing xyz")
    nz, ny, nx = (int(v) for v in values.shape)
    need = int(_lib.lib().pxt_iso_surface_workspace_bytes(nx, ny, nz)) if min(nx, ny, nz) >= 1 else -1
    _workspace(op, workspace, need, f"a {nz} x {ny} x {nx} lattice is not supported (every extent >= 1, <= 2^27 points)")
    _one_device(op, values, [(values, "values"), (workspace, "workspace")])
    g = [float(v) for v in grid]
    return _lib.IsoGrid(nx, ny, nz, g[0], (C.c_float * 3)(*g[1:4]), (C.c_float * 3)(*g[4:7]))


def _iso_surface_count(values, grid, workspace, counts):
    g = _iso_grid("iso_surface_count", values, grid, workspace)
    rec = _record("iso_surface_count", counts, "counts", torch.int32, 2, values.device)
    _lib.check(_lib.lib().pxt_iso_surface_count(values.data_ptr(), C.byref(g), workspace.data_ptr(), rec, _stream(values)),
               "pxt_iso_surface_count")


def _iso_surface_emit(values, grid, workspace, vertices, normals, triangles):
    op = "iso_surface_emit"
    g = _iso_grid(op, values, grid, workspace)
    n = int(_dense(op, vertices, "vertices", shape=(None, 3)).shape[0])
    m = int(_dense(op, triangles, "triangles", torch.int32, (None, 3)).shape[0])
    if normals is not None:
        _dense(op, normals, "normals", shape=(n, 3))
    _one_device(op, values, [(vertices, "vertices"), (normals, "normals"), (triangles, "triangles")])
    _lib.check(_lib.lib().pxt_iso_surface_emit(values.data_ptr(), C.byref(g), workspace.data_ptr(),
                                               vertices.data_ptr() if n else None, n,
                                               _lib.dptr(normals) if n else None, triangles.data_ptr() if m else None, m,
                                               _stream(values)), "pxt_iso_surface_emit")


def _max_pairwise_distance(points, out, workspace):
    op = "max_pairwise_distance"
    L = _lib.lib()
    n = int(_dense(op, points, "points", shape=(None, 3)).shape[0])
    _workspace(op, workspace, int(L.pxt_max_pairwise_distance_workspace_bytes(n)), f"{n} points is not supported (1..2^22)")
    rec = _record(op, out, "out", torch.int32, 4, points.device)
    _one_device(op, points, [(points, "points"), (workspace, "workspace")])
    _lib.check(L.pxt_max_pairwise_distance(points.data_ptr(), n, workspace.data_ptr(), rec, _stream(points)),
               "pxt_max_pairwise_distance")


def _mesh_inputs(op, vertices, triangles, views=None):
    """A mesh's vertices float32 [V, 3] and triangles int32 [T, 3], and the device tensor of view records -> (V, T)."""
    _dense(op, vertices, "vertices", shape=(None, 3))
    _dense(op, triangles, "triangles", torch.int32, (None, 3))
    if views is not None:
        _dense(op, views, "views", shape=(None, _lib.PXT_MESH_VIEW))
    return int(vertices.shape[0]), int(triangles.shape[0])


def _mesh_raster_workspace(op, workspace, P, V, T, W, H):
    need = int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, T, W, H)) if min(P, T, W, H) >= 1 and 1 <= V <= 1 << 24 else -1
    _workspace(op, workspace, need, f"{P} views of {W} x {H}, {V} vertices, {T} triangles are not supported "
                                    "(1..4096 views, 1..2^26 pixels, 1..2^24 vertices and triangles)")


def _mesh_raster(vertices, triangles, views, depth, triangle_ids, records, workspace):
    op = "mesh_raster"
    V, T = _mesh_inputs(op, vertices, triangles, views)
    P = int(views.shape[0])
    _dense(op, depth, "depth", shape=(P, None, None, 4))
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if triangle_ids is not None:
        _dense(op, triangle_ids, "triangle_ids", torch.int32, (P, H, W))
    _dense(op, records, "records", torch.int32, (P, _lib.PXT_MESH_RASTER_RECORD))
    _mesh_raster_workspace(op, workspace, P, V, T, W, H)
    _one_device(op, vertices, [(vertices, "vertices"), (triangles, "triangles"), (views, "views"), (depth, "depth"),
                               (records, "records"), (workspace, "workspace"), (triangle_ids, "triangle_ids")])
    _lib.check(_lib.lib().pxt_mesh_raster(vertices.data_ptr(), V, triangles.data_ptr(), T, views.data_ptr(), P, W, H,
                                          depth.data_ptr(), _lib.dptr(triangle_ids), records.data_ptr(),
                                          workspace.data_ptr(), _stream(vertices)), "pxt_mesh_raster")


def _mesh_render_checked(op, vertices, triangles, shading, views, width, height, rgba, rgb_u8, depth, depth_nz,
                         triangle_ids, records, workspace):
    """The checks mesh_render and mesh_render_textured share -> (V, T, P, W, H).  ``shading`` = (colors, uvs,
    triangle_uvs, texture), the call's own inputs."""
    V, T = _mesh_inputs(op, vertices, triangles, views)
    P, W, H = int(views.shape[0]), int(width), int(height)
    attrs = _mesh_shading_checked(op, V, T, *shading)
    outs = [(rgba, "rgba", torch.float32, (P, H, W, 4)), (rgb_u8, "rgb_u8", torch.uint8, (P, H, W, 3)),
            (depth, "depth", torch.float32, (P, H, W, 4)), (depth_nz, "depth_nz", torch.uint8, (P, H, W)),
            (triangle_ids, "triangle_ids", torch.int32, (P, H, W))]
    for t, name, dtype, shape in outs:
        if t is not None:
            _dense(op, t, name, dtype, shape)
    if all(t is None for t, *_ in outs):
        raise _lib.PxtError(f"{op}: no output was asked for")
    _dense(op, records, "records", torch.int32, (P, _lib.PXT_MESH_RASTER_RECORD))
    _mesh_raster_workspace(op, workspace, P, V, T, W, H)
    _one_device(op, vertices, [(vertices, "vertices"), (triangles, "triangles"), *attrs, (views, "views"),
                               (records, "records"), (workspace, "workspace"), *[(t, name) for t, name, *_ in outs]])
    return V, T, P, W, H


def _mesh_render(vertices, triangles, colors, views, width, height, rgba, rgb_u8, depth, depth_nz, triangle_ids,
                 records, workspace):
    V, T, P, W, H = _mesh_render_checked("mesh_render", vertices, triangles, (colors, None, None, None), views, width,
                                         height, rgba, rgb_u8, depth, depth_nz, triangle_ids, records, workspace)
    _lib.check(_lib.lib().pxt_mesh_render(
        vertices.data_ptr(), V, triangles.data_ptr(), T, colors.data_ptr(), views.data_ptr(), P, W, H, _lib.dptr(rgba),
        _lib.dptr(rgb_u8), _lib.dptr(depth), _lib.dptr(depth_nz), _lib.dptr(triangle_ids), records.data_ptr(),
        workspace.data_ptr(), _stream(vertices)), "pxt_mesh_render")


def _mesh_render_textured(vertices, triangles, uvs, triangle_uvs, texture, views, width, height, rgba, rgb_u8, depth,
                          depth_nz, triangle_ids, records, workspace):
    V, T, P, W, H = _mesh_render_checked(
        "mesh_render_textured", vertices, triangles, (None, uvs, triangle_uvs, texture), views, width, height, rgba,
        rgb_u8, depth, depth_nz, triangle_ids, records, workspace)
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
    op = "mesh_render_frame"
    L = _lib.lib()
    V, T = _mesh_inputs(op, vertices, triangles, views)
    P, need = mesh_frame_planes(geometry, offsets, op)
    if int(views.shape[0]) != P:
        raise _lib.PxtError(f"{op}: {int(views.shape[0])} views for {P} geometry entries")
    attrs = _mesh_shading_checked(op, V, T, colors, uvs, triangle_uvs, texture)
    outs, cap = _mesh_frame_buffers(op, need, rgba, rgb_u8, depth, depth_nz)
    _dense(op, records, "records", torch.int32, (P, _lib.PXT_MESH_RASTER_RECORD))
    geo = (C.c_int32 * (3 * P))(*[int(x) for x in geometry])
    off = (C.c_int64 * (4 * P))(*[int(x) for x in offsets])
    _workspace(op, workspace, int(L.pxt_mesh_render_frame_workspace_bytes(P, T, geo)) if T >= 1 and 1 <= V <= 1 << 24 else -1,
               f"{V} vertices, {T} triangles are not supported (1..2^24 vertices and triangles)")
    _one_device(op, vertices, [(vertices, "vertices"), (triangles, "triangles"), *attrs, (views, "views"),
                               (records, "records"), (workspace, "workspace"), *outs])
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
        return [(_dense(what, colors, "colors", shape=(V, 3)), "colors")]
    if uvs is None or triangle_uvs is None or texture is None:
        raise _lib.PxtError(f"{what}: a textured mesh needs uvs, triangle_uvs and texture")
    _dense(what, uvs, "uvs", shape=(None, 2))
    _dense(what, triangle_uvs, "triangle_uvs", torch.int32, (T, 3))
    _dense(what, texture, "texture", torch.uint8, (None, None, 4))
    if not (1 <= int(uvs.shape[0]) <= 1 << 24) or not (1 <= int(texture.shape[0]) <= 16384 and 1 <= int(texture.shape[1]) <= 16384):
        raise _lib.PxtError(f"{what}: uvs {tuple(uvs.shape)} / texture {tuple(texture.shape)}, expected [1..2^24, 2] / "
                            "[1..16384, 1..16384, 4]")
    return [(uvs, "uvs"), (triangle_uvs, "triangle_uvs"), (texture, "texture")]


def _mesh_frame_buffers(what, need, rgba, rgb_u8, depth, depth_nz):
    """The four flat output buffers hold the views' planes -> (the buffers named, their sizes in bytes)."""
    outs = [(rgba, "rgba", torch.float32), (rgb_u8, "rgb_u8", torch.uint8), (depth, "depth", torch.float32),
            (depth_nz, "depth_nz", torch.uint8)]
    out_bytes = []
    for (t, name, dtype), n in zip(outs, need):
        have = 0 if t is None else _dense(what, t, name, dtype).numel() * t.element_size()
        if have < n:
            raise _lib.PxtError(f"{what}: {name} holds {have} bytes, the views' planes need {n}")
        out_bytes.append(have)
    return [(t, name) for t, name, _ in outs], (C.c_int64 * 4)(*out_bytes)


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
    if len(pose_records) != P or len(radii) != P:
        raise _lib.PxtError(f"{what}: pose_records and radii hold one entry per view ({P}; got {len(pose_records)}, "
                            f"{len(radii)})")
    table = (_lib.MeshViewPose * P)()
    for p, (rec, radius) in enumerate(zip(pose_records, radii)):
        if rec is None:
            continue
        table[p].pose_record = _record(what, rec, f"pose_records[{p}]", torch.float32, 16, device)
        table[p].radius = radius = float(radius)
        if not (math.isfinite(radius) and radius >= 0.0):
            raise _lib.PxtError(f"{what}: view {p}'s radius is finite and >= 0 (got {radius})")
    if views_out is not None:
        _record(what, views_out, "views_out", torch.float32, 0, device, shape=(P, _lib.PXT_MESH_VIEW_OUT))
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
    if views.is_cuda:  # (the floats travel in the call's parameter record)
        raise _lib.PxtError(f"{what}: views is a CPU tensor (got {views.device})")
    _dense(what, views, "views", shape=(P, _lib.PXT_MESH_VIEW))
    named, descs, counts = [], (_lib.MeshDesc * M)(), []
    for m in range(M):
        v, t = vertices[m], triangles[m]
        V, T = _mesh_inputs(f"{what}: mesh {m}", v, t)
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
    outs, cap = _mesh_frame_buffers(what, need, rgba, rgb_u8, depth, depth_nz)
    _dense(what, records, "records", torch.int32, (P, _lib.PXT_MESH_RASTER_RECORD))
    geo = (C.c_int32 * (3 * P))(*[int(x) for x in geometry])
    off = (C.c_int64 * (4 * P))(*[int(x) for x in offsets])
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
        occ_have = 0 if occluder is None else _dense(what, occluder, "occluder", torch.uint8).numel()
        if occ_have < occ_need:
            raise _lib.PxtError(f"{what}: occluder holds {occ_have} bytes, the views' planes need {occ_need}")
    size_fn = L.pxt_mesh_render_frame_batch_workspace_bytes if scene is None else L.pxt_mesh_render_scene_batch_workspace_bytes
    _workspace(what, workspace, int(size_fn(M, (C.c_int32 * M)(*counts), P, vm, geo)),
               f"the views {list(geometry)} are not supported")
    _one_device(what, vertices[0], named + [(occluder, "occluder"), (records, "records"), (workspace, "workspace"), *outs])
    common = (descs, M, vm, views.data_ptr(), P, geo, off, _lib.dptr(rgba), _lib.dptr(rgb_u8), _lib.dptr(depth),
              _lib.dptr(depth_nz), cap)
    if posed is not None:
        pose_records, radii, views_out = posed
        table = mesh_view_poses(pose_records, radii, views_out, P, vertices[0].device, what)
        _lib.check(L.pxt_mesh_render_frame_batch_posed(*common, records.data_ptr(), workspace.data_ptr(), table,
                                                       _lib.dptr(views_out), _stream(vertices[0])),
                   "pxt_mesh_render_frame_batch_posed")
    elif scene is None:
        _lib.check(L.pxt_mesh_render_frame_batch(*common, records.data_ptr(), workspace.data_ptr(), _stream(vertices[0])),
                   "pxt_mesh_render_frame_batch")
    else:
        _lib.check(L.pxt_mesh_render_scene_batch(
            *common, (C.c_int32 * P)(*[int(x) for x in view_scene]), int(r_grow), _lib.dptr(occluder), occ_have,
            (C.c_int64 * P)(*[int(x) for x in occluder_offsets]), records.data_ptr(), workspace.data_ptr(),
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
