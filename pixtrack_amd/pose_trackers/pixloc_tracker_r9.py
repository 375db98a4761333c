"""PixLocPoseTrackerR9 -- the production tracker and its CLI
(reference pixtrack/pose_trackers/pixloc_tracker_r9.py:32-318).

Per-frame policy kept from the reference: cold start refines at image scales [4, 1] from the upright
reference pose; afterwards scale [1] with the query masked by the dilated NeRF depth silhouette of the previous pose; the
reference view is re-rendered with the NeRF at the current pose every frame (the THRESH = 0 dynamic-reference cache never
hits, Appendix D.2); success = optimiser success AND cost <= 1.1 x first-frame cost.

Device residency (the MI355X-first part): the NeRF frames, the mask, the query image, both feature pyramids and the sparse
reference features never leave HBM; the LM kernel writes the pose and the iteration log into pinned host memory.

CLI (unchanged): --object_path P --query DIR --out_dir DIR [--frames N] [--debug 0/1/2];
env UPRIGHT_REF_IMG, OBJ_AABB; outputs poses.pkl, trackers.pkl.
"""
from __future__ import annotations

import argparse
import ast
import logging
import os
import pickle as pkl
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from .. import _lib
from ..ops import ops
from ..geometry import Camera as PixCamera, Pose
from ..model3d import Model3D, extract_covisibility
from ..pinned import PinnedRing, SensorStage
from ..refiner import Paths, PoseTrackerLocalizer
from ..point_report import parse_mode
from ..tracker import DebugTracker
from ..utils.colmap import ColmapCamera
from ..utils.ingp_utils import initialize_ingp, load_nerf2sfm, sfm_to_nerf_pose
from ..utils.io import ArrayIterator, ImageIterator
from ..utils.pose_utils import (geodesic_distance_for_rotations, geodesic_distances_to,
                                get_camera_in_world_from_pixpose)
from ..visualization.run_vis_on_poses import get_nerf_image_device, rgba_to_u8
from .base_pose_tracker import PoseTracker

logger = logging.getLogger(__name__)


def infer_camera_from_image(width: int, height: int) -> ColmapCamera:
    """pycolmap.infer_camera_from_image without EXIF: SIMPLE_RADIAL, f = 1.2 max(w, h),
    principal point at the image centre, k = 0."""
    f = 1.2 * max(width, height)
    return ColmapCamera(None, "SIMPLE_RADIAL", int(width), int(height), np.array([f, width / 2.0, height / 2.0, 0.0]))


@dataclass(slots=True, eq=False)
class FramePlanes:
    """The device tensors of one frame of one object at one pose, on their way from who made them to who uses them.
    Records are compared by identity, and ``pose`` is compared with ``is``: planes made for another Pose object are not
    used.  Every other field is None until set and None again once handed out.  A tracker holds at most four records:

    ``_own`` - what this frame's own call produced for the current pose.  Set by ``_draw_frame`` (pose, mask, ref_u8;
    depth where a float depth image was drawn; view with a mesh template's depth plane), or it is the ``_ahead_ok``
    record that ``get_mask`` took.  ``get_reference_image`` hands out and clears ref_u8 (``keep=True``: leaves it for
    the next call); ``_create_dynamic_reference_from_render`` / ``_from_template`` hand out and clear depth and view;
    ``_apply_template_occlusion`` reads depth and view and leaves them.

    ``_primed`` - what lock-step tracking made in one call with the other objects'.  Set by ``prime`` alone, which empties
    the one holder a tracker has for a new pose object.  depth_nz, ref_u8 and mutual (occluder plane, scene record): taken, or
    dropped, by ``_draw_frame`` of a mesh template.  points (p3d, slot_valid, record): by
    ``_create_dynamic_reference_from_template``.  occlusion (the pass's frame dict, occlusion.pass_frame; its "mask_in"
    is the plain mask ``_draw_frame`` then does not make again): by ``_apply_template_occlusion``; also cleared by
    ``refine`` and ``_adopt_depth_sensor``.

    ``_ahead`` - the frame queued behind the last LM launch, its pose known to the device alone.  Set by
    ``_render_ahead``, ``_render_ahead_accept`` and ``_render_ahead_mesh_accept``: mask, ref_u8, depth, ``cams`` (the
    pinned camera records, or a mesh call's views_out rows, to verify) and ``keys`` (the view settings it baked in).
    Cleared by ``_frame_setup``, ``_query_tile_fallback`` and ``_verify_render_ahead``.

    ``_ahead_ok`` - that record once ``_verify_render_ahead`` has set pose (and, for a mesh depth plane, view: the
    host's record, proved bit-equal to the one the plane was drawn with).  ``get_mask`` takes it, as ``_own``, or drops
    it; assigning None discards it."""
    pose: Optional[Pose] = None
    depth_nz: Optional[torch.Tensor] = None   # uint8 [H, W]: the `uint8(depth * 255) != 0` plane a mesh frame call wrote
    mask: Optional[torch.Tensor] = None       # uint8 [H, W]: its morphology (_mask_of), before any occlusion pass
    ref_u8: Optional[torch.Tensor] = None     # uint8 [H, W, 3]: the reference image
    depth: Optional[torch.Tensor] = None      # float32 [H, W, 4]: the query view's Depth render / depth plane
    view: object = None                       # 20 floats: the view record a mesh template's ``depth`` was drawn with
    mutual: Optional[tuple] = None
    points: Optional[tuple] = None
    occlusion: Optional[dict] = None
    cams: object = None
    keys: Optional[list] = None


class PixLocPoseTrackerR9(PoseTracker):
    def __init__(self, object_path, data_path, loc_path, eval_path, debug=0, device=None, assets=None,
                 unet_precision="fp16", relocalizer=None, uncertainty=False, reference_points="sfm",
                 point_report=False, depth_refine=None, occlusion=None, template=None, reference_sfm=None,
                 upright_ref_img=None, reloc_depth=None, reloc_options=None):
        """``assets`` (optional) supplies everything that otherwise comes from disk, for the
        synthetic runs: dict(model3d, nerf2sfm, snapshot, weights, covis=None, aabb, upright_ref_img).
        ``unet_precision``: "fp16" (default) or "fp32" - the UNet pass the localizer builds (unet.UNet).
        ``relocalizer``: None / "off" (default: the reference's behaviour - cold start from the upright view, nothing
        relocalises), "views" (a relocalizer.Relocalizer over the mapping views) or a Relocalizer instance: the cold
        start and the frame after a failed frame then take their pose from Relocalizer.localize.  "mesh": the same for a
        mesh template (``template=MeshTemplate(...)``; ValueError without one), with ``reference_points`` "sfm" or
        "template" and with the sensor options: the bank is the mapping views of the mesh-built SfM model, its reference
        views drawn by the template itself, 32 per render_frame_batch call, beside the frame's own planes.
        From the first relocalisation of a segment on, the frame's reference image is the mapping image on the SIDE the
        camera sees instead of the nearest by rotation (_nearest_reference_ids says why); a tracker that never
        relocalises chooses as before.
        ``reloc_options``: keywords for that Relocalizer (views, rolls, shifts, top_k, max_views, ...).
        ``reloc_depth``: None or a relocalizer.RelocDepth (``relocalizer="mesh"`` only) - a relocalised frame that has a
        sensor image first scores a placement grid (lateral cell x distance per bank entry) against it in one
        pxt_score_pose_hypotheses_depth launch and hands the best to the feature scorer.  Shares the
        frame's one sensor upload with ``depth_refine`` / ``occlusion`` (the same lookup and scale, ValueError
        otherwise).  The history entry of a relocalised frame gains ``reloc_n_placed`` and ``reloc_n_geometric`` (None
        without the depth stage); nothing on the policy path reads them and the cost gate is untouched - it stays
        frozen at the cold start's cost, so a relocalised frame may refine well and still go untracked.
        ``uncertainty``: False (default: nothing changes) or True - every LM launch is followed by one
        pxt_lm_information problem at the pose it returns, and a frame's history entry gains ``pose_info`` (6 x 6),
        ``pose_cov`` (6 x 6 or None), ``observability``, ``info_level`` and ``info_n_valid`` from the frame's last LM
        launch (uncertainty.py); None for a frame whose refinement failed.  The cost gate, the pose update and
        ``tracked`` never read them.
        ``reference_points``: "sfm" (default: the reference's behaviour - a frame is refined on the SfM points of the
        nearest mapping image) or "render" - on up to ``reference_points_max`` points back-projected from a lattice of the
        frame's own Depth render (refiner.points_from_render): they cover the visible side, do not change when
        update_reference_ids switches and need no triangulated points.  A frame's history entry then gains
        ``n_reference_points`` and ``reference_point_stride``; nothing on the policy path reads them.  Not combined
        with ``relocalizer`` or ``uncertainty`` yet (ValueError).  "template" is "render" for a mesh template: the
        lattice is taken from the float depth plane the template's frame call draws for the query view
        (``MeshTemplate.frame(..., want_depth=True)``) and back-projected through the very view record it was drawn
        with (refiner.points_from_template, pxt_points_from_depth_views); same history keys, same refusals, and it needs
        ``template=MeshTemplate(...)`` - with the NeRF template the value is refused and "render" is the one to use.
        ``point_report``: False / "off" (default: nothing changes), "summary" or "full" - every LM launch is followed by
        one pxt_lm_point_report problem at the pose it returns (its last level), and a frame's history entry gains
        ``n_valid_points``, ``n_inliers``, ``inlier_ratio``, ``mean_robust_weight`` and ``rejected_points``
        (point_report.py; None for a frame whose refinement failed); "full" also adds ``point_report``, a dict of numpy
        arrays per point (p2d, valid, cost, rho, robust_weight, confidence, reject), and fills the DebugTracker's
        ``p3d`` / ``p3d_ids`` / ``point_report`` at debug >= 2.  Works with both ``reference_points`` settings.  The
        cost gate, the pose update and ``tracked`` never read any of it.
        ``depth_refine``: None (default: nothing changes) or a depth_refinement.DepthRefine (a conf, the sensor's scale, a
        ``lookup(frame_name) -> uint16 [H, W]`` and an optional diagonal prior): one pxt_depth_refine problem is queued
        behind the frame's last LM launch - its points, mask and unscaled query camera, the start pose read from the LM's
        record on the device - and the frame's pose becomes the depth-refined one when the frame succeeded (the LM's
        success and the cost gate are decided as ever, on the feature cost), the record's status is 1.0, it did not fail
        and its final mean depth cost is not above the initial one.  The history entry gains ``T_lm``,
        ``depth_refined``, ``depth_cost_before``, ``depth_cost_after``, ``depth_n_valid`` and ``depth_iters``;
        ``T_refined`` is the pose carried forward.  The sensor image is fetched and its upload queued before the frame's
        first launch; a frame with more than 4096 points uses the first 4096 (logged once).  Switches ``render_ahead`` off: the render queued behind the LM launch
        takes its camera from the LM kernel's epilogue, which is no longer the pose the next frame starts from.  Not
        combined with a relocalizer yet.  With a mesh template the option needs ``reference_points="template"``, whose
        points lie on the surface the sensor sees.
        ``occlusion``: None (default: nothing changes) or an occlusion.OcclusionMask (a conf, the sensor's scale and a
        ``lookup(frame_name) -> uint16 [H, W]``): on a frame that gets a mask, the pixels where the frame's sensor depth
        image lies in front of the mask view's Depth render - opened and grown, pxt_occlusion_mask - leave the query
        mask, and the reference points that project onto them at the start pose leave the LM's point mask
        (pxt_points_visible; uncertainty, point report and depth refinement of that frame use the same gated mask).  A
        frame without a mask (cold start, after a failed frame) or without a sensor image runs as without the option.
        The history entry gains ``occluded_fraction``, ``n_occluder_pixels``, ``n_points_gated`` and
        ``occlusion_applied`` (None / 0 / 0 / False where no pass ran); ``last_occlusion`` keeps the frame's tensors.
        With a mesh template the option needs ``reference_points="template"``: the pass then runs on the float depth
        plane that setting's frame call draws, whose unit is 1 / depth_q SfM units - depth_q the word [17] of the view
        record the plane was drawn with - so the quanta are formed per frame (occlusion.mesh_quanta) and the shift is
        (0, 0); the template's ``render_ahead`` stays usable.  The objects of one image that hide each other are lock-step
        tracking's ``mutual_occlusion`` (multi_object_tracker.py), which feeds the same mask fold and point gate.
        The cost gate, success and ``tracked`` are decided as ever.  ``render_ahead`` stays on: the render queued
        behind the LM launch keeps its float Depth image, and the pass runs in get_mask of the frame that consumes it.
        Shares the frame's one sensor upload with ``depth_refine`` (the two options must then name the same lookup and
        scale).  Not combined with a relocalizer yet.
        ``template``: None / "nerf" (default: the frame's mask and reference image are NeRF renders) or a
        mesh_template.MeshTemplate - they are renders of a coloured or textured mesh, the reference image anti-aliased
        by the template's ``supersample``, both from one pxt_mesh_render_frame call.  The SfM model is then one
        mesh_dataset built from that mesh (it is in the mesh's own frame), no snapshot, ``nerf2sfm.pkl`` or $OBJ_AABB is
        read (``assets`` may omit ``snapshot``, ``nerf2sfm`` and ``aabb``), ``testbed`` is None and ``render_ahead`` is
        the template's own option, off by default: with ``MeshTemplate(..., render_ahead=True)`` the next frame's views
        are ONE posed call queued behind the LM launch, their view records formed on the device from the LM's output
        record (pxt_mesh_render_frame_batch_posed), and used only if the host arrives at the same 20 floats per view.
        Everything downstream of the two images is
        unchanged.  A frame's history gains ``template`` ("mesh") and ``template_supersample``; nothing on the policy
        path reads them.  Not combined with ``relocalizer`` or ``reference_points="render"`` (its mesh counterpart is
        ``reference_points="template"``) yet, and with ``depth_refine`` or ``occlusion`` only when
        ``reference_points="template"`` (ValueError).
        ``reference_sfm``: the directory of the SfM model (the ``ref/`` directory mesh_dataset wrote) in place of
        ``loc_path/aug_sfm``; ``upright_ref_img``: the upright reference image's name in place of $UPRIGHT_REF_IMG."""
        point_report = parse_mode(point_report)  # (a bad value: ValueError before anything is built)
        self._check_reference_points(reference_points, relocalizer, uncertainty)
        self._check_depth_refine(depth_refine, relocalizer)
        self._check_occlusion(occlusion, relocalizer, depth_refine)
        self.template = self._check_template(template, relocalizer, reference_points, depth_refine, occlusion)
        self._check_reloc_depth(reloc_depth, relocalizer, depth_refine, occlusion)
        self.reloc_depth, self._reloc_options = reloc_depth, dict(reloc_options or {})
        self.reference_points = reference_points
        default_paths = Paths(query_images="query/", reference_images=loc_path, reference_sfm="aug_sfm",
                              query_list="*_with_intrinsics.txt", global_descriptors="features.h5",
                              retrieval_pairs="pairs_query.txt", results="pixloc_object.txt")
        pixloc_conf = {
            "experiment": "pixloc_megadepth",
            "unet_precision": unet_precision,
            "features": {},
            "optimizer": {"num_iters": 150, "pad": 1},
            "refinement": {"num_dbs": 1, "multiscale": [1], "point_selection": "all",
                           "normalize_descriptors": True, "average_observations": False,
                           "do_pose_approximation": False, "reference_points": reference_points},
        }
        self.debug = debug
        self.device = torch.device(device if device is not None else "cuda:0")
        paths = default_paths.add_prefixes(Path(data_path), Path(loc_path), Path(eval_path))
        if reference_sfm is not None:
            paths["reference_sfm"] = Path(reference_sfm)
        self._upright_ref_img = upright_ref_img
        if assets is not None:
            pixloc_conf["weights"] = assets["weights"]
            model3d = assets["model3d"]
        else:
            pixloc_conf["weights_path"] = os.environ.get(
                "PIXTRACK_WEIGHTS", str(Path(object_path) / "pixtrack/pixloc_megadepth.pt"))
            model3d = Model3D(paths.reference_sfm)
        self.localizer = PoseTrackerLocalizer(paths, pixloc_conf, device=self.device, model3d=model3d)
        self.eval_path = eval_path
        covis_path = Path(paths.reference_sfm) / "covis.pkl"
        if assets is not None and assets.get("covis") is not None:
            self.covis = assets["covis"]
        elif assets is None and os.path.isfile(covis_path):
            with open(covis_path, "rb") as f:
                self.covis = pkl.load(f)
        else:
            self.covis = extract_covisibility(self.localizer.model3d)
            if assets is None:
                with open(str(covis_path), "wb") as f:
                    pkl.dump(self.covis, f)
        self.pose_history = {}
        self.pose_tracker_history = {}
        self.cold_start = True
        self.pose = None
        self.reference_ids = self._initial_reference_ids(assets)
        self.reference_scale = 0.5
        self.localizer.refiner.reference_scale = self.reference_scale
        if self.template is not None:  # the mesh is in the SfM model's frame: nothing of the NeRF is read
            self.nerf2sfm = self.testbed = None
        else:
            if assets is not None:
                self.nerf2sfm = assets["nerf2sfm"]
                snapshot = assets["snapshot"]
            else:
                self.nerf2sfm = load_nerf2sfm(str(Path(data_path) / "nerf2sfm.pkl"))
                snapshot = str(Path(object_path) / "pixtrack/instant-ngp/snapshots/weights.msgpack")
            self.testbed = initialize_ingp(snapshot, self._render_aabb(assets), device=self.device)
        self.uncertainty = bool(uncertainty)
        self.localizer.refiner.information = self.uncertainty
        self.point_report = self.localizer.refiner.point_report = point_report
        self.localizer.refiner.warm_reference_points()  # static per-reference tables, off the frame path
        self.dynamic_id, self.cache_hit, self.cost_threshold, self.camera = None, False, None, None
        self.hits = self.misses = self.relocalization_count = 0
        self.success = True
        self.spp = 8  # run_vis_on_poses.py:29
        self.batch_frame_images = True  # reference render + masked query in one batched UNet pass
        # a frame's planes between producer and consumer (FramePlanes has the table): this frame's own call, and what
        # lock-step tracking drew, extracted or masked in one call with the other objects' (multi_object_tracker.py)
        self._own: Optional[FramePlanes] = None
        self._primed = FramePlanes()
        self.template_frames_batched = 0
        self._ref_cam_cache = self._coincide_cache = None
        self.keep_feature_history = False  # the reference leaks one entry per frame (Appendix D.2)
        self.steady_multiscale = [1]  # image scales of a tracked (non-cold-start) frame (:223)
        # A frame's mask (Depth, query camera) and reference image (Shade, SfM camera 1 x reference_scale) are rendered at
        # the same pose: ONE march when the two cameras coincide (fuse_identical_views; same size and fx: all
        # get_nerf_image reads), else both renders as ONE chain of launches (Testbed.render_frame_pair_device); the
        # renderer's last kernel writes the 8-bit reference image and the mask's `!= 0` plane itself.
        self.fuse_identical_views = True
        # The next frame's renders need only this frame's pose: with `render_ahead` they are enqueued
        # BEHIND this frame's LM launch, their camera taken from the slot(s) the LM kernel's epilogue fills, instead of
        # after the host has read the result, run the policy and converted the pose (~0.1 ms of GPU idle per frame).  They
        # are consumed only if the host, once it knows the pose, arrives at the same 12 camera floats; otherwise (failed
        # frame, cost gate, relocalisation, a different last bit) the frame renders as before.  PXT_RENDER_AHEAD=0: off.
        # With a mesh template the option is the template's (MeshTemplate(render_ahead=True), off by default): the frame's
        # views are ONE posed call (pxt_mesh_render_frame_batch_posed) whose view records are formed on the device from the
        # LM's output record, and the host compares the 20 floats of every view it was drawn with.
        self.render_ahead = self._render_ahead_default(self.template)
        self._ahead_ws = None         # mesh template: the FrameBatchWorkspace of the queued calls (this tracker's stream)
        self._ahead_rows = None       # ... and the PinnedRing of their views_out blocks
        self._ahead_cam = None   # the pinned camera record the LM epilogue of this frame writes
        self._ahead: Optional[FramePlanes] = None     # the frame queued behind the last LM launch
        self._ahead_ok: Optional[FramePlanes] = None  # ... once verified for a pose (None: none, or discarded)
        # queued renders: consumed / camera record never arrived within the poll bound / host and device disagree on a camera
        # bit / view settings changed between enqueue and use
        self.renders_ahead_used = self.renders_ahead_dropped = self.renders_ahead_rejected = self.renders_ahead_stale = 0
        # Query tiles: on a steady frame the query's fine map has one reader, the LM's fine level, so its pass computes only
        # the tiles around the points' projections at the frame's initial pose, grown by `query_tile_margin` fine pixels
        # (scripts/query_tile_share.py measures it), and the LM launch guards every read; a launch that leaves the computed
        # tiles has its frame redone in full (same bits as with the option off) and the option rests for 8 frames.
        # (the library's knobs decide beneath this: pxt_unet_set_query_tiles, PXT_UNET_QUERY_TILES=0)
        self.query_tiles = unet_precision == "fp16"
        self.query_tile_margin = 8
        self.query_tile_fallbacks = 0
        self._query_tile_rest = 0  # frames the option still stays off after a fallback
        self.unet_precision = unet_precision
        self.relocalizer = self._make_relocalizer(relocalizer)
        self._mesh_relocalizer = isinstance(relocalizer, str) and relocalizer == "mesh"
        self._reference_by_side = False  # set by a relocalisation with relocalizer="mesh" (_nearest_reference_ids)
        self._lost = False  # a frame failed: the next one is relocalised (relocalizer on only)
        self._accepted_pose = None  # the last pose a frame accepted (the relocaliser scores it as one more hypothesis)
        self.last_relocalization = None  # RelocResult of the last relocalisation
        self._relocalized_frame = False  # this frame's pose came from the relocaliser (history key "relocalized")
        self.depth_refine = depth_refine
        self._depth_conf = self._depth_ws = self._depth_sensor = None
        self._sensor_stage = SensorStage(self.device)  # one image per frame, whichever sensor option reads it
        self._depth_recs, self._depth_slot, self._depth_warned_points = [], 0, False
        if depth_refine is not None:
            from ..depth_refinement import points_extent

            self.render_ahead = False
            # the conf's lengths are fractions of the model's extent: resolved once, on the host
            pts = np.array([p.xyz for p in self.localizer.model3d.points3D.values()])
            self._depth_conf = depth_refine.conf if not depth_refine.conf.relative else depth_refine.conf.resolve(
                points_extent(pts))
            self.localizer.refiner.depth_hook = self._enqueue_depth_refine
        self.occlusion = occlusion
        self.sensor_uploads = 0       # sensor images staged so far (one per frame that has one, whoever reads it)
        self.last_occlusion = None    # the tensors and figures of the last frame's occlusion pass (None: none ran)
        self._occ_conf = self._occ_q = self._occ_shift = self._occ_record = self._occ_ws = self._occ_frame = None
        if occlusion is not None:
            from ..depth_refinement import points_extent
            from ..occlusion import RECORD as OCC_RECORD, quantize
            from ..render_evaluation import z_scale

            pts = np.array([p.xyz for p in self.localizer.model3d.points3D.values()])
            self._occ_conf = occlusion.conf if not occlusion.conf.relative else occlusion.conf.resolve(points_extent(pts))
            # sensor_q, delta_q: formed in float64, rounded once (as sensor_evaluation does); a mesh template's plane is
            # scaled by its frame's own depth_q, so its quanta are formed per frame (occlusion.mesh_quanta)
            if self.template is None:
                self._occ_q = quantize(self._occ_conf.delta, occlusion.sensor_depth_scale,
                                       z_scale(self.testbed, self.nerf2sfm))
            self._occ_record = torch.zeros(OCC_RECORD, dtype=torch.int32).pin_memory()
            self._occ_done = torch.cuda.Event()
            self.localizer.refiner.point_gate = self._gate_points
        # Mutual occlusion between the tracked objects of one image (lock-step tracking of mesh templates:
        # MultiObjectTracker(mutual_occlusion=...) calls enable_mutual_occlusion).  Off: nothing below is touched.
        self.mutual_occlusion = False
        self.last_mutual_occlusion = None  # the tensors and figures of the last frame's pass (None: none ran)
        self._mut_frame = self._mut_record = self._mut_scene = self._mut_done = None

    # ------------------------------------------------------------------ per-variant set-up
    supports_render_points = True  # (the YCB policy does not yet)

    @staticmethod
    def _render_ahead_default(template) -> bool:
        """``render_ahead`` as the constructor sets it: on for the NeRF template, a mesh template's own option for a mesh
        template (off unless it was built with render_ahead=True); PXT_RENDER_AHEAD=0 switches both off."""
        return os.environ.get("PXT_RENDER_AHEAD", "1") != "0" and (template is None or bool(template.render_ahead))

    def _check_reference_points(self, reference_points, relocalizer, uncertainty):
        if reference_points not in ("sfm", "render", "template"):
            raise ValueError(f"reference_points must be 'sfm', 'render' or 'template' (got {reference_points!r})")
        if reference_points != "sfm":  # ("template" is "render" for a mesh template: the same refusals)
            if not self.supports_render_points:
                raise ValueError(f"reference_points={reference_points!r} is not supported by {type(self).__name__} yet")
            if relocalizer is not None and relocalizer != "off" and not (relocalizer == "mesh" and reference_points == "template"):
                raise ValueError(f"reference_points={reference_points!r} is not combined with a relocalizer yet (its "
                                 "feature bank is built from the SfM points), except relocalizer='mesh' with "
                                 "reference_points='template'")
            if uncertainty:
                raise ValueError(f"reference_points={reference_points!r} is not combined with uncertainty=True yet")

    @staticmethod
    def _check_template(template, relocalizer, reference_points, depth_refine, occlusion):
        """-> None (the NeRF template) or the MeshTemplate; the options a mesh template is not combined with yet are
        refused by name."""
        if template is None or (isinstance(template, str) and template == "nerf"):
            if isinstance(relocalizer, str) and relocalizer == "mesh":
                raise ValueError("relocalizer='mesh' draws its bank with a mesh template: it needs "
                                 "template=MeshTemplate(...); with the NeRF template use relocalizer='views'")
            if reference_points == "template":
                raise ValueError("reference_points='template' takes its points from a mesh template's depth plane: it needs "
                                 "template=MeshTemplate(...); with the NeRF template use reference_points='render'")
            return None
        from ..mesh_template import MeshTemplate

        if not isinstance(template, MeshTemplate):
            raise ValueError(f"template must be None, 'nerf' or a mesh_template.MeshTemplate (got {template!r})")
        if relocalizer is not None and relocalizer != "off" and not (isinstance(relocalizer, str) and relocalizer == "mesh"):
            raise ValueError("a mesh template is not combined with a relocalizer yet (its hypothesis renders are NeRF "
                             "renders), except relocalizer='mesh'")
        if reference_points == "render":
            raise ValueError("a mesh template is not combined with reference_points='render' yet (the back-projection "
                             "reads the NeRF renderer's view record)")
        # the sensor options read the float depth plane of the query view and refine on points of the sensed surface:
        # both come with reference_points="template" alone
        if depth_refine is not None and reference_points != "template":
            raise ValueError("a mesh template is not combined with depth_refine unless reference_points='template' (its "
                             "points lie on the surface the sensor sees; the SfM points of a mesh model do not): pass "
                             "reference_points='template'")
        if occlusion is not None and reference_points != "template":
            raise ValueError("a mesh template is not combined with occlusion unless reference_points='template' (the pass "
                             "compares the sensor with the float depth plane that setting's frame call draws): pass "
                             "reference_points='template'")
        return template

    supports_depth_refine = True  # (the YCB policy does not yet: its refine() does not end in _frame_policy)

    def _check_depth_refine(self, depth_refine, relocalizer):
        if depth_refine is None:
            return
        if not self.supports_depth_refine:
            raise ValueError(f"depth_refine is not supported by {type(self).__name__} yet")
        if relocalizer is not None and relocalizer != "off" and not (isinstance(relocalizer, str) and relocalizer == "mesh"):
            raise ValueError("depth_refine is not combined with a relocalizer yet, except relocalizer='mesh'")
        if not callable(getattr(depth_refine, "lookup", None)) or not float(depth_refine.sensor_depth_scale) > 0:
            raise ValueError("depth_refine: a depth_refinement.DepthRefine with a lookup and a positive sensor_depth_scale")

    supports_occlusion = True  # (the YCB policy does not yet: its refine() renders its own mask and has its own tail)

    def _check_occlusion(self, occlusion, relocalizer, depth_refine):
        if occlusion is None:
            return
        if not self.supports_occlusion:
            raise ValueError(f"occlusion is not supported by {type(self).__name__} yet")
        if relocalizer is not None and relocalizer != "off" and not (isinstance(relocalizer, str) and relocalizer == "mesh"):
            raise ValueError("occlusion is not combined with a relocalizer yet, except relocalizer='mesh'")
        if not callable(getattr(occlusion, "lookup", None)) or not float(occlusion.sensor_depth_scale) > 0 \
                or not hasattr(getattr(occlusion, "conf", None), "resolve"):
            raise ValueError("occlusion: an occlusion.OcclusionMask with a lookup, a positive sensor_depth_scale and a conf")
        if depth_refine is not None and (depth_refine.lookup is not occlusion.lookup or float(
                depth_refine.sensor_depth_scale) != float(occlusion.sensor_depth_scale)):
            raise ValueError("depth_refine and occlusion read ONE sensor image per frame: they must be given the same "
                             "lookup and the same sensor_depth_scale")

    @staticmethod
    def _check_reloc_depth(reloc_depth, relocalizer, depth_refine, occlusion):
        if reloc_depth is None:
            return
        if not (isinstance(relocalizer, str) and relocalizer == "mesh"):
            raise ValueError("reloc_depth is the depth stage of relocalizer='mesh'")
        if not callable(getattr(reloc_depth, "lookup", None)) or not float(reloc_depth.sensor_depth_scale) > 0 \
                or not hasattr(reloc_depth, "n_geometric"):
            raise ValueError("reloc_depth: a relocalizer.RelocDepth with a lookup and a positive sensor_depth_scale")
        for name, other in (("depth_refine", depth_refine), ("occlusion", occlusion)):
            if other is not None and (other.lookup is not reloc_depth.lookup or float(other.sensor_depth_scale) != float(
                    reloc_depth.sensor_depth_scale)):
                raise ValueError(f"reloc_depth and {name} read ONE sensor image per frame: they must be given the same "
                                 "lookup and the same sensor_depth_scale")

    def _stage_depth_sensor(self, query_path):
        """Before the frame's first launch: fetch the frame's sensor image and queue its upload, from a pinned buffer
        into a device buffer that both live as long as the tracker.  What then stands between the LM launch and the
        depth problem is the enqueue alone.  Either option (depth_refine, occlusion) triggers it; one upload per frame
        serves both - they name the same lookup (_check_occlusion)."""
        self._depth_sensor, self._depth_slot = None, 0
        # (one lookup, whoever names it: _check_occlusion, _check_reloc_depth)
        option = next(o for o in (self.depth_refine, self.occlusion, self.reloc_depth) if o is not None)
        sensor = option.lookup(os.path.basename(str(query_path)))
        if sensor is None:
            return
        self._depth_sensor = self._sensor_stage.upload(sensor, query_path)
        self.sensor_uploads += 1

    def _adopt_depth_sensor(self, query_path, sensor):
        """_stage_depth_sensor for a frame of lock-step tracking: ``sensor`` is the frame's image on the device (None:
        the frame has none), staged once by the caller for every tracker that names it (multi_object_tracker.py)."""
        self._depth_frame_name = query_path
        self._depth_sensor, self._depth_slot = sensor, 0
        self._occ_frame = self._primed.occlusion = None

    def _check_sensor_size(self, h: int, w: int) -> None:
        """The frame's staged sensor image has the size of the query (ValueError: a wrong sensor directory)."""
        if tuple(self._depth_sensor.shape) != (h, w):
            raise ValueError(f"the sensor depth image of {self._depth_frame_name} is {tuple(self._depth_sensor.shape)}, "
                             f"the query {(h, w)}")

    def prime(self, pose, depth_nz=None, ref_u8=None, mutual=None, points=None, occlusion=None) -> None:
        """Lock-step tracking hands over what it made for this tracker's frame at ``pose`` in one call with the other
        objects': a mesh frame's planes (``depth_nz``, ``ref_u8``; ``mutual`` = (occluder plane, scene record) where it
        was drawn as part of a scene), its ``points`` (p3d, slot_valid, record), its ``occlusion`` pass
        (occlusion.pass_frame).  Each part is used once, by the method that would otherwise make its own call, and only
        for this very pose object."""
        primed = self._primed  # (one holder per tracker: a new pose object empties it)
        if primed.pose is not pose:
            primed.pose = pose
            primed.depth_nz = primed.ref_u8 = primed.mutual = primed.points = primed.occlusion = None
        if depth_nz is not None:
            primed.depth_nz, primed.ref_u8, primed.mutual = depth_nz, ref_u8, mutual
        if points is not None:
            primed.points = points
        if occlusion is not None:
            primed.occlusion = occlusion

    def enable_mutual_occlusion(self):
        """Lock-step tracking draws this tracker's frames as part of a scene (multi_object_tracker.MutualOcclusion): a
        primed frame then carries the plane G of the pixels where another tracked mesh lies in front, which leaves the
        frame's mask (pxt_mask_exclude) and gates the LM's points (pxt_points_visible) as the sensor option's plane
        does.  A mesh template only: the plane comes out of the mesh frames' key planes."""
        from ..occlusion import RECORD as OCC_RECORD

        if self.template is None:
            raise ValueError("mutual occlusion needs a mesh template (the occluder plane is made from the mesh frames' "
                             "depth keys); NeRF-template trackers are not part of a scene yet")
        self.mutual_occlusion = True
        # words 0, 1: pxt_mask_exclude's; 8..10: pxt_points_visible's (the sensor option's record layout)
        self._mut_record = torch.zeros(OCC_RECORD, dtype=torch.int32).pin_memory()
        self._mut_scene = torch.zeros(16, dtype=torch.int32).pin_memory()  # the query view's render record
        self._mut_done = torch.cuda.Event()
        self.localizer.refiner.point_gate = self._gate_points

    def _apply_mutual_occlusion(self, mask, mutual):
        """_mask_and_reference's tail on a primed frame that was drawn as part of a scene: ``mutual`` = (G uint8 [H, W],
        the query view's render record on the device).  One launch on the frame's stream and one copy into pinned
        memory, nothing awaited; the records are read in _frame_policy."""
        from ..occlusion import mask_exclude

        occluder, scene_record = mutual
        self._mut_record.zero_()  # (the last frame's were read in its _frame_policy)
        mask_exclude(mask, occluder, mask=mask, record=self._mut_record)
        self._mut_scene.copy_(scene_record, non_blocking=True)
        self._mut_frame = {"occluder": occluder, "mask": mask, "gates": [], "record_buffer": self._mut_record,
                           "done": self._mut_done}
        self._mut_done.record(torch.cuda.current_stream(self.device))
        return mask

    def _apply_occlusion(self, mask, depth, view20=None):
        """get_mask's tail with the option on: the frame's plain mask minus the pixels where the sensor image - staged
        before the frame's first launch - lies in front of the mask view's Depth render.  Two launches on the frame's
        stream, nothing awaited; the pinned record is read in _frame_policy.  The plain mask as it is when the option
        is off, the frame has no sensor image or no float Depth image came with the mask.  ``view20``: ``depth`` is a
        mesh template's float plane and this the view record it was drawn with - its word [17], depth_q, scales the
        plane, so the quanta are this frame's, and the view has the camera's true cx, cy: no shift."""
        if self.occlusion is None or self._depth_sensor is None or depth is None:
            return mask
        from ..occlusion import alignment, mesh_quanta, occlusion_mask, pass_frame

        sensor, conf = self._depth_sensor, self._occ_conf
        H, W = int(depth.shape[0]), int(depth.shape[1])
        self._check_sensor_size(H, W)
        if view20 is not None:
            sx = sy = 0
            self._occ_q = mesh_quanta(conf.delta, self.occlusion.sensor_depth_scale, view20)
        else:
            if self._occ_shift is None or self._occ_shift[0] is not self.camera:
                self._occ_shift = (self.camera, alignment(self.camera, conf.allow_misaligned))
            sx, sy, _ = self._occ_shift[1]
        if self._occ_ws is None or self._occ_ws[0] != (W, H):
            self._occ_ws = ((W, H), torch.empty(int(_lib.lib().pxt_occlusion_mask_workspace_bytes(W, H)), dtype=torch.uint8,
                                                 device=self.device))
        out = occlusion_mask(depth, sensor, mask, (sx, sy), conf.min_alpha, self._occ_q[0], self._occ_q[1], conf.r_open,
                             conf.r_grow, record=self._occ_record, workspace=self._occ_ws[1])
        self._occ_frame = pass_frame(depth, sensor, mask, out["mask"], out["occluder"], (sx, sy), conf.min_alpha,
                                     self._occ_q, (conf.r_open, conf.r_grow), self._occ_record, self._occ_done, view20)
        self._occ_done.record(torch.cuda.current_stream(self.device))
        return out["mask"]

    def _apply_template_occlusion(self, mask, pose):
        """_apply_occlusion on a mesh template's frame: the plane and the record are the ones ``_own`` holds for
        ``pose`` (drawn by this frame's call, or by the verified call queued behind the last LM launch) - unless
        lock-step tracking already ran the pass for this pose object."""
        primed, self._primed.occlusion = self._primed.occlusion, None
        if primed is not None and self._primed.pose is pose and self.occlusion is not None:
            self._occ_frame = primed
            return primed["mask"]
        own = self._own
        if self.occlusion is None or own is None or own.pose is not pose or own.depth is None:
            return mask
        return self._apply_occlusion(mask, own.depth, view20=own.view)

    def _occlusion_view(self, depth, view20):
        """What one view of a batched occlusion pass takes from this tracker for a mesh template's plane and its view
        record: (sensor, (sensor_q, delta_q)); None when the option is off or the frame has no sensor image."""
        if self.occlusion is None or self._depth_sensor is None:
            return None
        from ..occlusion import mesh_quanta

        self._check_sensor_size(int(depth.shape[0]), int(depth.shape[1]))
        return self._depth_sensor, mesh_quanta(self._occ_conf.delta, self.occlusion.sensor_depth_scale, view20)

    def _gate_points(self, ref, T_init, qcamera):
        """The refiner's point_gate: the LM's point mask of a frame whose occlusion pass ran - ref.valid minus the
        points whose projection at the start pose falls on the occluder plane (one launch, ahead of the LM's).  None:
        no pass ran this frame, the LM takes ref.valid.  The plane is the sensor option's (_apply_occlusion) or the
        other tracked meshes' (_apply_mutual_occlusion); each pass has its own record and event."""
        valid = None
        for frame in (self._occ_frame, self._mut_frame):
            if frame is not None:
                valid = self._gate_on_plane(frame, ref, ref.valid if valid is None else valid, T_init, qcamera)
        return valid

    def _gate_on_plane(self, frame, ref, valid_in, T_init, qcamera):
        """What the two occluder sources share: one pxt_points_visible launch on the frame's plane G, counted in the
        frame's own record, remembered in its ``gates``."""
        from ..occlusion import points_visible

        valid, _ = points_visible(ref.p3d, valid_in, T_init, qcamera, frame["occluder"], record=frame["record_buffer"])
        frame["gates"].append({"p3d": ref.p3d, "valid_in": valid_in, "valid": valid, "T_init": T_init, "camera": qcamera})
        frame["done"].record(torch.cuda.current_stream(self.device))
        return valid

    def _enqueue_depth_refine(self, prob, pending, qcamera):
        """The refiner's depth_hook: one pxt_depth_refine problem behind the LM launch `pending`, no host wait between
        them, on the sensor image `_stage_depth_sensor` uploaded.  None when the frame has no depth image (its pose
        stays the LM's).  A frame refined against several references queues one problem per reference; `_frame_policy`
        waits for all of them, so that the records and the sensor buffer are free when the next frame begins."""
        from ..depth_refinement import depth_refine_batch

        item = self._depth_problem(prob, pending, qcamera)
        if item is None:
            return None
        if self._depth_ws is None:
            self._depth_ws = torch.zeros(int(_lib.lib().pxt_depth_refine_workspace_bytes(1)), dtype=torch.uint8,
                                         device=self.device)
        return depth_refine_batch([item[0]], self._depth_conf, workspace=self._depth_ws, records=[item[1]])

    def _depth_problem(self, prob, pending, qcamera):
        """The problem _enqueue_depth_refine would launch, for a caller that launches the problems of several trackers
        in ONE pxt_depth_refine call (lock-step tracking): -> (problem dict, its pinned record), or None when the
        frame has no depth image."""
        from ..depth_refinement import MAX_POINTS, RECORD

        opt, sensor = self.depth_refine, self._depth_sensor
        if sensor is None:
            return None
        w, h = (int(round(float(x))) for x in qcamera.size.tolist())
        self._check_sensor_size(h, w)
        ref = prob["ref"]
        if ref.p3d.shape[0] > MAX_POINTS and not self._depth_warned_points:
            self._depth_warned_points = True
            logger.warning(f"depth_refine: {ref.p3d.shape[0]} points in a frame, the first {MAX_POINTS} are used")
        valid = prob.get("mask") if prob.get("mask") is not None else ref.valid  # (the occlusion option's gated mask)
        p3d, mask = ref.p3d[:MAX_POINTS], (None if valid is None else valid[:MAX_POINTS])
        if self._depth_slot == len(self._depth_recs):
            self._depth_recs.append(torch.zeros(RECORD, dtype=torch.float32).pin_memory())
        rec = self._depth_recs[self._depth_slot]
        self._depth_slot += 1
        return dict(points=p3d, mask=mask, sensor=sensor, sensor_scale=float(opt.sensor_depth_scale), camera=qcamera,
                    pose=pending, prior=opt.prior), rec

    def _initial_reference_ids(self, assets):
        """r9: the upright reference image named by $UPRIGHT_REF_IMG (:77-78)."""
        if assets is not None:
            upright_ref_img = assets["upright_ref_img"]
        else:
            upright_ref_img = self._upright_ref_img if self._upright_ref_img else os.environ["UPRIGHT_REF_IMG"]
        return [self.localizer.model3d.name2id[upright_ref_img]]

    def _render_aabb(self, assets):
        """r9: the render box is $OBJ_AABB (:85-86)."""
        return assets["aabb"] if assets is not None else ast.literal_eval(os.environ["OBJ_AABB"])

    # ------------------------------------------------------------------ relocalisation
    def _make_relocalizer(self, relocalizer):
        if relocalizer is None or relocalizer == "off":
            return None
        if relocalizer == "views":
            from ..relocalizer import Relocalizer

            return Relocalizer(self.localizer, render=self.get_reference_image, **self._reloc_options)
        if relocalizer == "mesh":
            from ..relocalizer import Relocalizer

            return Relocalizer(self.localizer, render_batch=self._draw_bank_views, depth=self.reloc_depth,
                               **self._reloc_options)
        if isinstance(relocalizer, str):
            raise ValueError(f"relocalizer must be 'off', 'views', 'mesh' or a Relocalizer (got {relocalizer!r})")
        return relocalizer

    def _draw_bank_views(self, poses):
        """The relocaliser's bank views of a mesh template: the reference view of ``MeshTemplate.requests`` at every
        pose (the reference camera, the template's supersample), up to 32 of them in ONE render_frame_batch call ->
        [uint8 [H, W, 3]].  The frame's own planes (_own, _primed) are not touched."""
        from .. import mesh_render as MR

        t, rcam = self.template, self._reference_camera()
        w, h = (int(round(float(x))) for x in rcam.size.tolist())
        requests = [(MR.view_record(rcam, pose, t.near, t.depth_q(pose)), w, h, t.supersample, ("rgb_u8",)) for pose in poses]
        if self.__dict__.get("_bank_ws") is None:
            self._bank_ws = MR.FrameBatchWorkspace()
        out = MR.render_frame_batch([(t.renderer, requests)], workspace=self._bank_ws, download_records=False)[0]
        return [o["rgb_u8"] for o in out]

    def relocalize(self, query):
        if self.relocalizer is not None and not self.cold_start:
            # called by run_single_frame after a failed frame: the NEXT frame is relocalised (_frame_setup)
            self._lost = True
            return
        if self.cold_start:
            self.camera = self.get_query_camera(query)
            self.cold_start = False
        if self.relocalizer is not None and self.pose is None:
            self._relocalize_from(query)
            return
        if self.pose is None:
            ref_img = self.localizer.model3d.dbs[self.reference_ids[0]]
            self.pose = Pose.from_Rt(ref_img.qvec2rotmat(), ref_img.tvec)
        self.relocalization_count += 1

    def _relocalize_from(self, query):
        """The pose of this query frame from the relocaliser; the reference image becomes the db view nearest to it by
        rotation (as start_segment picks it).  Keeps the last pose when every candidate's refinement failed."""
        image = query[1] if isinstance(query, tuple) else query
        if isinstance(image, (str, os.PathLike)):
            from ..utils.io import read_image

            image = read_image(image)
        # (the last ACCEPTED pose: self.pose may be a relocalised pose whose frame then failed the gate)
        if self.reloc_depth is not None and self._depth_sensor is not None:
            # (the frame's one staged upload, which depth_refine / occlusion read as well)
            w, h = (int(round(float(x))) for x in self.camera.size.tolist())
            self._check_sensor_size(h, w)
            res = self.relocalizer.localize(image, self.camera, last_pose=self._accepted_pose, sensor=self._depth_sensor)
        else:
            res = self.relocalizer.localize(image, self.camera, last_pose=self._accepted_pose)
        self.last_relocalization = res
        self._relocalized_frame = True
        self.relocalization_count += 1
        self._lost = False
        if res.pose is None:
            if self.pose is None:  # nothing better than the reference's cold start
                ref_img = self.localizer.model3d.dbs[self.reference_ids[0]]
                self.pose = Pose.from_Rt(ref_img.qvec2rotmat(), ref_img.tvec)
            return
        self.pose = res.pose
        if not self.keep_feature_history:
            self.localizer.refiner.features_dicts.pop(self.dynamic_id, None)
        self.dynamic_id, self.cache_hit = None, False
        # relocalizer="mesh": from here on the reference image is chosen by the side the camera sees (below)
        self._reference_by_side = self._mesh_relocalizer
        self.reference_ids = self._nearest_reference_ids(self.pose)

    def _view_sides(self, Rs, ts):
        """Unit vectors from the object's centre (the mean of the SfM points) to the camera centres of poses
        ``Rs`` [n, 3, 3], ``ts`` [n, 3]: which side of the object a camera sees, whatever its roll."""
        centre = self.__dict__.get("_object_centre")
        if centre is None:
            centre = self._object_centre = np.mean([p.xyz for p in self.localizer.model3d.points3D.values()], axis=0)
        d = -np.einsum("nji,nj->ni", np.asarray(Rs, np.float64), np.asarray(ts, np.float64)) - centre
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    def _nearest_reference_ids(self, pose):
        """The mapping image nearest to ``pose`` by rotation (as the reference ranks them).  After a relocalisation with
        relocalizer="mesh" the nearest by SIDE instead: a relocalised camera may be rolled by any angle against the
        mapping views (the bank holds rolls for that reason), a roll is a large geodesic distance to EVERY mapping
        image, and the nearest by rotation is then an image of another side of the object, most of whose points the
        frame does not see (measured: DESIGN 3.26)."""
        R_qry, t_qry = pose.numpy()
        dbs = self.localizer.model3d.dbs
        if self._reference_by_side:
            ids = sorted(dbs)
            sides = self._view_sides([dbs[r].qvec2rotmat() for r in ids], [dbs[r].tvec for r in ids])
            return [ids[int(np.argmax(sides @ self._view_sides([R_qry], [t_qry])[0]))]]
        return sorted(dbs, key=lambda r: geodesic_distance_for_rotations(R_qry, dbs[r].qvec2rotmat()))[:1]

    def start_segment(self, pose_init: Optional[Pose]):
        """Cold start of a frame SEGMENT that does not begin at the video's first frame (BASELINE configs[4]: one video cut
        into per-GPU segments).  The reference has no such entry point - its only cold start is the upright reference pose
        of frame 0 (:95-106) - so a segment head needs a pose from outside: ``pose_init``, or None to have the relocaliser
        find it on the segment's first frame (needs a tracker built with ``relocalizer``).  What follows is the
        reference's cold-start policy: image scales [4, 1], no mask, nearest reference image by rotation, cost threshold
        frozen again from this segment's first frame."""
        if pose_init is None and self.relocalizer is None:
            raise ValueError("start_segment(None) needs a tracker with a relocalizer")
        self.pose, self.cold_start, self.success = pose_init, True, True
        self._accepted_pose = pose_init
        self.cost_threshold, self.dynamic_id, self.cache_hit = None, None, False
        self._lost = False
        self._reference_by_side = False
        if pose_init is not None:
            self.reference_ids = self._nearest_reference_ids(pose_init)

    def get_query_camera(self, query):
        """Camera of the query stream from the frame size (EXIF-less pycolmap heuristic)."""
        image = query[1] if isinstance(query, tuple) else query
        if isinstance(image, (str, os.PathLike)):
            from ..utils.io import read_image

            image = read_image(image)
        h, w = int(image.shape[0]), int(image.shape[1])
        return PixCamera.from_colmap(infer_camera_from_image(w, h))

    # ------------------------------------------------------------------ reference selection
    def update_reference_ids(self):
        if self.cache_hit == True:  # noqa: E712  (kept: see Appendix D.2)
            return self.reference_ids
        # candidates: the current reference, then its covisible images (> 50 shared points), ranked by the
        # geodesic distance of their rotation to the current pose; ties keep this order (stable sort)
        curr = self.reference_ids[0]
        cache = self.__dict__.setdefault("_ref_candidates", {})  # static per model: rotations of each reference's candidates
        cand = cache.get(curr)
        if cand is None:
            dbs = self.localizer.model3d.dbs
            ids = list(dict.fromkeys([curr] + [k for k, v in self.covis[curr].items() if v > 50]))
            cand = cache[curr] = (ids, np.stack([dbs[r].qvec2rotmat() for r in ids]))
        ids, rots = cand
        if self._reference_by_side:  # (after a relocalisation with relocalizer="mesh": _nearest_reference_ids says why)
            dbs = self.localizer.model3d.dbs
            sides = self._view_sides(rots, [dbs[r].tvec for r in ids])
            self.reference_ids = [ids[int(np.argmax(sides @ self._view_sides(*[[x] for x in self.pose.numpy()])[0]))]]
            return self.reference_ids
        gd = geodesic_distances_to(self.pose.numpy()[0], rots)
        self.reference_ids = [ids[int(np.argmin(gd))]]
        return self.reference_ids

    # ------------------------------------------------------------------ NeRF reference + mask
    def _nerf_pose(self, pose):
        return sfm_to_nerf_pose(self.nerf2sfm, get_camera_in_world_from_pixpose(pose))

    def _reference_camera(self):
        key = float(self.reference_scale)
        if self._ref_cam_cache is None or self._ref_cam_cache[0] != key:
            self._ref_cam_cache = (key, PixCamera.from_colmap(self.localizer.model3d.cameras[1]).scale(key))
        return self._ref_cam_cache[1]

    def _views_coincide(self) -> bool:
        """Mask and reference cameras agree in (width, height, fx) - all that get_nerf_image reads from a camera
        (run_vis_on_poses.py:30-36); the answer only changes with the camera object or the reference scale."""
        if not self.fuse_identical_views or self.camera is None:
            return False
        key = (id(self.camera), float(self.reference_scale))
        if self._coincide_cache is None or self._coincide_cache[0] != key:
            vk = lambda cam: (int(cam.size[0]), int(cam.size[1]), float(cam.f[0]))
            self._coincide_cache = (key, vk(self._reference_camera()) == vk(self.camera))
        return self._coincide_cache[1]

    def get_reference_image(self, pose, keep: bool = False) -> torch.Tensor:
        """uint8 [H,W,3] NeRF render at ``pose`` with SfM camera 1 scaled by reference_scale.  The image the frame's mask
        call already made for this pose object is handed out once; ``keep``: it stays held for one more call (lock-step
        tracking asks in its phase A, get_dynamic_id again in phase C: the same tensor object)."""
        own = self._own if (self._own is not None and self._own.pose is pose) else None
        if own is not None and own.ref_u8 is not None:
            img = own.ref_u8
        elif self.template is not None:  # (a frame that rendered no mask: cold start, the frame after a failed one)
            own = self._draw_frame(pose, from_slot=False)
            img = own.ref_u8
        else:
            ref_camera = self._reference_camera()
            rgba = get_nerf_image_device(self.testbed, self._nerf_pose(pose), ref_camera, spp=self.spp)
            img = rgba_to_u8(rgba, 0.0)
            if keep and own is None:
                own = self._own = FramePlanes(pose=pose)
        if own is not None:
            own.ref_u8 = img if keep else None
        return img

    def create_dynamic_reference_image(self, pose):
        if self.reference_points == "render":
            return self._create_dynamic_reference_from_render(pose)
        if self.reference_points == "template":
            return self._create_dynamic_reference_from_template(pose)
        nerf_img = self.get_reference_image(pose)
        # (the reference hashes str(R); the id is only a dictionary key - the bytes of R serve, without numpy's
        # array printer on the per-frame host path)
        dynamic_id = hash(pose.numpy()[0].tobytes())
        features = self.localizer.refiner.extract_reference_features(self.reference_ids, pose, nerf_img)
        return dynamic_id, features

    def _create_dynamic_reference_from_render(self, pose):
        """create_dynamic_reference_image with reference_points="render": the points come from the frame's Depth render
        at ``pose`` - the one get_mask made (or the render queued behind the last LM launch); a frame that renders no
        mask (cold start, the frame after a failed one) renders Depth + reference here."""
        own = self._own
        if own is None or own.pose is not pose or own.depth is None:
            own = self._draw_frame(pose, from_slot=False)
        depth, own.depth = own.depth, None
        nerf_img = self.get_reference_image(pose)
        dynamic_id = hash(pose.numpy()[0].tobytes())
        features = self.localizer.refiner.extract_reference_features(self.reference_ids, pose, nerf_img, depth=depth,
                                                                     depth_view=self._depth_view(pose))
        return dynamic_id, features

    def _create_dynamic_reference_from_template(self, pose):
        """create_dynamic_reference_image with reference_points="template": the points come from the depth plane the
        mesh template drew for the query view at ``pose`` and the view record it was drawn with - the ones
        _mask_and_reference kept; a frame that renders no mask (cold start, the frame after a failed one) draws its frame
        here.  Points that lock-step tracking already extracted for this pose object are taken as they are."""
        points, self._primed.points = self._primed.points, None
        depth = view20 = None
        own = self._own
        if points is None or self._primed.pose is not pose:
            points = None
            if own is None or own.pose is not pose or own.depth is None:
                own = self._draw_frame(pose, from_slot=False)
            depth, view20 = own.depth, own.view
        if own is not None:
            own.depth = own.view = None
        ref_u8 = self.get_reference_image(pose)
        dynamic_id = hash(pose.numpy()[0].tobytes())
        features = self.localizer.refiner.extract_reference_features(self.reference_ids, pose, ref_u8, depth=depth,
                                                                     depth_view=view20, points=points)
        return dynamic_id, features

    def _depth_view(self, pose) -> dict:
        """The view record of the frame's Depth render at ``pose`` for refiner.points_from_render: xform = [M | b], the
        render's camera-to-ngp matrix (the 12 floats the renderer used) chained with ngp -> SfM object coordinates, in
        float64; focal and k1 as the render's view record holds them."""
        from ..ngp import ngp_to_sfm_affine, nerf_matrix_to_ngp

        snap = self.testbed._snap
        A = self.__dict__.get("_ngp2sfm")
        if A is None:
            A = self._ngp2sfm = ngp_to_sfm_affine(self.nerf2sfm, float(snap.scale), float(snap.offset))
        cam = nerf_matrix_to_ngp(np.asarray(self._nerf_pose(pose))[:3, :], snap.scale, snap.offset)
        cam = np.asarray(cam, np.float32).astype(np.float64)
        xform = np.concatenate([A[:, :3] @ cam[:, :3], (A[:, :3] @ cam[:, 3] + A[:, 3])[:, None]], axis=1)
        width, height, fov = self._frame_views()[0]
        view = self.testbed._view_for(width, height, fov)
        return {"xform": xform.reshape(-1).tolist(), "focal": view[12], "k1": view[13], "depth_scale": 1.0 / float(snap.scale)}

    def get_dynamic_id(self, pose):
        features_dicts = self.localizer.refiner.features_dicts
        if self.dynamic_id is None:
            self.dynamic_id, features = self.create_dynamic_reference_image(self.pose)
            features_dicts[self.dynamic_id] = {"pose": self.pose, "features": features}
            return self.dynamic_id
        # THRESH = 0 in the reference: a geodesic distance is never < 0, so every frame after
        # the first is a miss and renders a fresh reference (pixloc_tracker_r9.py:171-203).
        self.THRESH = 0
        self.cache_hit = False
        old_id = self.dynamic_id
        self.dynamic_id, features = self.create_dynamic_reference_image(self.pose)
        if not self.keep_feature_history:
            features_dicts.pop(old_id, None)
        features_dicts[self.dynamic_id] = {"pose": self.pose, "features": features,
                                           "ref_ids": self.update_reference_ids()}
        self.misses += 1
        self.cache_hit = True
        return self.dynamic_id

    def get_mask(self, pose) -> torch.Tensor:
        """uint8 [H,W] on the device: depth render != 0, erode 5x5 x1, dilate 5x5 x5."""
        ok, self._ahead_ok = self._ahead_ok, None
        if ok is not None and ok.pose is pose:
            # (it also baked in focal length, size, spp, lens, render box, background and minimum transmittance as they were
            # when it was enqueued: it stands in for this frame's render only if they are what this frame would use)
            if ok.keys == self._ahead_views_now():
                self.renders_ahead_used += 1
                self._own, depth = ok, ok.depth
                if self.reference_points != ("render" if self.template is None else "template"):
                    ok.depth = ok.view = None  # (the frame's points are not taken from it: not held)
                if self.template is not None:  # (with its depth plane comes the host's bit-equal view record)
                    return self._apply_template_occlusion(ok.mask, pose)
                return self._apply_occlusion(ok.mask, depth)
            self.renders_ahead_stale += 1
        planes = self._draw_frame(pose, from_slot=False)
        if self.template is not None:
            return self._apply_template_occlusion(planes.mask, pose)
        return self._apply_occlusion(planes.mask, planes.depth)

    def _frame_views(self):
        """(width, height, fov in degrees on x) of the frame's renders as get_nerf_image sets them up
        (run_vis_on_poses.py:30-38): [query camera] when mask and reference cameras coincide (one march yields both
        images), else [query camera (Depth), reference camera (Shade)]."""
        import math

        def fov_of(cam):
            w, h = (int(v) for v in cam.size)
            return w, h, math.atan(w / (float(cam.f[0]) * 2)) * 2 * 180 / np.pi

        return [fov_of(self.camera)] if self._views_coincide() else [fov_of(self.camera), fov_of(self._reference_camera())]

    def _mask_and_reference(self, pose, from_slot: bool):
        """(mask, ref_u8) of ``_draw_frame``."""
        planes = self._draw_frame(pose, from_slot)
        return planes.mask, planes.ref_u8

    def _draw_frame(self, pose, from_slot: bool) -> FramePlanes:
        """The frame's mask and 8-bit reference image at one pose (reference :145-152, :207-214): ONE march when the two
        views coincide, otherwise the Depth render (query camera) and the Shade render (reference camera) as one chain of
        launches on this stream.  ``from_slot``: the camera is the one the LM kernel ahead in the stream derived from its
        final pose (render-ahead); otherwise the host's conversion of ``pose``.  Returns the planes as a record, which is
        also kept as ``_own`` when a pose object is given.  With reference_points="render" or ``occlusion`` the Depth
        render also keeps its float image (``depth``).  With a mesh template both planes come from one
        ``MeshTemplate.frame`` call instead - or from the call lock-step tracking made for this pose object (``_primed``);
        everything after them is the same.  With reference_points="template" that call also writes the query view's
        float depth plane, kept with the view record it was drawn with (``depth``, ``view``)."""
        if self.template is not None:
            primed = self._primed
            mutual = depth = view20 = None
            if primed.depth_nz is not None and pose is not None and primed.pose is pose:
                # drawn with the other objects' frames (``mutual``: ... as part of a scene)
                nz, ref_u8, mutual = primed.depth_nz, primed.ref_u8, primed.mutual
                self.template_frames_batched += 1
            elif self.reference_points == "template":
                # (the view record the plane is drawn with is the one the points are back-projected through)
                requests = self.template.requests(pose, self.camera, self._reference_camera(), want_depth=True)
                nz, ref_u8, depth = self.template.frame(pose, self.camera, self._reference_camera(), want_depth=True,
                                                        requests=requests)
                view20 = requests[0][0]
            else:
                nz, ref_u8 = self.template.frame(pose, self.camera, self._reference_camera())
            primed.depth_nz = primed.ref_u8 = primed.mutual = None  # (handed out once; for another pose: dropped)
            occ = primed.occlusion
            # (a primed occlusion pass of this pose was fed the plain mask of this very plane: not made again)
            mask = occ["mask_in"] if (occ is not None and pose is not None and primed.pose is pose) else self._mask_of(nz)
            if mutual is not None:
                mask = self._apply_mutual_occlusion(mask, mutual)
            planes = self._own = FramePlanes(pose=pose, mask=mask, ref_u8=ref_u8, depth=depth, view=view20)
            return planes
        tb, spp = self.testbed, int(self.spp)
        want_depth = self.reference_points == "render" or self.occlusion is not None
        if not from_slot:
            tb.set_nerf_camera_matrix(np.asarray(self._nerf_pose(pose))[:3, :])
        views = self._frame_views()
        width, height, fov_q = views[0]
        if len(views) == 1:
            tb.fov = fov_q
            out = tb.render_frame_device(width, height, spp, mode=2, from_slot=from_slot,
                                         want_float="depth" if want_depth else False)
            ref_u8, nz, depth = out["rgb_u8"], out["depth_nz"], out.get("depth")
        elif want_depth:
            nz, ref_u8, depth = tb.render_frame_pair_device(views[0], views[1], spp, from_slot=from_slot, depth_float=True)
        else:
            nz, ref_u8 = tb.render_frame_pair_device(views[0], views[1], spp, from_slot=from_slot)
            depth = None
        planes = FramePlanes(pose=pose, mask=self._mask_of(nz), ref_u8=ref_u8, depth=depth)
        if pose is not None:
            self._own = planes
        return planes

    def _mask_of(self, nz):
        """get_mask's morphology on the `uint8(depth * 255) != 0` plane a render wrote: erode 5x5 once, dilate 5x5 five
        times (:211-213)."""
        mask = torch.empty(nz.shape[0], nz.shape[1], dtype=torch.uint8, device=self.device)
        ops.depth_mask_plane(nz, 1, 5, mask)
        return mask

    def _lm_camera(self):
        """What the refiner hands to the LM launch of a frame whose next render will be queued behind it: the pose ->
        camera conversion constants, the renderer camera slot(s) to fill, and a pinned record for the host's check."""
        conv = self.__dict__.get("_pose_conv")
        if conv is None:
            conv = self._pose_conv = self.testbed.pose_conversion(self.nerf2sfm)
        slots = [self.testbed.camera_slot()]
        if not self._views_coincide():  # the pair's Shade render runs through the testbed's second context
            slots.append(self.testbed.camera_slot(side=True))
        self._ahead_cam = self.testbed._next_cam_out()
        return conv, slots, self._ahead_cam

    # ------------------------------------------------------------------ the next frame's render, ahead of the host
    def _render_ahead(self, pending):
        """Called between the LM launch and the wait for its result: the mask + reference render(s) of the NEXT frame, whose
        camera the LM kernel's epilogue writes into the renderer's camera slot(s)."""
        keys = self._ahead_views_now()
        self._ahead = self._draw_frame(None, from_slot=True)
        self._ahead.cams, self._ahead.keys = [self._ahead_cam], keys

    def _render_ahead_mesh_request(self):
        """The mesh template's queued frame for a caller that draws several trackers' in one call (lock-step tracking,
        MeshTemplate.frames_ahead): -> (requests, want_depth, the view keys the frame bakes in)."""
        want_depth = self.reference_points == "template"
        requests = self.template.requests_ahead(self.camera, self._reference_camera(), want_depth)
        return requests, want_depth, self._ahead_view_keys(requests)

    def _render_ahead_mesh_accept(self, rows, keys, depth_nz, ref_u8, depth=None):
        """What _render_ahead_mesh() does after its call: ``rows`` = the views_out rows of this tracker's views, then
        the planes the call drew for them."""
        self._ahead = FramePlanes(mask=self._mask_of(depth_nz), ref_u8=ref_u8, depth=depth, cams=rows, keys=keys)

    def _render_ahead_mesh(self, pending):
        """_render_ahead with a mesh template: ONE posed call on this stream behind the LM launch, whose output record
        (``pending.buf``) the call's first launch turns into the views' records on the device."""
        from ..mesh_render import VIEW_OUT, W_VIEW_DONE, FrameBatchWorkspace
        from ..mesh_template import MeshTemplate

        if self._ahead_ws is None:
            self._ahead_ws, self._ahead_rows = FrameBatchWorkspace(), PinnedRing((2, VIEW_OUT), torch.float32)
        requests, want_depth, keys = self._render_ahead_mesh_request()
        rows = self._ahead_rows.next(len(requests))  # (one block per frame, read back at that frame's end)
        rows[:, W_VIEW_DONE] = 0.0
        planes = MeshTemplate.frames_ahead([self.template], [pending.buf], [self.camera], [self._reference_camera()],
                                           self._ahead_ws, rows, want_depth=[want_depth], requests=[requests])[0]
        self._render_ahead_mesh_accept(rows, keys, *planes)

    def _ahead_view_keys(self, requests):
        """Per view of a mesh template's frame what a queued call bakes in besides the pose: size, supersample, outputs,
        fx fy cx cy, near and the renderer."""
        return [(tuple(float(x) for x in v[12:17]), int(W), int(H), int(S), tuple(want), id(self.template.renderer))
                for v, W, H, S, want in requests]

    def _render_ahead_request(self):
        """For a caller that merges the queued renders of several trackers into one batched chain (lock-step tracking,
        Testbed.render_frame_batch_device): (width, height, spp) of this tracker's one-march mask + reference render with
        the testbed's view set for it - or None when the frame's render is not of that kind (two different cameras), in
        which case _render_ahead() is to be called as usual."""
        if not self._views_coincide():
            return None
        width, height, self.testbed.fov = self._frame_views()[0]
        return int(width), int(height), int(self.spp)

    def _render_ahead_accept(self, out):
        """What _render_ahead() does after its render, for a render that was part of a batched chain."""
        self._ahead = FramePlanes(mask=self._mask_of(out["depth_nz"]), ref_u8=out["rgb_u8"], cams=[self._ahead_cam],
                                  keys=self._ahead_views_now())

    def _ahead_views_now(self):
        """What a render queued now bakes in besides the camera pose, per render of the frame: focal length, lens, render
        box, background, minimum transmittance (floats 12.. of the view record), image size and spp - the keys
        get_mask / get_reference_image would render with right now."""
        if self.template is not None:
            return self._render_ahead_mesh_request()[2]
        spp = int(self.spp)
        return [(tuple(self.testbed._view_for(w, h, fov)[12:]), w, h, spp) for w, h, fov in self._frame_views()]

    def verified_ahead(self) -> Optional[FramePlanes]:
        """The frame that was drawn ahead and verified, if it is valid for the present pose and view settings - what
        get_mask will take this frame - else None."""
        ok = self._ahead_ok
        return ok if (self.success and ok is not None and ok.pose is self.pose and ok.keys == self._ahead_views_now()) else None

    def armed_ahead(self) -> Optional[str]:
        """Which render-ahead this frame's set-up armed behind the LM launch: "nerf" (_render_ahead), "mesh"
        (_render_ahead_mesh) or None."""
        if getattr(self.localizer.refiner, "after_lm_enqueued", None) is None:
            return None
        return "nerf" if self.template is None else "mesh"

    def _verify_render_ahead(self, success: bool):
        """The render queued behind the LM launch is kept for the next frame only if the pose was accepted and the
        host, going through the reference's own conversion chain, arrives at the 12 camera floats the device used."""
        ahead, self._ahead = self._ahead, None
        self._ahead_ok = None
        if ahead is None or not success:
            return
        if self.template is not None:
            return self._verify_mesh_render_ahead(ahead)
        self.testbed.set_nerf_camera_matrix(np.asarray(self._nerf_pose(self.pose))[:3, :])
        want = np.asarray(self.testbed._cam_ngp, np.float32).reshape(-1)
        for cam_out in ahead.cams:
            got = cam_out.numpy()
            for _ in range(200000):  # the camera kernel runs right behind the LM kernel whose result is already here
                if got[12] != 0.0:
                    break
            else:  # never arrived: the queued render is dropped (and counted), the frame renders as usual
                self.renders_ahead_dropped += 1
                return
            if not np.array_equal(want.view(np.uint32), got[:12].view(np.uint32)):
                self.renders_ahead_rejected += 1
                return
        ahead.pose, ahead.cams = self.pose, None
        self._ahead_ok = ahead

    def _verify_mesh_render_ahead(self, ahead):
        """_verify_render_ahead with a mesh template: every view of the queued call was drawn with the 20 floats the host
        forms from the accepted pose - ``view_record`` with ``template.depth_q`` - bit for bit, or the planes are not
        used.  With reference_points="template" the host's query record goes with the depth plane: it is the record the
        plane was drawn with."""
        from ..mesh_render import W_VIEW_DONE, view_record

        got = ahead.cams.numpy()
        cameras = [self.camera] if len(ahead.keys) == 1 else [self.camera, self._reference_camera()]
        q = self.template.depth_q(self.pose)
        want_q = None
        for row, camera in zip(got, cameras):
            for _ in range(200000):  # the call's first launch runs right behind the LM kernel whose result is already here
                if row[W_VIEW_DONE] != 0.0:
                    break
            else:  # never arrived: the queued frame is dropped (and counted), the frame renders as usual
                self.renders_ahead_dropped += 1
                return
            want = view_record(camera, self.pose, self.template.near, q)
            if row[W_VIEW_DONE] != 1.0 or not np.array_equal(want.view(np.uint32), row[:20].view(np.uint32)):
                self.renders_ahead_rejected += 1
                return
            want_q = want if want_q is None else want_q
        ahead.pose, ahead.cams, ahead.view = self.pose, None, (None if ahead.depth is None else want_q)
        self._ahead_ok = ahead

    # ------------------------------------------------------------------ one frame
    def refine(self, query):
        query_path, query_image = query
        refiner = self.localizer.refiner
        self._depth_frame_name = query_path
        self._occ_frame = self._mut_frame = self._primed.occlusion = None
        if self.depth_refine is not None or self.occlusion is not None or self.reloc_depth is not None:
            self._stage_depth_sensor(query_path)
        self._frame_setup(query)
        if self.occlusion is not None and self._depth_sensor is not None:
            # (on every frame, also one that gets no mask: a wrong sensor directory is not found out frames later)
            w, h = (int(round(float(x))) for x in self.camera.size.tolist())
            self._check_sensor_size(h, w)
        self.dynamic_id = self.get_dynamic_id(self.pose)
        trackers, rets, costs = {}, {}, {}
        for ref_id in self.reference_ids:
            pose_init = self._frame_pose_init()
            tracker = DebugTracker(refiner, self.debug)
            ret = self.localizer.run_query(query_path, self.camera, pose_init, [ref_id], image_query=query_image,
                                           pose=self.pose, reference_images_raw=None, dynamic_id=self.dynamic_id)
            rets[ref_id] = ret
            trackers[ref_id] = tracker
            costs[ref_id] = self._frame_cost()
        return self._frame_policy(query_path, rets, costs, trackers)

    def _frame_setup(self, query, lockstep: bool = False) -> str:
        """The head of refine() (reference :216-227): cold start -> image scales [4, 1] from the relocalised pose; a
        tracked frame -> scale [1] with the query masked by the silhouette at the last pose; after a failed frame no
        mask and whatever scales were last set (Appendix D.3).  Arms the extractor's two-image pass and the render that
        rides behind the LM launch.  Returns "cold" / "steady" / "plain".  ``lockstep``: the frame's two UNet passes
        and its LM launch are batched with other objects' by the caller (multi_object_tracker.py), which hands the
        maps over through the extractor's preload() - nothing is staged here."""
        query_path, query_image = query
        refiner = self.localizer.refiner
        refiner.query_mask = None
        kind = "plain"
        if self.cold_start:
            refiner.conf.multiscale = [4, 1]
            self.relocalize(query)
            self.cold_start = False
            kind = "cold"
        elif self._lost:
            # relocaliser on and the last frame failed: relocalise, then the cold-start policy from that pose (image scales
            # [4, 1], no mask); the cost gate stays frozen
            refiner.conf.multiscale = [4, 1]
            self._relocalize_from(query)
            kind = "cold"
        elif self.success:
            refiner.conf.multiscale = list(self.steady_multiscale)
            refiner.query_mask = self.get_mask(self.pose)  # multiplied inside the first conv

        # The masked query is fully known here, before the reference render is encoded: announce it so both images of
        # the frame go through the UNet in one batched pass.
        if not lockstep and self.batch_frame_images and refiner.conf.multiscale == [1]:
            refiner.feature_extractor.stage(query_image, 1, refiner.query_mask, True)
        else:
            refiner.feature_extractor.unstage()
        # one refinement, at full scale, of a tracked frame: its LM launch can carry the next frame's render(s)
        # behind it (one march when mask and reference views coincide, two renders otherwise)
        steady = (kind != "cold" and self.success and refiner.query_mask is not None
                  and refiner.conf.multiscale == [1] and len(self.reference_ids) == 1)
        self._ahead = None
        # (a mesh template's queued call reads the LM's pose record itself: no camera epilogue.  Objects that hide each
        # other are drawn as scenes at the head of a step: not ahead)
        mesh = self.template is not None
        ahead = self.render_ahead and steady and not (mesh and self.mutual_occlusion)
        refiner.after_lm_enqueued = (self._render_ahead_mesh if mesh else self._render_ahead) if ahead else None
        refiner.lm_camera = self._lm_camera if (ahead and not mesh) else None
        # the query computes only its LM's tiles on a steady frame of the staged pair pass, where nothing else reads its
        # fine map: no dense-map log, no relocaliser scoring, none of the opt-ins the refiner itself checks
        refiner.query_tiles = None
        refiner.after_query_tile_fallback = self._query_tile_fallback
        if self._query_tile_rest > 0:
            self._query_tile_rest -= 1
        elif (self.query_tiles and steady and not lockstep and self.batch_frame_images and self.debug < 2
              and self.relocalizer is None and self.reference_points == "sfm"):
            refiner.query_tiles = {"pose": self._frame_pose_init(), "camera": self.camera,
                                   "margin": int(self.query_tile_margin)}
        return "steady" if steady else kind

    def _query_tile_fallback(self):
        """The LM's tile guard ended this frame's launch (the refiner redoes the frame in full): the render queued behind
        that launch goes the way of a rejected one, and the option rests for the next 8 frames - a sequence whose motion
        exceeds the margin does not pay the redo on every frame."""
        self.query_tile_fallbacks += 1
        self._query_tile_rest = 8
        if self._ahead is not None:
            self._ahead = None
            self.renders_ahead_rejected += 1

    def _frame_pose_init(self) -> Pose:
        rotation, translation = self.pose.numpy()
        rotation = R.from_matrix(rotation).as_matrix()
        return Pose.from_Rt(rotation, translation)

    def _frame_cost(self) -> float:
        """mean over (scale, level) runs of the LAST logged cost; taken from the kernel log so it
        does not depend on --debug (the reference yields NaN with --debug 0, Appendix D.1)"""
        last = [c[-1] for res in self.localizer.refiner.last_lm for c in res.costs if len(c)]
        return float(np.mean(last)) if last else float("nan")

    def _frame_policy(self, query_path, rets, costs, trackers) -> bool:
        """The tail of refine() (reference :251-275): best reference by cost, the cost gate frozen from the first
        frame, pose update, history."""
        refiner = self.localizer.refiner
        avg_cost = costs[self.reference_ids[-1]]
        if hasattr(self, "pbar") and hasattr(self.pbar, "set_description"):
            self.pbar.set_description(f"Cost: {avg_cost}, Relocalizations: {self.relocalization_count}")
        best_ref_id = min(costs, key=costs.get)
        ret = rets[best_ref_id]

        if self.cost_threshold is None:
            thresh = min(costs.values())
            self.cost_threshold = thresh + 0.1 * thresh

        success = bool(ret["success"] and min(costs.values()) <= self.cost_threshold)
        if self.depth_refine is not None:  # (added keys only where the option is on; the LM decided `success` above)
            from ..depth_refinement import accept, decode_record

            handles = {k: r.pop("depth_pending", None) for k, r in rets.items()}
            records = {k: None if h is None else h.result()[0] for k, h in handles.items()}  # (waits for every one)
            rec = decode_record(records[best_ref_id]) if records[best_ref_id] is not None else None
            ret["T_lm"] = ret.get("T_refined")
            ret["depth_refined"] = accept(rec, success)
            seen = rec is not None and rec["status"] != -1.0
            ret["depth_cost_before"] = rec["cost_before"] if seen else None
            ret["depth_cost_after"] = rec["cost_after"] if seen else None
            ret["depth_n_valid"] = rec["n_valid_after"] if seen else 0
            ret["depth_iters"] = rec["iterations"] if seen else 0
            if ret["depth_refined"]:
                ret["T_refined"] = Pose(torch.from_numpy(rec["T"]).double())
        if self.occlusion is not None:  # (added keys only where the option is on; nothing above read them)
            # the pinned record: its launches sit ahead of the LM launch whose result is here (the event is over by then;
            # it is waited for only on a frame that ended before any LM launch)
            frame, self._occ_frame = self._occ_frame, None
            if frame is not None:
                frame["done"].synchronize()
            rec = None if frame is None else [int(x) for x in frame["record_buffer"].tolist()]
            ret["occluded_fraction"] = None if rec is None else (rec[2] / rec[0] if rec[0] else 0.0)
            ret["n_occluder_pixels"] = 0 if rec is None else rec[4]
            ret["n_points_gated"] = 0 if rec is None else rec[9] - rec[10]
            ret["occlusion_applied"] = rec is not None
            if frame is not None:
                frame["record"] = rec
            self.last_occlusion = frame
        if self.mutual_occlusion:  # (added keys only where the option is on; nothing above read them)
            # the pinned records: their launches sit ahead of the LM launch whose result is here (the sensor option's
            # pattern: the event is over by then)
            frame, self._mut_frame = self._mut_frame, None
            rec = scene = None
            if frame is not None:
                self._mut_done.synchronize()
                rec = [int(x) for x in self._mut_record.tolist()]
                scene = [int(x) for x in self._mut_scene.tolist()]
                frame["record"], frame["scene_record"] = rec, scene
            ret["mutual_occlusion_applied"] = frame is not None
            ret["n_mutually_hidden_pixels"] = 0 if scene is None else scene[10]
            ret["mutually_hidden_fraction"] = None if scene is None else (scene[10] / scene[0] if scene[0] else 0.0)
            ret["n_mutual_occluder_pixels"] = 0 if scene is None else scene[11]
            ret["n_points_gated_mutual"] = 0 if rec is None else rec[9] - rec[10]
            self.last_mutual_occlusion = frame
        if success:
            self.pose = self._accepted_pose = ret["T_refined"]
        self.success = success
        refiner.after_lm_enqueued = None
        refiner.lm_camera = None
        self._verify_render_ahead(success)
        # (`success` stays what the refiner said, as in the reference's poses.pkl; `tracked` - an added key - is the tracker's
        # decision: refiner success AND the cost gate.  bench.py and the pose gather count THIS one.)
        ret["tracked"] = success
        ret["camera"] = self.camera
        if self.relocalizer is not None:  # (an added key only where the option is on: the default history is unchanged)
            ret["relocalized"], self._relocalized_frame = self._relocalized_frame, False
            if ret["relocalized"]:  # (None without the depth stage; nothing on the policy path reads them)
                res = self.last_relocalization
                ret["reloc_n_placed"], ret["reloc_n_geometric"] = res.n_placed, res.n_geometric
        if self.reference_points != "sfm":  # (added keys only where the option is on)
            # the pinned record of this frame's extraction: its kernels ran ahead of the LM launch whose result is here
            rec = refiner.last_points_record
            ret["n_reference_points"], ret["reference_point_stride"] = (int(rec[2]), int(rec[1])) if rec is not None else (0, 0)
        if self.template is not None:  # (added keys only where the option is on)
            ret["template"], ret["template_supersample"] = "mesh", int(self.template.supersample)
        ret["reference_ids"] = self.reference_ids
        ret["query_path"] = query_path
        ret["cost"] = costs[best_ref_id]
        img_name = os.path.basename(str(query_path))
        self.pose_history[img_name] = ret
        self.pose_tracker_history[img_name] = trackers[best_ref_id]
        return success

    def get_query_frame_iterator(self, image_folder, max_frames):
        return image_folder if isinstance(image_folder, (ArrayIterator, ImageIterator)) else ImageIterator(image_folder, max_frames)

    def save_poses(self, pixloc_pickles: bool = False):
        """poses.pkl (reference :281-284).  ``pixloc_pickles`` writes Pose/Camera under pixloc's
        class path so the reference's own tools (run_vis_on_poses.py, GetMetrics.ipynb) load it."""
        _dump(self.pose_history, os.path.join(self.eval_path, "poses.pkl"), pixloc_pickles)


def _dump(obj, path, pixloc_pickles: bool):
    if pixloc_pickles:
        from ..utils.io import dump_reference_pickle

        dump_reference_pickle(obj, path)
    else:
        with open(path, "wb") as f:
            pkl.dump(obj, f)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument("--object_path", type=Path)
    parser.add_argument("--query", type=Path)
    parser.add_argument("--out_dir", type=Path)
    parser.add_argument("--frames", type=int, default=None)
    parser.add_argument("--debug", type=int, default=0)
    parser.add_argument("--pixloc_pickles", action="store_true",
                        help="write poses.pkl/trackers.pkl with pixloc's Pose/Camera class paths")
    parser.add_argument("--unet_precision", choices=("fp16", "fp32"), default="fp16",
                        help="UNet activations: fp16 (default, fastest) or fp32 (pixloc's precision)")
    parser.add_argument("--uncertainty", action="store_true",
                        help="add the pose information matrix, covariance and observability of every frame to poses.pkl")
    parser.add_argument("--point_report", choices=("off", "summary", "full"), default="off",
                        help="add every frame's valid / inlier point counts and mean robust weight to poses.pkl (summary), "
                             "and the per-point projections, residuals and weights as well (full)")
    parser.add_argument("--reference_points", choices=("sfm", "render", "template"), default="sfm",
                        help="the points a frame is refined on: sfm (default: the SfM points of the nearest mapping image), "
                             "render (a lattice of the frame's own depth render, back-projected) or template (--template "
                             "mesh: the same lattice of the depth plane the mesh template draws for the frame)")
    parser.add_argument("--depth_refine", action="store_true",
                        help="refine every frame's pose on its sensor depth image after the LM (needs --sensor_depth_dir "
                             "and --sensor_depth_scale; with --template mesh: --reference_points template)")
    parser.add_argument("--sensor_depth_dir", type=Path, default=None, help="the 16-bit depth images, one per frame")
    parser.add_argument("--sensor_depth_scale", type=float, default=None, help="SfM units per raw count")
    parser.add_argument("--sensor_depth_template", default="{stem}.png",
                        help="file name of a frame's depth image: {stem} / {name} of the frame (default {stem}.png)")
    parser.add_argument("--sensor_depth_sub", nargs=2, metavar=("OLD", "NEW"), default=None,
                        help="replace OLD by NEW in the frame's name first (YCB-Video: color depth)")
    parser.add_argument("--depth_prior", nargs=2, type=float, metavar=("WT", "WR"), default=None,
                        help="diagonal prior on the depth refinement's accumulated update: translation, rotation weight")
    parser.add_argument("--occlusion_mask", action="store_true",
                        help="take the pixels where the sensor depth image lies in front of the object out of every "
                             "frame's mask and point set (needs --sensor_depth_dir and --sensor_depth_scale; with "
                             "--template mesh: --reference_points template)")
    parser.add_argument("--occlusion_delta", type=float, default=None,
                        help="how much closer the sensor's surface must be, as a fraction of the model's extent (default 0.1)")
    parser.add_argument("--occlusion_radii", nargs=2, type=int, metavar=("OPEN", "GROW"), default=None,
                        help="box radii of the opening and the growth of the occluder plane (default 1 3)")
    parser.add_argument("--relocalize", choices=("off", "views", "mesh"), default="off",
                        help="off (default: cold start from the upright view, a lost track stays lost), views "
                             "(relocalise the cold start and the frame after a failed frame against the mapping views) or "
                             "mesh (the same with --template mesh: the bank's views are drawn by the mesh template)")
    parser.add_argument("--relocalize_depth", action="store_true",
                        help="--relocalize mesh: score a placement grid (lateral cell x distance per bank entry) against "
                             "the frame's sensor depth image first (needs --sensor_depth_dir and --sensor_depth_scale; "
                             "untuned defaults, relocalizer.RelocDepth)")
    parser.add_argument("--template", choices=("nerf", "mesh"), default="nerf",
                        help="what a frame's mask and reference image are rendered from: nerf (default: the object's "
                             "instant-ngp snapshot) or mesh (--mesh; no snapshot, nerf2sfm.pkl or $OBJ_AABB is read)")
    parser.add_argument("--mesh", type=Path, default=None,
                        help="--template mesh: the mesh, as mesh_dataset reads it (vertex colours, or a texture map)")
    parser.add_argument("--texture", type=Path, default=None, help="the texture map, in place of the one the mesh names")
    parser.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the mesh's vertices (BOP's models are in mm)")
    parser.add_argument("--mesh_supersample", type=int, choices=(1, 2, 4), default=2,
                        help="samples per pixel and axis of the mesh template's reference image (default 2, untuned)")
    parser.add_argument("--mesh_render_ahead", action="store_true",
                        help="--template mesh: queue the next frame's mesh views behind this frame's LM launch; their view "
                             "records are formed on the device from the LM's output record (default: off)")
    parser.add_argument("--reference_sfm", type=Path, default=None,
                        help="the SfM model's directory (the ref/ directory mesh_dataset wrote), in place of "
                             "<object_path>/pixtrack/aug_nerf_sfm/aug_sfm")
    parser.add_argument("--upright_ref_img", default=None,
                        help="the name of the upright reference image (default: $UPRIGHT_REF_IMG)")
    return parser


def template_from_args(args, device="cuda:0"):
    """--template mesh and its companions -> a mesh_template.MeshTemplate (None for the NeRF template)."""
    if getattr(args, "template", "nerf") != "mesh":
        if getattr(args, "mesh", None) is not None:
            raise ValueError("--mesh goes with --template mesh")
        return None
    if args.mesh is None:
        raise ValueError("--template mesh needs --mesh")
    from ..mesh_template import MeshTemplate

    return MeshTemplate.from_files(args.mesh, texture=args.texture, mesh_scale=args.mesh_scale, device=device,
                                   supersample=args.mesh_supersample,
                                   render_ahead=bool(getattr(args, "mesh_render_ahead", False)))


def _sensor_lookup_from_args(args, flag: str):
    """The frame name -> sensor depth image lookup of --sensor_depth_dir / _template / _sub, kept on ``args`` so that
    --depth_refine and --occlusion_mask share ONE (the tracker uploads a frame's image once for both).  A file missing
    before any was found raises (a wrong directory, template or substitution: not a run that silently does nothing);
    later ones are logged and the frame runs without its image."""
    if args.sensor_depth_dir is None or args.sensor_depth_scale is None:
        raise ValueError(f"{flag} needs --sensor_depth_dir and --sensor_depth_scale")
    lookup = getattr(args, "_sensor_lookup", None)
    if lookup is not None:
        return lookup
    from ..sensor_evaluation import read_sensor_depth, sensor_file_name

    found = []

    def lookup(frame_name):
        path = Path(args.sensor_depth_dir) / sensor_file_name(frame_name, args.sensor_depth_template, args.sensor_depth_sub)
        if path.is_file():
            found.append(path)
            return read_sensor_depth(path)
        if not found:
            raise FileNotFoundError(f"{flag}: no sensor depth image {path} for frame {frame_name}")
        logger.warning(f"{flag}: no sensor depth image {path}: {frame_name} runs without it")
        return None

    args._sensor_lookup = lookup
    return lookup


def depth_option_from_args(args):
    """--depth_refine and its companions -> a depth_refinement.DepthRefine (None when the option is off)."""
    if not getattr(args, "depth_refine", False):
        return None
    lookup = _sensor_lookup_from_args(args, "--depth_refine")
    from ..depth_refinement import DepthRefine

    return DepthRefine(lookup=lookup, sensor_depth_scale=float(args.sensor_depth_scale),
                       prior=tuple(args.depth_prior) if args.depth_prior else None)


def occlusion_option_from_args(args):
    """--occlusion_mask and its companions -> an occlusion.OcclusionMask (None when the option is off)."""
    if not getattr(args, "occlusion_mask", False):
        return None
    lookup = _sensor_lookup_from_args(args, "--occlusion_mask")
    from ..occlusion import OcclusionConf, OcclusionMask

    kw = {}
    if getattr(args, "occlusion_delta", None) is not None:
        kw["delta"] = float(args.occlusion_delta)
    if getattr(args, "occlusion_radii", None):
        kw["r_open"], kw["r_grow"] = (int(x) for x in args.occlusion_radii)
    return OcclusionMask(lookup=lookup, sensor_depth_scale=float(args.sensor_depth_scale), conf=OcclusionConf(**kw))


def reloc_depth_option_from_args(args):
    """--relocalize_depth and its companions -> a relocalizer.RelocDepth (None when the option is off)."""
    if not getattr(args, "relocalize_depth", False):
        return None
    lookup = _sensor_lookup_from_args(args, "--relocalize_depth")
    from ..relocalizer import RelocDepth

    return RelocDepth(lookup=lookup, sensor_depth_scale=float(args.sensor_depth_scale))


def main(argv=None):
    args = build_parser().parse_args(argv)
    data_path = args.object_path / "pixtrack/pixsfm/dataset"
    eval_path = args.out_dir
    loc_path = args.object_path / "pixtrack/aug_nerf_sfm"
    os.makedirs(eval_path, exist_ok=True)
    if torch.cuda.is_available():
        from ..parallel import bind_to_device_numa

        bind_to_device_numa(0)
    tracker = PixLocPoseTrackerR9(template=template_from_args(args), reference_sfm=args.reference_sfm,
                                  upright_ref_img=args.upright_ref_img,
                                  depth_refine=depth_option_from_args(args), occlusion=occlusion_option_from_args(args),
                                  reloc_depth=reloc_depth_option_from_args(args),
                                  object_path=str(args.object_path), data_path=str(data_path),
                                  eval_path=str(eval_path), loc_path=str(loc_path), debug=args.debug,
                                  unet_precision=args.unet_precision, relocalizer=args.relocalize,
                                  uncertainty=args.uncertainty, reference_points=args.reference_points,
                                  point_report=args.point_report)
    import gc

    gc.collect()
    gc.freeze()   # the assets stay; a generation-2 collection inside the frame loop is a 10 ms
    gc.disable()  # stall of the host that feeds the GPU
    try:
        tracker.run(args.query, max_frames=args.frames if args.frames is not None else np.inf)
    finally:
        gc.enable()
    tracker.save_poses(args.pixloc_pickles)
    print("Cache hits: %d, misses: %d" % (tracker.hits, tracker.misses))
    _dump(tracker.pose_tracker_history, os.path.join(tracker.eval_path, "trackers.pkl"), args.pixloc_pickles)
    print("Done")


if __name__ == "__main__":
    main()
