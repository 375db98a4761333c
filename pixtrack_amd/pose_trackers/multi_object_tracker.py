"""MultiObjectTracker -- K objects tracked in lock-step on ONE GPU.

The reference tracks one object per process: `pixloc_tracker_r9.py:287-318` builds one
``PixLocPoseTrackerR9`` from one ``config/<object>.sh`` and runs it over one video.  BASELINE configs[3]
("8 objects from config/*.sh tracked concurrently") on fewer than 8 GPUs means several such trackers per
GPU.  Running them one after the other (or as processes sharing the GPU) leaves the small stages of a
frame as they are: every tracker's deep UNet layers fill a third of the chip, every tracker's LM launch
pays its own inter-workgroup exchange and single-lane solve per iteration.  Here the K trackers keep
their own state and policy - each one IS a PixLocPoseTrackerR9, advanced through the same per-frame
methods - and only the device work of a frame step is merged:

* the 2 K images of a step (K reference renders, K masked queries) go through the UNet in ONE batched
  pass (``pxt_unet_forward_batch``): the 30x40 / 60x80 / decoder layers get 2 K x the workgroups;
* the K refinements run in ONE persistent launch (``pxt_lm_refine_batch``): workgroup i works on
  problem i mod K, an iteration's exchange and solve are paid once for all K;
* renders stay one renderer context per object (each object has its own NeRF), the render of step
  t + 1 queued behind the batched LM launch with the camera from the LM epilogue's slot, as in the
  one-object tracker;
* trackers with a mesh template (``template=MeshTemplate(...)``) have no NeRF: the frames of a group's
  mesh trackers - each one's depth_nz plane and reference image - are drawn at the head of the step in
  ONE call (``MeshTemplate.frames``, ``pxt_mesh_render_frame_batch``).  Both kinds may share a group.
* ``mutual_occlusion=MutualOcclusion(scenes=[...])`` (opt-in): mesh trackers that name one scene are objects in ONE
  image.  That call then also tells, per object, the pixels where another object of its scene lies in front
  (``pxt_mesh_render_scene_batch``); they leave the object's query mask, and the reference points that project onto them
  leave its LM's point mask.
* mesh templates built with ``render_ahead=True`` (opt-in): behind the batched LM launch the NEXT frames of the group's
  mesh trackers are drawn in ONE call whose view records are formed on the device from the LM's output records
  (``MeshTemplate.frames_ahead``, ``pxt_mesh_render_frame_batch_posed``); the next step's head-of-step call then draws
  only the trackers whose queued frame was not verified for their pose.  Not with ``mutual_occlusion``: a step's scenes
  are formed from who takes the lock-step path in that step, so its mesh trackers are not drawn ahead (tracking is
  unchanged).
* mesh trackers with ``reference_points="template"`` refine on a lattice of their own frame's depth plane: that call
  then also writes their query views' float depth planes, and ONE ``pxt_points_from_depth_views`` call behind it
  extracts the points of all of them (three launches for the group instead of three per object).

A tracker in cold start (image scales [4, 1]: two dependent refinements) runs that frame by itself
through ``run_single_frame``; everything else is lock-step.  Per object the results are those of the
one-object tracker: bit for bit with ``per_image_plan=True`` and ``lm_workgroups`` equal to the solo
grid (the UNet layers then take a single image's tile / split-K plan, the LM folds the same number of
partials); with the defaults (batch-planned layers: no split-K where the batch fills the chip; 256 / K
workgroups per problem) equal up to fp32 summation order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import os

import torch

from .. import _lib
from ..ops import ops
from ..optimizer import PixTrackOptimizer
from ..pinned import PinnedRing, SensorStage
from ..tracker import DebugTracker
from ..point_report import parse_mode
from .pixloc_tracker_r9 import PixLocPoseTrackerR9


@dataclass
class MutualOcclusion:
    """The lock-step option: ``scenes[k]`` = the scene of tracker k (any hashable; None: the tracker is alone).  The
    trackers of a scene see ONE image: same query camera (size, f, c; no lens terms), mesh templates.  ``r_grow``: the box
    radius by which the plane of hidden pixels is grown before it leaves the mask and gates the points (0..8).  The
    default 2 is an untuned starting value: nobody has run this on real multi-object sequences."""
    scenes: Sequence
    r_grow: int = 2


MUTUAL_HISTORY_KEYS = ("mutual_occlusion_applied", "n_mutually_hidden_pixels", "mutually_hidden_fraction",
                       "n_mutual_occluder_pixels", "n_points_gated_mutual")


def _same_scene_camera(a, b) -> bool:
    """Two query cameras see one image: equal size, f and c, no lens terms."""
    da, db = (c._data.detach().cpu().double().reshape(-1) for c in (a, b))
    return bool(torch.equal(da[:6], db[:6]) and not da[6:].any() and not db[6:].any())


def _chunks_by(items, key, limit: int):
    """What the step's batched calls share: ``items`` grouped by ``key(item)`` - the settings one call holds for all its
    views or problems; keys in first-seen order, compared with ``==`` - and each group cut into chunks of at most
    ``limit``, one chunk per call.  Yields (key, chunk)."""
    groups: list = []
    for item in items:
        k = key(item)
        for k0, members in groups:
            if k0 == k:
                members.append(item)
                break
        else:
            groups.append((k, [item]))
    for k, members in groups:
        for a in range(0, len(members), limit):
            yield k, members[a:a + limit]


class _Group:
    """The objects whose device work is merged: one stream, one UNet context (workspace), one LM batch workspace."""

    def __init__(self, index, members, stream, model):
        from ..mesh_render import VIEW_OUT
        from ..occlusion import MAX_VIEWS as OCC_MAX_VIEWS, RECORD as OCC_RECORD

        self.index, self.members, self.stream, self.model = index, members, stream, model
        self.batch_ws: Optional[torch.Tensor] = None
        self.info_ws: Optional[torch.Tensor] = None  # parameter records and partial sums of the step's information launch
        self.report_ws: Optional[torch.Tensor] = None  # ... and of the step's point-report launch
        self.render_ws: Optional[torch.Tensor] = None  # parameter records of the batched render chain
        self.mesh_ws = None  # mesh_render.FrameBatchWorkspace of the group's mesh-template frames (made on first use)
        self.points_ws: Optional[torch.Tensor] = None  # workspace of the step's pxt_points_from_depth_views call(s)
        self.points_records = PinnedRing((_lib.PXT_POINTS_MAX_VIEWS, 4), torch.int32)  # the records of those calls
        self.occ_ws: Optional[torch.Tensor] = None  # workspace of the step's pxt_occlusion_mask_views call(s)
        self.occ_records = PinnedRing((OCC_MAX_VIEWS, OCC_RECORD), torch.int32)  # the records of those calls
        self.depth_ws: Optional[torch.Tensor] = None  # workspace of the step's pxt_depth_refine call(s)
        self.sensor_slots: List[SensorStage] = []  # one per distinct sensor image of a step
        # views_out blocks of the group's MeshTemplate.frames_ahead calls (a step's rows are read at that step's end)
        self.ahead_rows = PinnedRing((64, VIEW_OUT), torch.float32)
        self.unet_done: Optional[torch.cuda.Event] = None
        self.pend = None  # what _enqueue left for _finish


class _OneDepth:
    """One problem's share of a batched pxt_depth_refine call, with the interface of the solo tracker's handle:
    ``result()`` waits for the call and returns [that problem's record]."""

    def __init__(self, pending, index: int):
        self.pending, self.index = pending, index

    def result(self):
        return [self.pending.result()[self.index]]


class MultiObjectTracker:
    def __init__(self, trackers: Sequence[PixLocPoseTrackerR9], lm_workgroups: int = 0, per_image_plan: bool = False,
                 max_unet_batch: int = _lib.PXT_UNET_MAX_BATCH, n_groups: int = 1, batch_renders: Optional[bool] = None,
                 uncertainty: Optional[bool] = None, point_report=None, mutual_occlusion: Optional[MutualOcclusion] = None):
        """``mutual_occlusion``: None (default) changes nothing - the same op, the same launches, the same poses and
        histories.  A ``MutualOcclusion`` assigns the mesh-template trackers to scenes.  Per step, the members of a scene
        that take the lock-step path are drawn as that scene (if there are at least two of them); a member that sits
        the step out or goes through ``run_single_frame`` (cold start, the frame after a failed frame, multiscale) is not
        part of the scene that step: it neither hides anything nor is hidden.  Each history entry gains
        ``MUTUAL_HISTORY_KEYS``.  ValueError: a scene with a tracker that has no mesh template; query cameras of a scene
        that differ in size, f or c or have lens terms (checked here where a tracker already has its camera, else at the
        first step that draws the scene); a scene that cannot be kept in one group; any tracker with
        ``reference_points="template"`` (not combined yet).
        Trackers built with ``reference_points="template"`` (mesh templates only; ``"render"`` stays refused) are accepted
        beside ``"sfm"`` ones: per step and group the points of all of them that take the lock-step path come from ONE
        pxt_points_from_depth_views call behind the frame call (``points_calls`` counts them); a tracker that runs a step
        alone extracts its own.
        Mesh-template trackers with ``reference_points="template"`` may carry ``occlusion`` and ``depth_refine`` (DESIGN
        3.23; NeRF-template trackers with either stay refused).  Per step and group: the trackers whose options name the
        same ``lookup`` object and frame name share ONE staged sensor image (``sensor_uploads``); behind the frame call
        and the points call comes ONE pxt_occlusion_mask_views call for every tracker that takes a mask
        (``occlusion_view_calls``), behind the batched LM launch ONE pxt_depth_refine call with the problems of all that
        asked (``depth_refine_calls``); history keys, point gate and policy are each tracker's own, as solo.  Not with
        ``mutual_occlusion`` (which refuses "template" trackers): the sensor's plane already contains the other objects,
        so the two kinds of occluder plane never meet.
        ``uncertainty``: None keeps each tracker's own setting, True / False sets it for all of them (the ``uncertainty``
        option of PixLocPoseTrackerR9): the information problems of a group's step then go out as ONE pxt_lm_information
        launch behind its batched LM launch and its queued renders.
        ``point_report``: None keeps each tracker's own setting; False / "off", "summary" or "full" sets it for all of
        them (the ``point_report`` option of PixLocPoseTrackerR9): the report problems of a group's step then go out as
        ONE pxt_lm_point_report launch, next to the information launch.
        ``n_groups`` > 1: the trackers are dealt to that many groups, each with its own stream, batched UNet pass and
        batched LM launch per step; the groups' UNet passes take turns (an event token), so that one group's MFMA-bound
        UNet pass runs beside the other group's latency-bound renders instead of beside its UNet pass."""
        if not trackers:
            raise ValueError("MultiObjectTracker needs at least one tracker")
        if point_report is not None:
            point_report = parse_mode(point_report)  # (ValueError before anything is touched)
        self.trackers: List[PixLocPoseTrackerR9] = list(trackers)
        self.device = self.trackers[0].device
        for tr in self.trackers:
            if tr.device != self.device:
                raise _lib.PxtError("lock-step trackers share one device")
            # the step below is PixLocPoseTrackerR9.refine() in pieces: a tracker with its own refine() (the YCB policy:
            # ground-truth-gated updates, pixloc_tracker_ycb.py:241-295) would silently run r9's policy here
            if type(tr).refine is not PixLocPoseTrackerR9.refine or type(tr)._frame_policy is not PixLocPoseTrackerR9._frame_policy:
                raise _lib.PxtError(f"{type(tr).__name__} overrides refine(): lock-step tracking implements PixLocPoseTrackerR9's policy only")
            points = getattr(tr, "reference_points", "sfm")
            if points == "template":
                # (phase A extracts the points of a group's "template" trackers in one call, from the planes of their
                # mesh templates' one frame call)
                from ..mesh_template import MeshTemplate

                if not isinstance(getattr(tr, "template", None), MeshTemplate):
                    raise ValueError("reference_points='template' in lock-step tracking needs a tracker with a mesh template")
                if mutual_occlusion is not None:
                    raise ValueError("mutual_occlusion is not combined with a reference_points='template' tracker yet (the "
                                     "scene call does not hand out the depth planes)")
            elif points != "sfm":
                # (the batched render chain carries no float Depth image and the batched reference pass encodes the SfM window)
                raise ValueError(f"reference_points={points!r} is not supported by lock-step tracking yet")
            # the sensor options ride on the float depth planes of the mesh frame call and on its points: a mesh template
            # with reference_points="template" (the batched NeRF render chain carries no float Depth image)
            if getattr(tr, "depth_refine", None) is not None and points != "template":
                raise ValueError("depth_refine is supported by lock-step tracking for mesh-template trackers with "
                                 "reference_points='template' only")
            if getattr(tr, "occlusion", None) is not None and points != "template":
                raise ValueError("occlusion is supported by lock-step tracking for mesh-template trackers with "
                                 "reference_points='template' only")
            template = getattr(tr, "template", None)
            if template is not None:
                from ..mesh_template import MeshTemplate

                # (phase A draws the frames of a group's mesh templates in one MeshTemplate.frames call)
                if not isinstance(template, MeshTemplate):
                    raise ValueError("lock-step tracking takes a mesh template that is a mesh_template.MeshTemplate "
                                     f"(got {template!r})")
        self.mutual_occlusion = mutual_occlusion
        self._scene_of: List = [None] * len(self.trackers)
        if mutual_occlusion is not None:
            self._scene_of = self._checked_scenes(mutual_occlusion)  # (ValueError before anything is touched)
        # one UNet context runs every image of a group's step: the trackers must hold the same checkpoint in the same
        # precision (pixloc_megadepth is one network for all objects; reference pixloc_pose_refiners.py:49-60; the
        # signature names the precision)
        sig = getattr(self.trackers[0].localizer.extractor.model, "weights_signature", None)
        for tr in self.trackers[1:]:
            if getattr(tr.localizer.extractor.model, "weights_signature", None) != sig:
                raise _lib.PxtError("lock-step trackers must share one UNet checkpoint and unet_precision")
        if uncertainty is not None:
            for tr in self.trackers:
                tr.uncertainty = tr.localizer.refiner.information = bool(uncertainty)
        if point_report is not None:
            for tr in self.trackers:
                tr.point_report = tr.localizer.refiner.point_report = point_report
        for k, s in enumerate(self._scene_of):
            if s is not None:
                self.trackers[k].enable_mutual_occlusion()  # (its frames may now come with an occluder plane)
        self.groups: List[_Group] = []
        # a group's queued renders as ONE chain of launches carrying the rays of all its objects (pxt_ngp_render_frame_batch;
        # bit for bit the single renders); PXT_BATCH_RENDERS=0: one chain per object, one after the other
        self.batch_renders = (os.environ.get("PXT_BATCH_RENDERS", "1") != "0") if batch_renders is None else bool(batch_renders)
        self.set_groups(n_groups)
        self.lm_workgroups = int(lm_workgroups)      # grid per problem of the batched launch; 0: the library's default
        self.per_image_plan = bool(per_image_plan)   # UNet layers planned as for one image (bit-identity with solo runs)
        self.max_unet_batch = int(max_unet_batch)
        self.steps = 0
        self.solo_frames = 0       # frames that ran through run_single_frame (cold starts, several references)
        self.lockstep_frames = 0
        self.mesh_prime_calls = 0  # MeshTemplate.frames calls made at the head of a step (one per group that needs one)
        self.mesh_ahead_calls = 0  # MeshTemplate.frames_ahead calls queued behind a step's LM launch (one per group)
        self.points_calls = 0      # pxt_points_from_depth_views calls made for "template" trackers (one per group and step)
        self.occlusion_view_calls = 0  # pxt_occlusion_mask_views calls (one per group and step once masks exist)
        self.depth_refine_calls = 0    # pxt_depth_refine calls behind a step's LM launch (one per group and step)
        self.sensor_uploads = 0        # sensor images staged for lock-step frames (one per (lookup, frame name) and step)
        self.timing = None         # set to {} to collect HIP-event pairs per phase (bench.py's untimed diagnostic pass)

    def _checked_scenes(self, option: MutualOcclusion) -> list:
        """The option's scene of every tracker, checked (ValueError); nothing is touched."""
        from ..mesh_render import BATCH_MAX_MESHES, SCENE_MAX_GROW
        from ..mesh_template import MeshTemplate

        scenes = list(option.scenes)
        if len(scenes) != len(self.trackers):
            raise ValueError(f"mutual_occlusion.scenes names one scene (or None) per tracker ({len(self.trackers)}; got "
                             f"{len(scenes)})")
        if int(option.r_grow) != option.r_grow or not (0 <= int(option.r_grow) <= SCENE_MAX_GROW):
            raise ValueError(f"mutual_occlusion.r_grow is an integer in 0..{SCENE_MAX_GROW} (got {option.r_grow})")
        members: dict = {}
        for k, s in enumerate(scenes):
            if s is not None:
                members.setdefault(s, []).append(k)
        for s, ks in members.items():
            for k in ks:
                if not isinstance(getattr(self.trackers[k], "template", None), MeshTemplate):
                    raise ValueError(f"mutual occlusion: tracker {k} of scene {s!r} has no mesh template; a scene's trackers "
                                     "are all mesh-template trackers (NeRF-template trackers are not part of a scene yet)")
            if len(ks) > BATCH_MAX_MESHES:
                raise ValueError(f"mutual occlusion: scene {s!r} has {len(ks)} trackers; a scene is drawn in one call of "
                                 f"at most {BATCH_MAX_MESHES} meshes")
            self._check_scene_cameras(s, ks)
        return scenes

    def _check_scene_cameras(self, scene, ks) -> None:
        """The trackers ``ks`` of ``scene`` that have a camera (it comes with a tracker's first frame) see one image."""
        cams = [(k, self.trackers[k].camera) for k in ks if getattr(self.trackers[k], "camera", None) is not None]
        for k, cam in cams[1:]:
            if not _same_scene_camera(cams[0][1], cam):
                raise ValueError(f"mutual occlusion: trackers {cams[0][0]} and {k} of scene {scene!r} have different query "
                                 "cameras (size, f, c; no lens terms): a scene is one image")
        if len(cams) == 1 and not _same_scene_camera(cams[0][1], cams[0][1]):
            raise ValueError(f"mutual occlusion: tracker {cams[0][0]} of scene {scene!r} has a query camera with lens terms")

    def _check_scene_groups(self) -> None:
        """Every scene's trackers sit in one group: a scene is drawn in one call on one stream."""
        group_of = {k: g.index for g in self.groups for k in g.members}
        seen: dict = {}
        for k, s in enumerate(self._scene_of):
            if s is not None and seen.setdefault(s, group_of[k]) != group_of[k]:
                raise ValueError(f"mutual occlusion: the trackers of scene {s!r} have been placed in different groups "
                                 f"({seen[s]} and {group_of[k]}); a scene stays in one group")

    def set_groups(self, n_groups: int) -> None:
        """(Re)deals the trackers to ``n_groups`` groups, tracker k to group k mod n_groups - with ``mutual_occlusion`` a
        scene stays together: its trackers follow its first one (ValueError if a group would then hold more trackers
        than one batched LM launch takes).  Synchronises the device: a tracker's tensors of the last step were produced
        on its old group's stream."""
        n_groups = max(1, min(int(n_groups), len(self.trackers)))
        if any(g.pend for g in self.groups):
            raise _lib.PxtError("set_groups between steps only")
        torch.cuda.synchronize(self.device)
        dealt = [k % n_groups for k in range(len(self.trackers))]
        first: dict = {}
        for k, s in enumerate(self._scene_of):
            if s is not None:
                dealt[k] = first.setdefault(s, dealt[k])
        if first and max(dealt.count(g) for g in range(n_groups)) > _lib.PXT_LM_MAX_BATCH:
            raise ValueError(f"mutual occlusion: keeping every scene in one of {n_groups} groups puts more than "
                             f"{_lib.PXT_LM_MAX_BATCH} trackers into a group")
        self.groups = []
        for g in range(n_groups):
            members = [k for k in range(len(self.trackers)) if dealt[k] == g]
            if not members:  # (scenes kept together may leave a group empty)
                continue
            stream = None if n_groups == 1 else _group_stream(self.device, g)
            self.groups.append(_Group(g, members, stream, self.trackers[members[0]].localizer.extractor.model))
        self.model = self.groups[0].model
        self._last_unet_done = None
        self._check_scene_groups()

    # ------------------------------------------------------------------ helpers
    def _lm_batch_ws(self, grp: _Group) -> torch.Tensor:
        if grp.batch_ws is None:
            need = int(_lib.lib().pxt_lm_batch_workspace_bytes(_lib.PXT_LM_MAX_BATCH))
            grp.batch_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return grp.batch_ws

    def _mark(self, name: str):
        if self.timing is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.timing.setdefault(name, []).append(e)
        return e

    def _unet_batch(self, grp: _Group, jobs) -> None:
        """jobs: [(extractor, image, scale, mask, normalize)] -> every pyramid computed in batched passes (images of
        one size per pass, at most max_unet_batch each) and handed to its extractor through preload()."""
        prepared = []
        for ex, image, scale, mask, normalize in jobs:
            img, rest_mask, scales = ex.prepared(image, scale, mask)
            prepared.append((img, rest_mask, scales))
        sizes = {}
        for i, (img, _m, _s) in enumerate(prepared):
            sizes.setdefault((int(img.shape[0]), int(img.shape[1])), []).append(i)
        cur = torch.cuda.current_stream(self.device)
        if len(self.groups) > 1 and self._last_unet_done is not None:
            cur.wait_event(self._last_unet_done)  # the groups' UNet passes take turns
        grp.model.set_batch_plan(self.per_image_plan)
        try:
            for idx in sizes.values():
                for a in range(0, len(idx), self.max_unet_batch):
                    part = idx[a:a + self.max_unet_batch]
                    outs = grp.model.forward_packed_batch([(prepared[i][0], prepared[i][1], jobs[i][4]) for i in part])
                    for i, maps in zip(part, outs):
                        ex, image, scale, mask, normalize = jobs[i]
                        ex.preload(image, scale, mask, normalize, maps, prepared[i][2])
        finally:
            grp.model.set_batch_plan(False)
        if len(self.groups) > 1:
            grp.unet_done = torch.cuda.Event()
            grp.unet_done.record(cur)
            self._last_unet_done = grp.unet_done

    # ------------------------------------------------------------------ one step = one frame of every object
    def run_single_frames(self, frames) -> List[bool]:
        """frames[k] = (path, image) of tracker k (None: that tracker sits this step out).  The lock-step counterpart
        of PoseTracker.run_single_frame (reference base_pose_tracker.py:24-30) for K trackers at once."""
        assert len(frames) == len(self.trackers)
        out: List[Optional[bool]] = [None] * len(frames)
        self._mark("step_begin")
        for grp in self.groups:
            if grp.stream is None:
                self._enqueue(grp, frames, out)
            else:
                with torch.cuda.stream(grp.stream):
                    self._enqueue(grp, frames, out)
        for grp in self.groups:
            if grp.stream is None:
                self._finish(grp, frames, out)
            else:
                with torch.cuda.stream(grp.stream):
                    self._finish(grp, frames, out)
        self._mark("step_end")
        self.steps += 1
        return out

    def _enqueue(self, grp: _Group, frames, out) -> None:
        live = []
        grp.pend = []
        # ---- phase A: per-object frame set-up (policy head, mask + reference render or the render queued last step)
        self._stage_sensors(grp, frames)  # (the sensor options: before the step's first launch)
        self._prime_mesh_frames(grp, frames)
        for k in grp.members:
            tr, frame = self.trackers[k], frames[k]
            if frame is None:
                continue
            if not self._takes_lockstep(tr, frame):
                tr.run_single_frame(frame)
                out[k] = bool(tr.success)
                self.solo_frames += 1
                continue
            tr._frame_setup(frame, lockstep=True)
            if self.mutual_occlusion is not None and tr.template is not None:
                # (a step's scenes are formed from who takes the lock-step path in THAT step: not drawn ahead)
                tr.localizer.refiner.after_lm_enqueued = None
            ref_u8 = tr.get_reference_image(tr.pose, keep=True)  # (get_dynamic_id asks again: the same tensor object)
            live.append((k, tr, frame, ref_u8))
        self._mark("renders_enqueued")
        if not live:
            return
        # ---- phase B: the step's 2 K images through the UNet in batched passes
        jobs = []
        for k, tr, (path, image), ref_u8 in live:
            ex = tr.localizer.refiner.feature_extractor
            # extract_reference_features encodes the window of the render its points depend on (refiner.reference_window)
            # - but a reference render of the query's own size goes through the UNet with everybody else's: a window
            # would take it out of the batch (one 14-image pass became a 13-image pass + two small ones: 4.5 -> 5.3 ms)
            refiner = tr.localizer.refiner
            if refiner.render_points:  # ("template": the points are not the SfM table's - the whole image, as solo)
                ref_in = ref_u8
            else:
                if tuple(ref_u8.shape[:2]) == tuple(image.shape[:2]):
                    refiner._window_memo = (ref_u8, tr.pose, ref_u8, None)
                ref_in, _win = refiner.reference_window(tr.reference_ids, tr.pose, ref_u8)
            jobs.append((ex, ref_in, 1, None, False))                               # extract_reference_features
            jobs.append((ex, image, 1, tr.localizer.refiner.query_mask, True))      # refine_query_pose's query pass
        self._unet_batch(grp, jobs)
        self._mark("unet_enqueued")
        # ---- phase C: per object, the reference's bookkeeping + sparse sampling + the LM problem
        pend = []
        for k, tr, (path, image), ref_u8 in live:
            refiner = tr.localizer.refiner
            tr.dynamic_id = tr.get_dynamic_id(tr.pose)
            ref_id = tr.reference_ids[0]
            pose_init = tr._frame_pose_init()
            dbg = DebugTracker(refiner, tr.debug)
            status, x = refiner.begin_refine(path, tr.camera, pose_init, [ref_id], image, tr.dynamic_id)
            refiner.feature_extractor.unstage()  # (drops a preloaded pyramid nobody asked for)
            pend.append((k, tr, path, ref_id, dbg, status, x))
        self._mark("sampling_enqueued")
        # ---- phase D: ONE persistent launch for every refinement, then each object's next render behind it
        probs = [x for (_k, _tr, _p, _r, _d, status, x) in pend if status == "lm"]
        handles = []
        if probs:
            conf = probs[0]["conf"]
            for pr in probs[1:]:
                if bytes(pr["conf"]) != bytes(conf):
                    raise _lib.PxtError("lock-step trackers must share the optimizer configuration")
            conf.n_workgroups = self.lm_workgroups
            if len(self.groups) > 1:
                # the groups' launches may run side by side: together they must fit the device's resident workgroups
                # (one 8-wave workgroup per CU: pxt_lm.hip), or both would sit partly resident and time out - also when the
                # caller asked for a grid per problem (lm_workgroups > 0: clamped to the groups' share)
                share = max(8, _device_cus() // (len(self.groups) * len(probs)) // 8 * 8)
                conf.n_workgroups = share if conf.n_workgroups <= 0 else min(conf.n_workgroups, share)
            handles = PixTrackOptimizer.refine_levels_batch(probs, conf, self._lm_batch_ws(grp), pool_key=grp.index)
        self._mark("lm_enqueued")
        it = iter(handles)
        grp.pend = [(k, tr, path, ref_id, dbg, status, x, next(it) if status == "lm" else None)
                    for (k, tr, path, ref_id, dbg, status, x) in pend]
        batched = self._batched_renders_ahead(grp) if self.batch_renders else set()
        batched |= self._mesh_frames_ahead(grp)
        for k, tr, path, ref_id, dbg, status, x, handle in grp.pend:
            hook = getattr(tr.localizer.refiner, "after_lm_enqueued", None)
            if handle is not None and hook is not None and k not in batched:
                hook(handle)
        self._mark("ahead_enqueued")
        # ---- the step's pose information (opt-in): ONE launch for every object that asked, behind the renders
        asked = [(x, handle, tr.localizer.refiner) for (_k, tr, _p, _r, _d, status, x, handle) in grp.pend
                 if status == "lm" and tr.localizer.refiner.information]
        if asked:
            if grp.info_ws is None:
                need = int(_lib.lib().pxt_lm_information_workspace_bytes(_lib.PXT_LM_MAX_BATCH))
                grp.info_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
            info = PixTrackOptimizer.information_levels([rf.information_item(x, h) for x, h, rf in asked], asked[0][0]["conf"],
                                                        grp.info_ws, pool_key=("group", grp.index))
            for i, (x, _h, _rf) in enumerate(asked):
                x["info"] = (info, i)
        # ---- the step's point reports (opt-in): ONE launch for every object that asked, next to the information launch
        asked = [(x, handle, tr.localizer.refiner) for (_k, tr, _p, _r, _d, status, x, handle) in grp.pend
                 if status == "lm" and tr.localizer.refiner.point_report]
        if asked:
            if grp.report_ws is None:
                need = int(_lib.lib().pxt_lm_point_report_workspace_bytes(_lib.PXT_LM_MAX_BATCH))
                grp.report_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
            report = PixTrackOptimizer.point_report_levels([rf.point_report_item(x, h) for x, h, rf in asked],
                                                           asked[0][0]["conf"], grp.report_ws, pool_key=("group", grp.index))
            for i, (x, _h, _rf) in enumerate(asked):
                x["report"] = (report, i)
        # ---- the step's sensor-depth refinements (opt-in): ONE launch for every object that asked, next to them
        self._enqueue_depth_refinements(grp)

    @staticmethod
    def _takes_lockstep(tr, frame) -> bool:
        """This step, the tracker's frame goes through the merged device work (else: through run_single_frame)."""
        if frame is None:
            return False
        scales = tr.steady_multiscale if tr.success else tr.localizer.refiner.conf.multiscale
        return not (tr.cold_start or len(tr.reference_ids) != 1 or list(scales or [1]) != [1])

    def _prime_mesh_frames(self, grp: _Group, frames) -> None:
        """The frames of the group's mesh-template trackers that take the lock-step path, at their poses, in ONE
        MeshTemplate.frames call on the group's stream; each tracker's _mask_and_reference then takes its planes instead
        of making its own call.  (A tracker that renders no mask this frame - the frame after a failed one - still needs
        its reference image: it rides along with the same requests and drops its depth_nz plane.)"""
        part = [self.trackers[k] for k in grp.members
                if self.trackers[k].template is not None and self._takes_lockstep(self.trackers[k], frames[k])]
        # a tracker whose frame was drawn ahead, behind the last step's LM launch, and verified for its pose keeps that
        # frame (its get_mask takes it); with "template" points its plane still joins the step's one points call
        ahead = [(tr, tr.verified_ahead()) for tr in part]
        part = [tr for tr, ok in ahead if ok is None]
        ahead = [(tr, ok) for tr, ok in ahead if ok is not None]
        ahead_points = [(tr, ok.depth, ok.view) for tr, ok in ahead if tr.reference_points == "template" and ok.depth is not None]
        # the occlusion option's pass for the trackers that take a mask this step: their planes, with the plain masks
        ahead_occ = [(tr, ok.mask, ok.depth, ok.view) for tr, ok in ahead if self._takes_occlusion(tr) and ok.depth is not None]
        if not part:  # (NeRF trackers only: nothing of the mesh path is touched; or every mesh frame was drawn ahead)
            if ahead_points:
                self._prime_template_points(grp, ahead_points)
            self._prime_occlusion(grp, ahead_occ)
            return
        self.mesh_prime_calls += 1
        from ..mesh_render import FrameBatchWorkspace
        from ..mesh_template import MeshTemplate

        if grp.mesh_ws is None:
            grp.mesh_ws = FrameBatchWorkspace()
        scenes = self._step_scenes(grp, frames) if self.mutual_occlusion is not None else None
        views = ([tr.template for tr in part], [tr.pose for tr in part], [tr.camera for tr in part],
                 [tr._reference_camera() for tr in part])
        want_depth = [tr.reference_points == "template" for tr in part]
        if any(want_depth):  # (never with mutual_occlusion: refused at construction)
            planes = MeshTemplate.frames(*views, workspace=grp.mesh_ws, want_depth=want_depth)
            for tr, (nz, ref_u8, _depth, _view) in zip(part, planes):
                tr.prime(tr.pose, depth_nz=nz, ref_u8=ref_u8)
            self._prime_template_points(grp, ahead_points + [(tr, depth, view) for tr, (_nz, _ref, depth, view)
                                                             in zip(part, planes) if depth is not None])
            self._prime_occlusion(grp, ahead_occ + [(tr, tr._mask_of(nz), depth, view) for tr, (nz, _ref, depth, view)
                                                    in zip(part, planes) if depth is not None and self._takes_occlusion(tr)])
            return
        if ahead_points:
            self._prime_template_points(grp, ahead_points)
        if scenes is None:  # (also: no scene has two members in this step - the call is the one made without the option)
            for tr, (nz, ref_u8) in zip(part, MeshTemplate.frames(*views, workspace=grp.mesh_ws)):
                tr.prime(tr.pose, depth_nz=nz, ref_u8=ref_u8)
            return
        planes = MeshTemplate.frames(*views, workspace=grp.mesh_ws, scenes=scenes, r_grow=int(self.mutual_occlusion.r_grow),
                                     records=True)
        for tr, (nz, ref_u8, occluder, record) in zip(part, planes):
            tr.prime(tr.pose, depth_nz=nz, ref_u8=ref_u8, mutual=None if occluder is None else (occluder, record))

    def _mesh_frames_ahead(self, grp: _Group) -> set:
        """The next frames of the group's mesh trackers whose hook is the mesh render-ahead, behind the batched LM launch
        in ONE MeshTemplate.frames_ahead call on the group's stream and workspace (more than 16 meshes or 32 views: in
        consecutive calls); every view takes its pose on the device from its tracker's LM record.  Returns the members
        served."""
        items = []
        for k, tr, path, ref_id, dbg, status, x, handle in grp.pend:
            if handle is not None and tr.armed_ahead() == "mesh":
                items.append((k, tr, handle, *tr._render_ahead_mesh_request()))
        if not items:
            return set()
        from ..mesh_render import W_VIEW_DONE, FrameBatchWorkspace
        from ..mesh_template import MeshTemplate

        if grp.mesh_ws is None:
            grp.mesh_ws = FrameBatchWorkspace()
        n_views = sum(len(requests) for _k, _tr, _h, requests, _d, _keys in items)
        rows = grp.ahead_rows.next(n_views)
        rows[:, W_VIEW_DONE] = 0.0
        planes = MeshTemplate.frames_ahead([tr.template for _k, tr, *_ in items], [h.buf for _k, _tr, h, *_ in items],
                                           [tr.camera for _k, tr, *_ in items], [tr._reference_camera() for _k, tr, *_ in items],
                                           grp.mesh_ws, rows, want_depth=[d for *_, d, _keys in items],
                                           requests=[requests for _k, _tr, _h, requests, _d, _keys in items])
        self.mesh_ahead_calls += 1
        first = 0
        for (k, tr, _h, requests, _d, keys), out in zip(items, planes):
            tr._render_ahead_mesh_accept(rows[first:first + len(requests)], keys, *out)
            first += len(requests)
        return {k for k, *_ in items}

    def _prime_template_points(self, grp: _Group, items) -> None:
        """``items`` = [(tracker, depth plane, view record)] of the group's "template" trackers in this step: their
        points in ONE pxt_points_from_depth_views call behind the frame call (one per distinct (n_max, erode, min_alpha),
        normally one; more than 16 views in chunks); each tracker keeps its (pose, p3d, slot_valid, record), which its
        get_dynamic_id consumes in phase C instead of extracting again."""
        def settings(item):
            conf = item[0].localizer.refiner.conf
            return int(conf.reference_points_max), int(conf.reference_points_erode), float(conf.reference_points_min_alpha)

        L, C = _lib.lib(), _lib.C
        for (n_max, erode, min_alpha), chunk in _chunks_by(items, settings, _lib.PXT_POINTS_MAX_VIEWS):
            n = len(chunk)
            sizes = [x for _tr, depth, _v in chunk for x in (int(depth.shape[1]), int(depth.shape[0]))]
            need = int(L.pxt_points_from_depth_views_workspace_bytes(n, (C.c_int32 * (2 * n))(*sizes)))
            if need <= 0:
                raise _lib.PxtError(f"depth planes of {sizes} are not supported by pxt_points_from_depth_views")
            # (one workspace serves one call at a time: the group's calls follow each other on its stream)
            if grp.points_ws is None or grp.points_ws.numel() < need:
                grp.points_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            record = grp.points_records.next(n)  # (read in the step's _frame_policy)
            p3d = torch.empty(n, n_max, 3, dtype=torch.float32, device=self.device)
            slot_valid = torch.empty(n, n_max, dtype=torch.uint8, device=self.device)
            ops.points_from_depth_views([depth for _tr, depth, _v in chunk],
                                        [float(x) for _tr, _d, view in chunk for x in view.reshape(-1)], min_alpha, erode,
                                        n_max, p3d, slot_valid, record, grp.points_ws)
            self.points_calls += 1
            for i, (tr, _depth, _view) in enumerate(chunk):
                tr.prime(tr.pose, points=(p3d[i], slot_valid[i], record[i]))

    @staticmethod
    def _takes_occlusion(tr) -> bool:
        """This step, the tracker's _frame_setup asks for a mask (a tracked frame) and the occlusion option has a
        sensor image to hold against it."""
        return bool(tr.occlusion is not None and tr._depth_sensor is not None and tr.success and not tr._lost)

    def _stage_sensors(self, grp: _Group, frames) -> None:
        """Before the step's first launch: the sensor image of every tracker of the group that takes the lock-step path
        with ``depth_refine`` or ``occlusion``.  Trackers whose options name the same ``lookup`` object and the same
        frame name share ONE staged image - the K objects of one RGB-D frame: one fetch, one upload
        (``sensor_uploads`` counts images).  A tracker that runs the step alone stages its own (run_single_frame)."""
        staged = {}
        for k in grp.members:
            tr, frame = self.trackers[k], frames[k]
            if not self._takes_lockstep(tr, frame):
                continue
            option = tr.depth_refine if tr.depth_refine is not None else tr.occlusion  # (one lookup: _check_occlusion)
            if option is None:
                continue
            name = os.path.basename(str(frame[0]))
            key = (id(option.lookup), name)
            if key not in staged:
                sensor = option.lookup(name)
                if sensor is not None:
                    slot = sum(v is not None for v in staged.values())
                    if slot == len(grp.sensor_slots):
                        grp.sensor_slots.append(SensorStage(self.device))
                    sensor = grp.sensor_slots[slot].upload(sensor, frame[0])
                    self.sensor_uploads += 1
                staged[key] = sensor
            tr._adopt_depth_sensor(frame[0], staged[key])

    def _prime_occlusion(self, grp: _Group, items) -> None:
        """``items`` = [(tracker, plain mask, depth plane, view record)] of the group's trackers whose occlusion pass
        runs this step: ONE pxt_occlusion_mask_views call behind the frame call and the points call (one per distinct
        (min_alpha, r_open, r_grow), normally one; more than 16 views in chunks).  Each tracker keeps (pose, plain mask,
        the pass's frame) - its get_mask takes them instead of making its own call, and its point gate, history keys
        and ``last_occlusion`` are the solo tracker's."""
        if not items:
            return
        from .. import occlusion as OC

        def settings(item):
            conf = item[0]._occ_conf
            return float(conf.min_alpha), int(conf.r_open), int(conf.r_grow)

        L, C = _lib.lib(), _lib.C
        for (min_alpha, r_open, r_grow), chunk in _chunks_by(items, settings, OC.MAX_VIEWS):
            n = len(chunk)
            per_view = [tr._occlusion_view(depth, view) for tr, _m, depth, view in chunk]
            sizes = [x for _tr, _m, depth, _v in chunk for x in (int(depth.shape[1]), int(depth.shape[0]))]
            need = int(L.pxt_occlusion_mask_views_workspace_bytes(n, (C.c_int32 * (2 * n))(*sizes)))
            if need <= 0:
                raise _lib.PxtError(f"depth planes of {sizes} are not supported by pxt_occlusion_mask_views")
            # (one workspace serves one call at a time: the group's calls follow each other on its stream)
            if grp.occ_ws is None or grp.occ_ws.numel() < need:
                grp.occ_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            records = grp.occ_records.next(n)  # (read in the step's _frame_policy)
            out = OC.occlusion_mask_views([depth for _tr, _m, depth, _v in chunk], [s for s, _q in per_view],
                                          [m for _tr, m, _d, _v in chunk], [(0, 0)] * n, min_alpha,
                                          [q for _s, q in per_view], r_open, r_grow, records=records,
                                          workspace=grp.occ_ws)
            self.occlusion_view_calls += 1
            cur = torch.cuda.current_stream(self.device)
            for i, (tr, mask_in, depth, view) in enumerate(chunk):
                sensor, quanta = per_view[i]
                frame = OC.pass_frame(depth, sensor, mask_in, out["masks"][i], out["occluders"][i], (0, 0), min_alpha,
                                      quanta, (r_open, r_grow), records[i], tr._occ_done, view)
                tr._occ_done.record(cur)
                tr.prime(tr.pose, occlusion=frame)

    def _enqueue_depth_refinements(self, grp: _Group) -> None:
        """Behind the step's batched LM launch: ONE pxt_depth_refine call with the problems of all the group's trackers
        that asked (one per distinct conf; more than the call's maximum in chunks).  Each problem reads its own LM record
        on the device; each tracker's _frame_policy reads its own record."""
        from ..depth_refinement import MAX_PROBLEMS, depth_refine_batch

        asked = []
        for _k, tr, _p, _r, _d, status, x, handle in grp.pend:
            if status != "lm" or tr.depth_refine is None:
                continue
            item = tr._depth_problem(x, handle, tr.camera)
            if item is not None:  # (None: the frame has no depth image - its pose stays the LM's)
                asked.append((tr._depth_conf, x, item))
        for conf, chunk in _chunks_by(asked, lambda a: a[0], MAX_PROBLEMS):
            if grp.depth_ws is None:
                grp.depth_ws = torch.zeros(int(_lib.lib().pxt_depth_refine_workspace_bytes(MAX_PROBLEMS)),
                                           dtype=torch.uint8, device=self.device)
            pending = depth_refine_batch([item[0] for _c, _x, item in chunk], conf, workspace=grp.depth_ws,
                                         records=[item[1] for _c, _x, item in chunk])
            self.depth_refine_calls += 1
            for i, (_c, x, _item) in enumerate(chunk):
                x["depth"] = _OneDepth(pending, i)

    def _step_scenes(self, grp: _Group, frames):
        """The scene of each of the group's mesh trackers that take the lock-step path this step (the order of
        _prime_mesh_frames' ``part``), None where the tracker is alone: a scene counts only with two members in the
        step.  None: no scene is drawn this step."""
        ks = [k for k in grp.members
              if self.trackers[k].template is not None and self._takes_lockstep(self.trackers[k], frames[k])]
        ids = [self._scene_of[k] for k in ks]
        scenes = [s if s is not None and ids.count(s) >= 2 else None for s in ids]
        if all(s is None for s in scenes):
            return None
        for s in {s for s in scenes if s is not None}:
            self._check_scene_cameras(s, [k for k, t in zip(ks, scenes) if t == s])
        index = {s: i for i, s in enumerate(dict.fromkeys(s for s in scenes if s is not None))}
        return [None if s is None else index[s] for s in scenes]

    def _batched_renders_ahead(self, grp: _Group) -> set:
        """The group's queued renders (behind the batched LM launch, cameras from its epilogue's slots) in one batched
        chain per (spp) - returns the members served; the others take their own _render_ahead()."""
        from ..ngp import Testbed

        by_spp = {}
        for k, tr, path, ref_id, dbg, status, x, handle in grp.pend:
            if handle is None or tr.armed_ahead() != "nerf":
                continue
            req = tr._render_ahead_request()
            if req is not None:
                by_spp.setdefault(req[2], []).append((k, tr, req))
        served = set()
        for spp, items in by_spp.items():
            if len(items) < 2:
                continue
            if grp.render_ws is None:
                grp.render_ws = torch.empty(Testbed.batch_workspace_bytes(_lib.PXT_NGP_MAX_BATCH), dtype=torch.uint8,
                                            device=self.device)
            for a in range(0, len(items), _lib.PXT_NGP_MAX_BATCH):
                part = items[a:a + _lib.PXT_NGP_MAX_BATCH]
                outs = Testbed.render_frame_batch_device([tr.testbed for _k, tr, _r in part], [(r[0], r[1]) for _k, _t, r in part],
                                                         spp, mode=2, from_slot=True, workspace=grp.render_ws)
                for (k, tr, _r), out in zip(part, outs):
                    tr._render_ahead_accept(out)
                    served.add(k)
        return served

    def _finish(self, grp: _Group, frames, out) -> None:
        # ---- phase E: results, per-object policy (cost gate, pose update, history), the loop's tail
        for k, tr, path, ref_id, dbg, status, x, handle in grp.pend or []:
            refiner = tr.localizer.refiner
            ret = refiner.finish_refine(x, handle.result()) if handle is not None else x
            if handle is not None and x.get("depth") is not None:
                ret["depth_pending"] = x["depth"]  # (read, and waited for, by the tracker's _frame_policy)
            ok = tr._frame_policy(path, {ref_id: ret}, {ref_id: tr._frame_cost()}, {ref_id: dbg})
            if not ok:
                tr.relocalize(frames[k])
            tr.update_reference_ids()
            out[k] = bool(ok)
            self.lockstep_frames += 1
        grp.pend = None

    def run(self, frame_iterators, max_frames=float("inf")):
        """Advances every tracker over its own frame iterator (``get_query_frame_iterator`` objects or any iterables of
        (path, image)), one frame of each per step, until all are exhausted."""
        its = [iter(f) for f in frame_iterators]
        n = 0
        while n < max_frames:
            frames = [next(it, None) for it in its]
            if all(f is None for f in frames):
                break
            self.run_single_frames(frames)
            n += 1
        return n


_GROUP_STREAMS = {}


def _group_stream(device, g: int) -> "torch.cuda.Stream":
    """Group g's stream on ``device``: made once per process (HIP deals streams to its hardware queues in creation order:
    fresh streams per tracker would make the groups' overlap depend on how many trackers the process has seen)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), g)
    if key not in _GROUP_STREAMS:
        _GROUP_STREAMS[key] = torch.cuda.Stream(device)
    return _GROUP_STREAMS[key]


def _device_cus() -> int:
    import ctypes as C

    n = C.c_int(0)
    _lib.check(_lib.lib().pxt_device_cus(C.byref(n)), "pxt_device_cus")
    return int(n.value)


def parse_config_sh(path) -> dict:
    """The two settings a reference `config/<object>.sh` exports for the tracker: OBJ_AABB and UPRIGHT_REF_IMG
    (e.g. /root/reference/config/premier_protein.sh:14; read as text, the file is not executed)."""
    import re

    out = {}
    for line in open(path):
        m = re.match(r"\s*(?:export\s+)?(OBJ_AABB|UPRIGHT_REF_IMG)\s*=\s*(.*?)\s*$", line)
        if m:
            out[m.group(1)] = m.group(2).strip().strip("'\"")
    return out


def build_parser():
    import argparse
    from pathlib import Path

    ap = argparse.ArgumentParser()
    ap.add_argument("--object_path", type=Path, nargs="+", required=True)
    ap.add_argument("--query", type=Path, nargs="+", required=True)
    ap.add_argument("--out_dir", type=Path, nargs="+", required=True)
    ap.add_argument("--config", type=Path, nargs="*", default=None, help="config/<object>.sh per object")
    ap.add_argument("--obj_aabb", nargs="*", default=None)
    ap.add_argument("--upright_ref_img", nargs="*", default=None)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--debug", type=int, default=0)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--pixloc_pickles", action="store_true")
    ap.add_argument("--unet_precision", choices=("fp16", "fp32"), default="fp16",
                    help="UNet activations of every object: fp16 (default, fastest) or fp32 (pixloc's precision)")
    ap.add_argument("--uncertainty", action="store_true",
                    help="add the pose information matrix, covariance and observability of every frame to poses.pkl")
    ap.add_argument("--point_report", choices=("off", "summary", "full"), default="off",
                    help="add every frame's valid / inlier point counts and mean robust weight to poses.pkl (summary), and "
                         "the per-point projections, residuals and weights as well (full)")
    ap.add_argument("--template", choices=("nerf", "mesh"), default="nerf",
                    help="what every object's mask and reference image are rendered from: nerf (default) or mesh (--mesh; "
                         "no snapshot, nerf2sfm.pkl or OBJ_AABB is read; a group's frames are drawn in one call)")
    ap.add_argument("--mesh", type=Path, nargs="+", default=None, help="--template mesh: the mesh of each object")
    ap.add_argument("--texture", type=Path, nargs="+", default=None, help="the texture map of each object's mesh")
    ap.add_argument("--mesh_scale", type=float, nargs="+", default=[1.0], help="factor on each mesh's vertices")
    ap.add_argument("--mesh_supersample", type=int, nargs="+", choices=(1, 2, 4), default=[2],
                    help="samples per pixel and axis of each mesh template's reference image (default 2, untuned)")
    ap.add_argument("--mesh_render_ahead", action="store_true",
                    help="--template mesh: draw every object's next frame in one call queued behind the step's LM launch "
                         "(default: off; not with --mutual_occlusion, whose scenes are drawn at the head of a step)")
    ap.add_argument("--reference_sfm", type=Path, nargs="+", default=None,
                    help="each object's SfM model directory (the ref/ directory mesh_dataset wrote)")
    ap.add_argument("--reference_points", choices=("sfm", "template"), default="sfm",
                    help="the points every object's frames are refined on: sfm (default: the SfM points of the nearest "
                         "mapping image) or template (--template mesh: a lattice of the depth plane the mesh template draws "
                         "for the frame; a group's points are extracted in one call)")
    ap.add_argument("--depth_refine", action="store_true",
                    help="--template mesh --reference_points template: refine every object's pose on its sensor depth image "
                         "after the LM; a group's problems go out in one call (needs --sensor_depth_dir and "
                         "--sensor_depth_scale)")
    ap.add_argument("--occlusion_mask", action="store_true",
                    help="--template mesh --reference_points template: take the pixels where the sensor depth image lies in "
                         "front of an object out of its mask and point set; a group's passes go out in one call (needs "
                         "--sensor_depth_dir and --sensor_depth_scale)")
    ap.add_argument("--sensor_depth_dir", type=Path, nargs="+", default=None,
                    help="the 16-bit depth images, one per frame: one directory per object or one for all - objects with "
                         "equal directory, template and substitution share one image upload per step")
    ap.add_argument("--sensor_depth_scale", type=float, nargs="+", default=None, help="SfM units per raw count, per object or one for all")
    ap.add_argument("--sensor_depth_template", nargs="+", default=None,
                    help="file name of a frame's depth image: {stem} / {name} of the frame (default {stem}.png)")
    ap.add_argument("--sensor_depth_sub", nargs=2, metavar=("OLD", "NEW"), default=None,
                    help="replace OLD by NEW in the frame's name first (YCB-Video: color depth)")
    ap.add_argument("--depth_prior", nargs=2, type=float, metavar=("WT", "WR"), default=None,
                    help="diagonal prior on the depth refinement's accumulated update: translation, rotation weight")
    ap.add_argument("--occlusion_delta", type=float, nargs="+", default=None,
                    help="how much closer the sensor's surface must be, as a fraction of the model's extent (default 0.1)")
    ap.add_argument("--occlusion_radii", nargs=2, type=int, metavar=("OPEN", "GROW"), default=None,
                    help="box radii of the opening and the growth of the occluder plane (default 1 3)")
    ap.add_argument("--mutual_occlusion", action="store_true",
                    help="--template mesh: objects whose --query paths are equal share an image; the pixels where another of "
                         "them lies in front leave an object's mask and gate its points")
    ap.add_argument("--mutual_occlusion_grow", type=int, default=2,
                    help="box radius by which the hidden pixels are grown, 0..8 (default 2, untuned)")
    return ap


def _per_object(values, k: int, K: int, flag: str):
    """A list option's entry for object k: one entry per object, or one entry for all (None: not given)."""
    if values is None:
        return None
    if len(values) not in (1, K):
        raise ValueError(f"{flag} takes one entry per object or one entry for all (got {len(values)} for {K} objects)")
    return values[k if len(values) == K else 0]


def sensor_options_from_args(args, k: int, K: int, shared: dict) -> dict:
    """--depth_refine / --occlusion_mask and their companions -> the two options of object k (``{}`` when both are off).
    ``shared``: the lookups made so far, by (directory, template, substitution) - objects that agree in the three get ONE
    lookup object, so that lock-step tracking uploads their frame's image once."""
    import argparse

    from .pixloc_tracker_r9 import depth_option_from_args, occlusion_option_from_args

    if not (getattr(args, "depth_refine", False) or getattr(args, "occlusion_mask", False)):
        return {}
    if args.template != "mesh" or args.reference_points != "template":
        raise ValueError("--depth_refine and --occlusion_mask go with --template mesh --reference_points template")
    directory = _per_object(args.sensor_depth_dir, k, K, "--sensor_depth_dir")
    template = _per_object(args.sensor_depth_template, k, K, "--sensor_depth_template") or "{stem}.png"
    sub = tuple(args.sensor_depth_sub) if args.sensor_depth_sub else None
    key = (None if directory is None else os.path.normpath(str(directory)), template, sub)
    one = argparse.Namespace(depth_refine=args.depth_refine, occlusion_mask=args.occlusion_mask, sensor_depth_dir=directory,
                             sensor_depth_scale=_per_object(args.sensor_depth_scale, k, K, "--sensor_depth_scale"),
                             sensor_depth_template=template, sensor_depth_sub=sub, depth_prior=args.depth_prior,
                             occlusion_delta=_per_object(args.occlusion_delta, k, K, "--occlusion_delta"),
                             occlusion_radii=args.occlusion_radii, _sensor_lookup=shared.get(key))
    out = {"depth_refine": depth_option_from_args(one), "occlusion": occlusion_option_from_args(one)}
    shared[key] = one._sensor_lookup
    return out


def mutual_occlusion_from_args(args) -> Optional[MutualOcclusion]:
    """--mutual_occlusion [--mutual_occlusion_grow R] -> the option (None when off): the objects whose --query paths are
    equal share a scene; an object whose query path is its own is in none."""
    if not getattr(args, "mutual_occlusion", False):
        return None
    if args.template != "mesh":
        raise ValueError("--mutual_occlusion goes with --template mesh")
    paths = [os.path.normpath(str(q)) for q in args.query]
    return MutualOcclusion(scenes=[p if paths.count(p) >= 2 else None for p in paths], r_grow=args.mutual_occlusion_grow)


def main(argv=None):
    """Several objects, one GPU: the reference's tracker command line (pixloc_tracker_r9.py:288-318) once per object, in
    lock-step.  Every list takes one entry per object; an object's OBJ_AABB / UPRIGHT_REF_IMG come from --config (a
    reference config/<object>.sh) or from --obj_aabb / --upright_ref_img.  Outputs per object as r9's CLI writes them:
    <out_dir>/poses.pkl, <out_dir>/trackers.pkl, and the `Cache hits / Done` lines per object."""
    import gc
    import os
    from pathlib import Path

    import numpy as np

    import argparse

    from .pixloc_tracker_r9 import _dump, template_from_args

    ap = build_parser()
    args = ap.parse_args(argv)
    K = len(args.object_path)
    if len(args.query) != K or len(args.out_dir) != K:
        ap.error("--object_path, --query and --out_dir take one entry per object")
    if torch.cuda.is_available():
        from ..parallel import bind_to_device_numa

        bind_to_device_numa(0)
    trackers, lookups = [], {}
    for k in range(K):
        conf = parse_config_sh(args.config[k]) if args.config else {}
        if args.obj_aabb:
            conf["OBJ_AABB"] = args.obj_aabb[k]
        if args.upright_ref_img:
            conf["UPRIGHT_REF_IMG"] = args.upright_ref_img[k]
        needed = ("UPRIGHT_REF_IMG",) if args.template == "mesh" else ("OBJ_AABB", "UPRIGHT_REF_IMG")
        if any(name not in conf for name in needed):
            ap.error(f"object {k}: {' and '.join(needed)} needed (--config, or --obj_aabb / --upright_ref_img)")
        os.environ.update({name: conf[name] for name in needed})  # read in the constructor (:77, :85)
        obj = args.object_path[k]
        os.makedirs(args.out_dir[k], exist_ok=True)
        try:
            one = argparse.Namespace(template=args.template, mesh=_per_object(args.mesh, k, K, "--mesh"),
                                     texture=_per_object(args.texture, k, K, "--texture"),
                                     mesh_scale=_per_object(args.mesh_scale, k, K, "--mesh_scale"),
                                     mesh_supersample=_per_object(args.mesh_supersample, k, K, "--mesh_supersample"),
                                     mesh_render_ahead=args.mesh_render_ahead)
            template = template_from_args(one)
            reference_sfm = _per_object(args.reference_sfm, k, K, "--reference_sfm")
            sensor = sensor_options_from_args(args, k, K, lookups)
        except ValueError as e:
            ap.error(str(e))
        trackers.append(PixLocPoseTrackerR9(template=template, reference_sfm=reference_sfm,
                                            object_path=str(obj), data_path=str(obj / "pixtrack/pixsfm/dataset"),
                                            eval_path=str(args.out_dir[k]), loc_path=str(obj / "pixtrack/aug_nerf_sfm"),
                                            debug=args.debug, unet_precision=args.unet_precision,
                                            uncertainty=args.uncertainty, point_report=args.point_report,
                                            reference_points=args.reference_points, **sensor))
    try:
        mutual = mutual_occlusion_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    multi = MultiObjectTracker(trackers, n_groups=args.groups, mutual_occlusion=mutual)
    its = [tr.get_query_frame_iterator(q, args.frames if args.frames is not None else np.inf)
           for tr, q in zip(trackers, args.query)]
    gc.collect()
    gc.freeze()
    gc.disable()
    try:
        multi.run(its)
    finally:
        gc.enable()
    for tr in trackers:
        tr.save_poses(args.pixloc_pickles)
        print("Cache hits: %d, misses: %d" % (tr.hits, tr.misses))
        _dump(tr.pose_tracker_history, os.path.join(tr.eval_path, "trackers.pkl"), args.pixloc_pickles)
    print("Done")


if __name__ == "__main__":
    main()
