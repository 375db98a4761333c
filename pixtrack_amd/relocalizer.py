"""Relocaliser: a pose for a query frame without a prior, for cold starts and lost tracks.

The reference has no relocaliser (PixLocPoseTrackerR9.relocalize takes the upright mapping view on a cold start and
afterwards only counts).  This one reuses the tracker's own pieces:

* HYPOTHESES: for every mapping view ``rolls`` rotations about the optical axis (R = Rz(theta) R_v,
  t = Rz(theta) t_v; theta = 0 is the db pose), optionally a ``shifts x shifts`` grid of lateral translations that moves
  the object centre across the image at the view's depth, plus (per call) the last accepted pose with its nearest
  entry of the bank.
* a VIEW BANK, built once: the reference rendered at every (view, roll) pose with the reference camera, one UNet pass
  each, the view's points sampled at all three levels through ``extract_reference_features``.  The features are
  rendered per roll because the UNet's descriptors are not invariant to an in-plane rotation of the image: the same
  point seen upright and rolled by 90 degrees has different descriptors (measured: refining a rolled query against the
  upright view's features converges in 21-29 % of the trials, against the nearest entry's in 83-96 %).  The stride-16 records
  of all entries form one flat point bank for scoring; each entry keeps its ``SparseReferenceFeatures`` for the LM.
* per ``localize``: one unmasked UNet pass over the query, ONE ``score_pose_hypotheses`` launch on the ``score_level``
  map, a ranking on the device, and the top-K candidates refined in ONE batched LM launch (levels 2, 1, 0, each with
  its own view's features).  Two host reads: the top-K indices, then the K results.

Defaults (``scripts/bench_relocalize.py``, 640x480 synthetic assets, profiles/r07_bench_relocalize.json).
``rolls = 24`` (15 degrees between neighbours, a 7.5-degree worst case): refined from the nearest entry's features, the
LM recovered 83-96 % of the seeded trials at every in-plane error measured up to 30 degrees (from the view's upright
features: 21-29 %, which is why the bank holds one entry per (view, roll)), so 24 rolls leave margin;
fewer rolls would shrink the bank (memory grows as views x rolls) and are the first thing to try on real assets.
``top_k = 8``: neighbouring views at the right roll score close to the right one, and eight refinements cost one
batched LM launch (1.7 ms) - 88 % of 50 lost-frame trials recovered.  ``shifts = 1``: the synthetic objects stay near
the image centre; a lost track with the object far off-centre wants ``shifts = 3``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .geometry import Camera, Pose
from .ops import ops
from .optimizer import PixTrackOptimizer
from .unet import OUTPUT_DIMS
from .utils.pose_utils import geodesic_distances_to


# ------------------------------------------------------------------------------------------ host helpers (pure)
def robust_rho(kind: int, alpha: float, scale: float, x: float) -> float:
    """The LM's loss (pxt_lm.hip robust_loss, pixloc scaled_loss) of a squared distance ``x``, in float64."""
    if kind == 0:
        return float(x)
    a2 = scale * scale
    y = x / a2
    if kind == 1:
        l = y if y <= 1.0 else 2.0 * math.sqrt(y) - 1.0
    elif alpha == 0.0:
        l = 2.0 * math.log1p(0.5 * y)
    elif alpha == 2.0:
        l = y
    else:
        beta = max(abs(alpha - 2.0), 1e-7)
        a = (1.0 if alpha >= 0 else -1.0) * max(abs(alpha), 1e-7)
        l = 2.0 * (beta / a) * ((y / beta + 1.0) ** (0.5 * alpha) - 1.0)
    return l * a2


def rank_scores(out: torch.Tensor, counts: torch.Tensor, rho2: float, min_valid: int) -> torch.Tensor:
    """Score of each hypothesis from the kernel's sums (out [M, 4], counts [M] = points of its range):
    (sum rho + (N_h - n_valid) rho(2)) / N_h - a point outside the image costs what two independent unit descriptors
    cost, so leaving the image is not free.  Hypotheses with n_valid < min_valid score +inf (ranked last)."""
    n = counts.to(out.dtype)
    score = (out[:, 0] + (n - out[:, 1]) * rho2) / n.clamp_min(1)
    return torch.where(out[:, 1] >= min_valid, score, torch.full_like(score, float("inf")))


def top_candidates(score: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k lowest scores, ties broken by index (a stable sort: the same order on every run)."""
    return torch.sort(score, stable=True).indices[: min(k, score.numel())]


def _rz(theta: float) -> np.ndarray:
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def shift_pixels(camera10: Sequence[float], shifts: int) -> List[Tuple[float, float]]:
    """Target pixels of the object centre for a ``shifts x shifts`` grid over the middle half of the image
    (row-major).  shifts = 1: none (the view's own placement)."""
    if shifts <= 1:
        return []
    w, h = float(camera10[0]), float(camera10[1])
    f = [0.25 + 0.5 * i / (shifts - 1) for i in range(shifts)]
    return [(w * fx - 0.5, h * fy - 0.5) for fy in f for fx in f]


def make_hypotheses(views: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], rolls: int, shifts: int = 1,
                    camera10: Optional[Sequence[float]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Hypothesis poses for ``views`` = [(R_v, t_v, object centre in world)]: for each view, ``rolls`` rotations about
    the optical axis (roll j: theta = 2 pi j / rolls, R = Rz R_v, t = Rz t_v; j = 0 is the db pose itself) and, when
    ``shifts`` > 1, for each roll the ``shifts x shifts`` grid of translations that put the object centre's pinhole
    projection on shift_pixels(camera10, shifts) at the centre's depth.  Returns (poses [M, 12] float64, view index
    [M]) with M = views x rolls x max(1, shifts)^2, ordered view, roll, shift."""
    targets = shift_pixels(camera10, shifts) if shifts > 1 else [None]
    if shifts > 1 and camera10 is None:
        raise ValueError("shift hypotheses need the query camera")
    poses, owner = [], []
    for vi, (Rv, tv, centre) in enumerate(views):
        Rv, tv, centre = (np.asarray(a, np.float64) for a in (Rv, tv, centre))
        for j in range(rolls):
            Rz = _rz(2.0 * math.pi * j / rolls)
            R, t = (Rv, tv) if j == 0 else (Rz @ Rv, Rz @ tv)
            for tgt in targets:
                tt = t
                if tgt is not None:
                    fx, fy, cx, cy = (float(x) for x in camera10[2:6])
                    c = R @ centre + t
                    tt = t + np.array([(tgt[0] - cx) / fx * c[2] - c[0], (tgt[1] - cy) / fy * c[2] - c[1], 0.0])
                poses.append(np.concatenate([R.reshape(-1), tt]))
                owner.append(vi)
    return np.asarray(poses, np.float64).reshape(-1, 12), np.asarray(owner, np.int64)


# ---------------------------------------------------------------------------------------------------- result
@dataclass
class RelocResult:
    pose: Optional[Pose]        # the refined pose of the best candidate (None: every refinement failed)
    cost: float                 # its final masked-mean cost (level 0, last iteration); inf when none succeeded
    view_id: Optional[int]      # db id of the view whose features refined it
    n_hypotheses: int
    candidates: List[Dict] = field(default_factory=list)  # per refined candidate: hypothesis, view_id, score, cost, failed, pose


@dataclass
class _View:
    """One bank entry: a mapping view at one roll."""
    dbid: int
    roll: int
    R: np.ndarray
    t: np.ndarray
    centre: np.ndarray
    begin: int
    count: int
    ref: object  # SparseReferenceFeatures (all three levels)


class Relocalizer:
    """``localize(query_image, camera)`` -> RelocResult.  ``localizer``: the tracker's PoseTrackerLocalizer (its
    refiner, extractor and optimizers are used as they are); ``render(pose) -> uint8 [H, W, 3]``: the reference image
    at a pose with the reference camera (PixLocPoseTrackerR9.get_reference_image); ``views``: db ids of the mapping
    views to bank (default: all, at most ``max_views`` of them, evenly spaced in id order)."""

    def __init__(self, localizer, views: Optional[Sequence[int]] = None, rolls: int = 24, shifts: int = 1, top_k: int = 8,
                 score_level: int = 2, max_views: int = 64, render: Optional[Callable] = None, min_valid: Optional[int] = None):
        if not 1 <= top_k <= _lib.PXT_LM_MAX_BATCH:
            raise ValueError(f"top_k must be in 1..{_lib.PXT_LM_MAX_BATCH}")
        if rolls < 1 or shifts < 1 or not 0 <= score_level < len(OUTPUT_DIMS):
            raise ValueError("rolls >= 1, shifts >= 1, score_level a pyramid level")
        self.localizer = localizer
        self.refiner = localizer.refiner
        self.device = self.refiner.device
        self.view_ids = list(views) if views is not None else None
        self.rolls, self.shifts, self.top_k, self.score_level, self.max_views = int(rolls), int(shifts), int(top_k), int(score_level), int(max_views)
        self.render = render
        opt = self.refiner.optimizer[score_level]
        self.conf = opt.native_conf()
        self.min_valid = int(self.conf.min_valid if min_valid is None else min_valid)
        self.rho2 = robust_rho(self.conf.loss, self.conf.loss_alpha, self.conf.loss_scale, 2.0)
        self.views: List[_View] = []
        self.bank = None  # (p3d [N, 3], fref [N, cstride], valid [N]) of the score level
        self.bank_bytes = 0
        self.timing = False   # record device events per localize (scripts/bench_relocalize.py)
        self.last_events = None
        self._hyp_key = None
        self._ws = None

    # ------------------------------------------------------------------------------------------- view bank
    def _bank_view_ids(self) -> List[int]:
        ids = sorted(int(k) for k in (self.view_ids if self.view_ids is not None else self.refiner.model3d.dbs))
        if len(ids) > self.max_views:
            ids = [ids[int(i * len(ids) / self.max_views)] for i in range(self.max_views)]
        return ids

    @torch.no_grad()
    def build_bank(self) -> int:
        """Renders, encodes and samples every banked view once; returns the bank's bytes."""
        if self.render is None:
            raise _lib.PxtError("Relocalizer needs render(pose) -> reference image to build its view bank")
        refiner = self.refiner
        dbs = refiner.model3d.dbs
        saved = refiner.conf.multiscale
        refiner.feature_extractor.unstage()
        refiner.conf.multiscale = [1]
        self.views = []
        p3ds, frefs, valids = [], [], []
        begin = 0
        try:
            dbids = [d for d in self._bank_view_ids() if len(refiner._points_of([d])[0]) >= max(1, self.min_valid)]
            db_poses = [(dbs[d].qvec2rotmat(), dbs[d].tvec, refiner._p3d_host[int(d)].mean(0)) for d in dbids]
            poses, owner = make_hypotheses(db_poses, self.rolls)  # one entry per (view, roll), view-major
            for k, (pose12, vi) in enumerate(zip(poses, owner)):
                dbid = dbids[int(vi)]
                R, t = pose12[:9].reshape(3, 3), pose12[9:]
                pose = Pose.from_Rt(R.astype(np.float32), t.astype(np.float32))
                ref = refiner.extract_reference_features([dbid], pose, self.render(pose))["1"]
                n = int(ref.p3d.shape[0])
                self.views.append(_View(int(dbid), k % self.rolls, R, t, db_poses[int(vi)][2], begin, n, ref))
                p3ds.append(ref.p3d)
                frefs.append(ref.packed[self.score_level])
                valids.append(ref.valid)
                begin += n
        finally:
            refiner.conf.multiscale = saved
        if not self.views:
            raise _lib.PxtError("Relocalizer: no mapping view with enough points")
        self.bank = (torch.cat(p3ds).float().contiguous(), torch.cat(frefs).contiguous(), torch.cat(valids).contiguous())
        per_view = sum(t.numel() * t.element_size() for v in self.views for t in (*v.ref.packed, v.ref.valid))
        self.bank_bytes = int(sum(t.numel() * t.element_size() for t in self.bank) + per_view)
        self._hyp_key = None
        return self.bank_bytes

    def _hypotheses(self, camera10: List[float]):
        key = tuple(camera10) if self.shifts > 1 else ()
        if self._hyp_key == key:
            return
        heads = self.views[::self.rolls]  # roll 0 of each view: the db poses
        poses, _ = make_hypotheses([(v.R, v.t, v.centre) for v in heads], self.rolls, self.shifts, camera10)
        owner = np.arange(poses.shape[0]) // (self.shifts * self.shifts)  # the (view, roll) entry of each hypothesis
        M = poses.shape[0]
        ranges = np.array([[self.views[o].begin, self.views[o].count] for o in owner] + [[0, 0]], np.int32)
        self.hyp_poses = np.concatenate([poses, np.zeros((1, 12))]).astype(np.float32)  # + a slot for the last pose
        self.hyp_owner = np.concatenate([owner, [0]])
        self._poses_dev = torch.from_numpy(self.hyp_poses).to(self.device)
        self._ranges_dev = torch.from_numpy(ranges).to(self.device)
        self._counts_dev = self._ranges_dev[:, 1].clone()
        self._out = torch.empty(M + 1, 4, device=self.device)
        self.n_static = M
        self._hyp_key = key

    @property
    def n_views(self) -> int:
        return len(self.views) // self.rolls

    def nearest_view(self, R: np.ndarray) -> int:
        """Index into self.views (the bank's (view, roll) entries) of the entry nearest to rotation R (geodesic distance)."""
        return int(np.argmin(geodesic_distances_to(np.asarray(R, np.float64), np.stack([v.R for v in self.views]))))

    # ------------------------------------------------------------------------------------------- localize
    @torch.no_grad()
    def localize(self, query_image, camera: Camera, last_pose: Optional[Pose] = None) -> RelocResult:
        if self.bank is None:
            self.build_bank()
        refiner = self.refiner
        camera10 = [float(x) for x in camera.as10().tolist()]
        self._hypotheses(camera10)
        M = self.n_static
        stream = torch.cuda.current_stream(self.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.timing else None
        if ev:
            ev[0].record(stream)
        if last_pose is not None:  # the tracker's last accepted pose, scored with its nearest view's points
            R, t = last_pose.numpy()
            vi = self.nearest_view(R)
            v = self.views[vi]
            self.hyp_poses[M] = np.concatenate([np.asarray(R).reshape(-1), np.asarray(t).reshape(-1)])
            self.hyp_owner[M] = vi
            # (pinned sources and non-blocking copies: no wait on the stream)
            self._poses_dev[M].copy_(torch.from_numpy(self.hyp_poses[M].copy()).pin_memory(), non_blocking=True)
            self._ranges_dev[M].copy_(torch.tensor([v.begin, v.count], dtype=torch.int32).pin_memory(), non_blocking=True)
            self._counts_dev[M].fill_(v.count)
            M += 1
        # 1. one unmasked UNet pass over the query at image scale 1
        refiner.feature_extractor.unstage()
        maps_q, scales_q = refiner.dense_feature_extraction(query_image, "relocalize", 1, mask=None, normalize=True)
        if ev:
            ev[1].record(stream)
        # 2. one scoring launch on the score level
        lvl = self.score_level
        cam_l = camera.scale(scales_q[lvl])
        p3d, fref, valid = self.bank
        out = self._out[:M]
        ops.score_pose_hypotheses(maps_q[lvl], int(OUTPUT_DIMS[lvl]), [float(x) for x in cam_l.as10().tolist()],
                                  int(cam_l._data.shape[-1] - 6), p3d, fref, valid, self._poses_dev[:M],
                                  self._ranges_dev[:M], int(self.conf.pad), int(self.conf.loss), float(self.conf.loss_alpha),
                                  float(self.conf.loss_scale), out)
        # 3. ranking on the device; host read 1: the top-K indices
        score = rank_scores(out, self._counts_dev[:M], self.rho2, self.min_valid)
        top = top_candidates(score, self.top_k)
        top_score = score[top]
        if ev:
            ev[2].record(stream)
        pair = torch.stack([top.double(), top_score.double()]).cpu()
        idx, scores = [int(x) for x in pair[0].tolist()], pair[1].tolist()
        # 4. the K candidates refined in one batched LM launch, each with its own view's features
        if self._ws is None:
            n = int(_lib.lib().pxt_lm_workspace_bytes())
            self._ws = [torch.zeros(n, dtype=torch.uint8, device=self.device) for _ in range(_lib.PXT_LM_MAX_BATCH)]
            self._batch_ws = torch.empty(int(_lib.lib().pxt_lm_batch_workspace_bytes(_lib.PXT_LM_MAX_BATCH)),
                                         dtype=torch.uint8, device=self.device)
        saved_cam = getattr(refiner, "lm_camera", None)
        refiner.lm_camera = None
        try:
            problems = []
            for k, h in enumerate(idx):
                view = self.views[int(self.hyp_owner[h])]
                prob = refiner.lm_problem(maps_q, scales_q, camera, Pose(torch.from_numpy(self.hyp_poses[h].copy())), view.ref)
                prob["workspace"] = self._ws[k]
                problems.append(prob)
        finally:
            refiner.lm_camera = saved_cam
        conf = problems[0]["conf"]
        pending = PixTrackOptimizer.refine_levels_batch(problems, conf, self._batch_ws, want_log=True, pool_key="relocalize")
        if ev:
            ev[3].record(stream)
        # host read 2: the K results
        results = [p.result() for p in pending]
        self.last_events = ev
        cands = []
        for h, s, res in zip(idx, scores, results):
            view = self.views[int(self.hyp_owner[h])]
            final = res.costs[-1][-1] if res.costs and res.costs[-1] else float("nan")
            cost = float("inf") if res.failed or not math.isfinite(final) else float(final)
            cands.append({"hypothesis": int(h), "view_id": view.dbid, "score": float(s), "cost": cost,
                          "failed": bool(res.failed), "pose": None if res.failed else Pose(res.T.as12().clone())})
        best = min(cands, key=lambda c: c["cost"])
        if best["pose"] is None:
            return RelocResult(None, float("inf"), None, M, cands)
        return RelocResult(best["pose"], best["cost"], best["view_id"], M, cands)

    def timings_ms(self) -> Optional[Dict[str, float]]:
        """Device times of the last localize (timing = True): UNet pass, scoring + ranking, batched LM."""
        ev = self.last_events
        if not ev:
            return None
        ev[3].synchronize()
        return {"unet": ev[0].elapsed_time(ev[1]), "score": ev[1].elapsed_time(ev[2]), "lm": ev[2].elapsed_time(ev[3]),
                "total": ev[0].elapsed_time(ev[3])}
