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

The DEPTH STAGE (opt-in: ``Relocalizer(depth=RelocDepth(...))`` and ``localize(..., sensor=plane)``).
Every hypothesis above sits where its mapping view puts the object; a query taken with another camera, at another
distance or with the object off-centre needs a PLACEMENT grid per entry - lateral cell x distance factor
(``make_placements``) - which the feature scorer cannot afford (about 4 MB of gathers per hypothesis).  With a sensor
depth image a point of a hypothesis either lies on the sensed surface or it does not, which costs 14 bytes per point:
ONE ``pxt_score_pose_hypotheses_depth`` launch scores all placements on a depth bank (a seeded subset of every entry's
points), the ranking ``n_agree / count`` (-inf where fewer than ``min_in`` of the points are in the image), the stable
sort and the gather of the best ``n_geometric`` poses and ranges stay on the device, and those go through the feature
scorer, the top-K read and the batched LM as ever.  The stage does not read descriptors, so it does not depend on their
scale; the K candidates are still refined with their ENTRY's features, drawn at the mapping distance - drawing the
candidates' reference frames at their own placements is the next step.
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


# ------------------------------------------------------------------------------- the depth stage
def cell_centres(camera10: Sequence[float], grid: Tuple[int, int]) -> List[Tuple[float, float]]:
    """Centres of a ``gx x gy`` grid of cells over the image, row-major, in the Camera convention (pixel centres at
    integer coordinates): ``((i + .5) W / gx - .5, (j + .5) H / gy - .5)``."""
    gx, gy = int(grid[0]), int(grid[1])
    if gx < 1 or gy < 1:
        raise ValueError(f"grid is (gx, gy) with gx, gy >= 1 (got {grid})")
    w, h = float(camera10[0]), float(camera10[1])
    return [((i + 0.5) * w / gx - 0.5, (j + 0.5) * h / gy - 0.5) for j in range(gy) for i in range(gx)]


def make_placements(views: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], rolls: int, camera10: Sequence[float],
                    grid: Tuple[int, int] = (8, 6), distances: Sequence[float] = (1.0,)) -> Tuple[np.ndarray, np.ndarray]:
    """Placement hypotheses for ``views`` = [(R_v, t_v, object centre in world)], float64 throughout.  Per (view, roll)
    ENTRY of ``make_hypotheses(views, rolls)`` with pose (R, t) and centre c: first the entry's own pose, then for every
    distance factor s and every cell centre (px, py) of ``cell_centres(camera10, grid)`` the pose (R, t + c' - (R c + t))
    with c' = s (R c + t)_z ((px - cx) / fx, (py - cy) / fy, 1): the same rotation, the object's centre on the cell's
    pinhole ray at s times the entry's depth.  Entry-major, then distance, then the cells row-major.
    -> (poses [M, 12], entry index [M]), M = E (1 + |distances| gx gy)."""
    cells = cell_centres(camera10, grid)
    fx, fy, cx, cy = (float(x) for x in camera10[2:6])
    entries, owner = make_hypotheses(views, rolls)
    poses, entry_of = [], []
    for e, (pose12, vi) in enumerate(zip(entries, owner)):
        R, t = pose12[:9].reshape(3, 3), pose12[9:]
        centre = np.asarray(views[int(vi)][2], np.float64)
        c = R @ centre + t
        poses.append(pose12)
        for s in distances:
            z = float(s) * c[2]
            for px, py in cells:
                placed = np.array([z * ((px - cx) / fx), z * ((py - cy) / fy), z])
                poses.append(np.concatenate([pose12[:9], t + placed - c]))
        entry_of += [e] * (1 + len(distances) * len(cells))
    return np.asarray(poses, np.float64).reshape(-1, 12), np.asarray(entry_of, np.int64)


def score_hypotheses_depth_reference(p3d, valid, poses, ranges, sensor, sensor_scale, tolerance, camera,
                                     dtype=np.float32) -> Dict:
    """numpy restatement of ``pxt_score_pose_hypotheses_depth`` (include/pixtrack_hip.h has the rule): ``p3d`` [N, 3],
    ``valid`` uint8 [N] or None, ``poses`` [M, 12], ``ranges`` int [M, 2], ``sensor`` uint16 [H, W], ``camera`` a
    geometry.Camera or (10 floats, ndist).  Projection and pixel addressing are ``occlusion.points_visible_reference``'s
    (called on an all-ones plane: the points it gates are the points inside the image); d = raw * scale and r = d - p.z
    are one operation of ``dtype`` each.

    -> dict(out int32 [M, 4] = (n_in, n_measured, n_agree, n_behind), -1 for a range outside the bank; points: per
    hypothesis None or dict(index, inside, measured, agree, behind, r, pz, u, v, projectable) over its range)."""
    from .occlusion import points_visible_reference

    dt = np.dtype(dtype).type
    X = np.asarray(p3d, dtype=dt).reshape(-1, 3)
    N = len(X)
    s = np.asarray(sensor)
    if s.dtype != np.uint16 or s.ndim != 2:
        raise ValueError(f"sensor must be a uint16 [H, W] array (got {s.dtype} {s.shape})")
    vin = np.ones(N, np.uint8) if valid is None else (np.asarray(valid).reshape(N) != 0).astype(np.uint8)
    P = np.asarray(poses).reshape(-1, 12)
    rg = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    ones = np.ones(s.shape, np.uint8)
    scale, tol = dt(sensor_scale), dt(tolerance)
    out = np.zeros((len(P), 4), np.int32)
    points = []
    for h, (T12, (begin, count)) in enumerate(zip(P, rg)):
        if begin < 0 or count < 0 or begin + count > N:
            out[h] = -1
            points.append(None)
            continue
        idx = np.arange(begin, begin + count)
        ref = points_visible_reference(X[idx], vin[idx], T12, camera, ones, dtype=dt)
        inside = ref["gated"]  # in the mask, projected by project_point, texel inside the image
        T = np.asarray(T12, dtype=dt).reshape(12)
        x = X[idx]
        pz = T[6] * x[:, 0] + T[7] * x[:, 1] + T[8] * x[:, 2] + T[11]  # (points_visible_reference's own expression)
        raw = s[ref["texel"][:, 1], ref["texel"][:, 0]]
        with np.errstate(all="ignore"):
            d = raw.astype(dt) * scale
            r = d - pz
            assert d.dtype == np.dtype(dt) and r.dtype == np.dtype(dt)
            measured = inside & (raw != 0)
            agree = inside & (np.abs(r) <= tol)
            behind = inside & (r > tol)
        out[h] = [inside.sum(), measured.sum(), agree.sum(), behind.sum()]
        points.append({"index": idx, "inside": inside, "measured": measured, "agree": agree, "behind": behind, "r": r,
                       "pz": pz, "u": ref["u"], "v": ref["v"], "projects": ref["projects"]})
    return {"out": out, "points": points}


MAX_DEPTH_HYPOTHESES = 1 << 22  # pxt_score_pose_hypotheses_depth's bound on M


def score_hypotheses_depth(p3d: torch.Tensor, valid: Optional[torch.Tensor], poses: torch.Tensor, ranges: torch.Tensor,
                           sensor: torch.Tensor, sensor_scale: float, tolerance: float, camera,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Enqueue ONE ``pxt_score_pose_hypotheses_depth`` launch on the current stream: ``p3d`` float32 [N, 3] and
    ``valid`` (uint8 [N] or None) the point bank, ``poses`` float32 [M, 12], ``ranges`` int32 [M, 2] (begin, count),
    ``sensor`` the frame's raw depth counts (uint16 / int16 [H, W], 0 = no measurement) - all contiguous, on one ROCm
    device - ``camera`` the UNSCALED query camera (a geometry.Camera or (10 floats, ndist)) of the sensor's size.
    -> ``out`` int32 [M, 4] = (n_in, n_measured, n_agree, n_behind) per hypothesis, on the device.  The entry point is
    called directly (it is not a registered op); the tensor checks are ops.py's."""
    from .depth_refinement import _camera10
    from .ops import _dense, _one_device, _point_mask, _sensor, _stream

    op = "score_hypotheses_depth"
    cam10, ndist = _camera10(camera)
    n = int(_dense(op, p3d, "p3d", shape=(None, 3)).shape[0])
    if n < 1:
        raise _lib.PxtError(f"{op}: p3d is {tuple(p3d.shape)}, expected [N >= 1, 3]")
    _point_mask(op, valid, n, "valid")
    M = int(_dense(op, poses, "poses", shape=(None, 12)).shape[0])
    if not 1 <= M <= MAX_DEPTH_HYPOTHESES:
        raise _lib.PxtError(f"{op}: poses is {tuple(poses.shape)}, expected [1 <= M <= {MAX_DEPTH_HYPOTHESES}, 12]")
    _dense(op, ranges, "ranges", torch.int32, (M, 2))
    _sensor(op, sensor, "sensor", (None, None))
    H, W = int(sensor.shape[0]), int(sensor.shape[1])
    if H < 1 or W < 1 or (float(cam10[0]), float(cam10[1])) != (float(W), float(H)):
        raise _lib.PxtError(f"{op}: the camera is {cam10[0]:g} x {cam10[1]:g}, the sensor image {W} x {H}")
    if out is None:
        out = torch.empty(M, 4, dtype=torch.int32, device=p3d.device)
    _dense(op, out, "out", torch.int32, (M, 4))
    _one_device(op, p3d, [(p3d, "p3d"), (valid, "valid"), (poses, "poses"), (ranges, "ranges"), (sensor, "sensor"),
                          (out, "out")])
    bank = _lib.RelocBank(p3d.data_ptr(), None, _lib.dptr(valid), n)
    cam = (_lib.C.c_float * 10)(*cam10)
    _lib.check(_lib.lib().pxt_score_pose_hypotheses_depth(
        _lib.C.byref(bank), poses.data_ptr(), ranges.data_ptr(), M, sensor.data_ptr(), W, H, float(sensor_scale),
        float(tolerance), cam, int(ndist), out.data_ptr(), _stream(p3d)), "pxt_score_pose_hypotheses_depth")
    return out


def rank_depth_scores(out: torch.Tensor, counts: torch.Tensor, min_in: float) -> torch.Tensor:
    """Score of each hypothesis from the depth kernel's counts (out int32 [M, 4], counts [M] = points of its range):
    n_agree / count, -inf (ranked last) where fewer than ``min_in`` of its points fall inside the image - a hypothesis
    that pushes the object out of the image must not win on the few points it keeps - or the range was refused."""
    n = counts.to(torch.float32)
    score = out[:, 2].to(torch.float32) / n.clamp_min(1)
    ok = (out[:, 0] >= 0) & (n > 0) & (out[:, 0].to(torch.float32) >= float(min_in) * n)
    return torch.where(ok, score, torch.full_like(score, float("-inf")))


def best_candidates(score: torch.Tensor, k: int) -> torch.Tensor:
    """Indices of the k HIGHEST scores, ties broken by index (a stable sort: the same order on every run)."""
    return torch.sort(score, descending=True, stable=True).indices[: min(k, score.numel())]


@dataclass
class RelocDepth:
    """The relocaliser's depth stage (``Relocalizer(depth=...)``, ``PixLocPoseTrackerR9(reloc_depth=...)``):
    ``lookup(frame_name) -> uint16 [H, W]`` (None: the frame has no depth image and is relocalised without the stage) and
    the sensor's scale in SfM units per count.  ``tolerance``: how far a point may lie from the sensed surface and
    still agree, as a FRACTION of the model's extent (resolved once, as DepthRefine's conf is).  ``grid`` / ``distances``:
    the placement grid per bank entry (make_placements).  ``depth_points``: points per entry in the depth bank, a seeded,
    fixed subset of the entry's bank points.  ``n_geometric``: how many placements go on to the feature scorer.
    ``min_in``: the share of an entry's points that must fall inside the image for a placement to be ranked.

    Every default is an untuned starting value: nobody has run this on real depth frames."""
    lookup: Callable[[str], Optional[np.ndarray]]
    sensor_depth_scale: float
    tolerance: float = 0.05
    grid: Tuple[int, int] = (8, 6)
    distances: Tuple[float, ...] = (0.5, 0.71, 1.0, 1.41, 2.0)
    depth_points: int = 256
    n_geometric: int = 512
    min_in: float = 0.5

    def __post_init__(self):
        if not callable(self.lookup) or not float(self.sensor_depth_scale) > 0:
            raise ValueError("RelocDepth: a lookup(frame_name) and a positive sensor_depth_scale")
        if len(self.grid) != 2 or min(int(g) for g in self.grid) < 1 or not len(self.distances) \
                or not all(float(s) > 0 and math.isfinite(float(s)) for s in self.distances):
            raise ValueError(f"RelocDepth: grid is (gx, gy) >= 1 and distances are positive factors (got {self.grid}, "
                             f"{self.distances})")
        if int(self.depth_points) < 1 or int(self.n_geometric) < 1 or not 0.0 <= float(self.min_in) <= 1.0 \
                or not (float(self.tolerance) >= 0 and math.isfinite(float(self.tolerance))):
            raise ValueError("RelocDepth: depth_points >= 1, n_geometric >= 1, 0 <= min_in <= 1, tolerance >= 0")


# ---------------------------------------------------------------------------------------------------- result
@dataclass
class RelocResult:
    pose: Optional[Pose]        # the refined pose of the best candidate (None: every refinement failed)
    cost: float                 # its final masked-mean cost (level 0, last iteration); inf when none succeeded
    view_id: Optional[int]      # db id of the view whose features refined it
    n_hypotheses: int
    candidates: List[Dict] = field(default_factory=list)  # per refined candidate: hypothesis, view_id, score, cost, failed, pose
    n_placed: Optional[int] = None      # placements the depth stage scored (None: the stage did not run)
    n_geometric: Optional[int] = None   # ... and how many of them went on to the feature scorer


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
    views to bank (default: all, at most ``max_views`` of them, evenly spaced in id order).  ``render_batch(poses) ->
    [uint8 [H, W, 3]]``: the same images for up to 32 poses in one call (a mesh template draws them as one batch); used
    for the bank where given.  ``depth``: a RelocDepth - ``localize(..., sensor=plane)`` then scores a placement grid
    against the frame's sensor depth first and hands its best to the feature scorer (module docstring, "depth stage")."""

    RENDER_BATCH = 32  # views per render_batch call (mesh_render.BATCH_MAX_VIEWS)

    def __init__(self, localizer, views: Optional[Sequence[int]] = None, rolls: int = 24, shifts: int = 1, top_k: int = 8,
                 score_level: int = 2, max_views: int = 64, render: Optional[Callable] = None, min_valid: Optional[int] = None,
                 depth: Optional[RelocDepth] = None, render_batch: Optional[Callable] = None):
        if not 1 <= top_k <= _lib.PXT_LM_MAX_BATCH:
            raise ValueError(f"top_k must be in 1..{_lib.PXT_LM_MAX_BATCH}")
        if rolls < 1 or shifts < 1 or not 0 <= score_level < len(OUTPUT_DIMS):
            raise ValueError("rolls >= 1, shifts >= 1, score_level a pyramid level")
        self.localizer = localizer
        self.refiner = localizer.refiner
        self.device = self.refiner.device
        self.view_ids = list(views) if views is not None else None
        self.rolls, self.shifts, self.top_k, self.score_level, self.max_views = int(rolls), int(shifts), int(top_k), int(score_level), int(max_views)
        self.render, self.render_batch = render, render_batch
        self.depth = depth
        self.depth_tolerance = None  # SfM units: depth.tolerance x the model's extent, resolved once
        if depth is not None:
            from .depth_refinement import points_extent

            pts = np.array([p.xyz for p in self.refiner.model3d.points3D.values()])
            self.depth_tolerance = float(depth.tolerance) * points_extent(pts)
        self.depth_bank = None       # (p3d [Nd, 3], valid [Nd]): up to depth.depth_points points of every entry
        self.depth_ranges = None     # int [entries, 2]: an entry's (begin, count) in the depth bank
        self.last_geometric = None   # device int64 [n_geometric]: the placements the last depth stage kept, best first
        self.last_feature_scores = None
        self._place_key = None
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
        if self.render is None and self.render_batch is None:
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
            entry_poses = [Pose.from_Rt(p[:9].reshape(3, 3).astype(np.float32), p[9:].astype(np.float32)) for p in poses]
            images: Dict[int, torch.Tensor] = {}
            for k, (pose12, vi) in enumerate(zip(poses, owner)):
                dbid = dbids[int(vi)]
                R, t = pose12[:9].reshape(3, 3), pose12[9:]
                pose = entry_poses[k]
                if self.render_batch is not None and k not in images:  # the next 32 entries' images in one call
                    chunk = range(k, min(k + self.RENDER_BATCH, len(entry_poses)))
                    images = dict(zip(chunk, self.render_batch([entry_poses[j] for j in chunk])))
                image = images.pop(k) if self.render_batch is not None else self.render(pose)
                ref = refiner.extract_reference_features([dbid], pose, image)["1"]
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
        self._hyp_key = self._place_key = None
        if self.depth is not None:
            self.bank_bytes += self._build_depth_bank()
        return self.bank_bytes

    def _build_depth_bank(self) -> int:
        """The depth stage's bank: per entry a seeded, fixed subset of at most ``depth.depth_points`` of its bank
        points (in bank order), gathered into one flat bank of their own -> its bytes."""
        rng = np.random.default_rng(20261)
        take, ranges, begin = [], [], 0
        for v in self.views:
            n = min(int(self.depth.depth_points), v.count)
            take.append(v.begin + np.sort(rng.choice(v.count, size=n, replace=False)))
            ranges.append((begin, n))
            begin += n
        index = torch.from_numpy(np.concatenate(take).astype(np.int64)).to(self.device)
        p3d, _, valid = self.bank
        self.depth_bank = (p3d.index_select(0, index).contiguous(), valid.index_select(0, index).contiguous())
        self.depth_ranges = np.asarray(ranges, np.int32).reshape(-1, 2)
        return int(sum(t.numel() * t.element_size() for t in self.depth_bank))

    def placement_index(self, entry: int, distance: Optional[int] = None, cell: Optional[Tuple[int, int]] = None) -> int:
        """The index among the placements (make_placements' order) of bank entry ``entry`` (an index into self.views):
        its own pose, or with ``distance`` (an index into depth.distances) and ``cell`` = (i, j) the placed one."""
        gx, gy = (int(g) for g in self.depth.grid)
        per = 1 + len(self.depth.distances) * gx * gy
        if distance is None:
            return entry * per
        return entry * per + 1 + (int(distance) * gy + int(cell[1])) * gx + int(cell[0])

    def _placements(self, camera10: List[float]):
        """The placement hypotheses of a camera, formed once: poses, their ranges in the depth bank and in the feature
        bank on the device, the poses and owners on the host for the LM."""
        key = tuple(camera10)
        if self._place_key == key:
            return
        d = self.depth
        heads = self.views[::self.rolls]
        poses, entry = make_placements([(v.R, v.t, v.centre) for v in heads], self.rolls, camera10, d.grid, d.distances)
        Mp = poses.shape[0]
        if Mp > MAX_DEPTH_HYPOTHESES:
            raise ValueError(f"{Mp} placements (at most {MAX_DEPTH_HYPOTHESES}): a smaller grid, fewer distances or views")
        self.place_poses = poses.astype(np.float32)
        self.place_entry = entry
        feat = np.array([[self.views[e].begin, self.views[e].count] for e in entry], np.int32)
        self._place_poses_dev = torch.from_numpy(self.place_poses).to(self.device)
        self._place_depth_ranges = torch.from_numpy(np.ascontiguousarray(self.depth_ranges[entry])).to(self.device)
        self._place_feat_ranges = torch.from_numpy(feat).to(self.device)
        self._place_counts = self._place_depth_ranges[:, 1].clone()
        self._place_out = torch.empty(Mp, 4, dtype=torch.int32, device=self.device)
        G = min(int(d.n_geometric), Mp)
        # the feature stage's inputs: the G survivors, + a slot for the last pose
        self._geo_poses = torch.zeros(G + 1, 12, device=self.device)
        self._geo_ranges = torch.zeros(G + 1, 2, dtype=torch.int32, device=self.device)
        self._geo_out = torch.empty(G + 1, 4, device=self.device)
        self._geo_last = torch.full((1,), Mp, dtype=torch.int64, device=self.device)  # the last pose's "placement index"
        self.n_placed, self.n_geometric = Mp, G
        self._place_key = key

    def _depth_stage(self, camera: Camera, camera10: List[float], sensor: torch.Tensor):
        """Steps 1-4 of a localize with the depth stage: ONE depth launch over all placements, the ranking on the device,
        the survivors' poses and feature-bank ranges gathered on the device.  No host read."""
        self._placements(camera10)
        p3d, valid = self.depth_bank
        score_hypotheses_depth(p3d, valid, self._place_poses_dev, self._place_depth_ranges, sensor,
                               float(self.depth.sensor_depth_scale), self.depth_tolerance, camera, out=self._place_out)
        score = rank_depth_scores(self._place_out, self._place_counts, self.depth.min_in)
        keep = best_candidates(score, self.n_geometric)
        G = self.n_geometric
        torch.index_select(self._place_poses_dev, 0, keep, out=self._geo_poses[:G])
        torch.index_select(self._place_feat_ranges, 0, keep, out=self._geo_ranges[:G])
        self.last_geometric = keep
        return keep

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
    def localize(self, query_image, camera: Camera, last_pose: Optional[Pose] = None, sensor=None) -> RelocResult:
        """``sensor``: the frame's raw depth counts on the device (uint16 / int16 [H, W] of the camera's size; a numpy
        uint16 array is uploaded) - with a ``depth`` option the placement grid is scored against it first; without
        either, exactly the feature-only relocalisation."""
        if self.bank is None:
            self.build_bank()
        if self.depth is not None and sensor is not None:
            return self._localize_placed(query_image, camera, last_pose, sensor)
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
        pending = self._refine_candidates(maps_q, scales_q, camera,
                                          [(self.hyp_poses[h], int(self.hyp_owner[h])) for h in idx])
        if ev:
            ev[3].record(stream)
        # host read 2: the K results
        results = [p.result() for p in pending]
        self.last_events = ev
        return self._result(idx, scores, [self.views[int(self.hyp_owner[h])] for h in idx], results, M)

    @torch.no_grad()
    def _localize_placed(self, query_image, camera: Camera, last_pose: Optional[Pose], sensor) -> RelocResult:
        """localize with the depth stage: the placements are ranked by the sensor depth (one launch), the best
        ``n_geometric`` of them - and the last pose - by the feature scorer (one launch), the top K of those refined in
        one batched LM launch.  The same two host reads as without the stage."""
        refiner = self.refiner
        camera10 = [float(x) for x in camera.as10().tolist()]
        if not torch.is_tensor(sensor):
            plane = np.ascontiguousarray(np.asarray(sensor))
            if plane.dtype != np.uint16 or plane.ndim != 2:
                raise ValueError(f"sensor is uint16 [H, W] (got {plane.dtype} {plane.shape})")
            sensor = torch.from_numpy(plane.view(np.int16)).to(self.device)
        if tuple(sensor.shape) != (int(round(camera10[1])), int(round(camera10[0]))):
            raise ValueError(f"the sensor depth image is {tuple(sensor.shape)}, the query camera "
                             f"{int(round(camera10[0]))} x {int(round(camera10[1]))}")
        stream = torch.cuda.current_stream(self.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if self.timing else None
        if ev:
            ev[0].record(stream)
        # 1.-4. the depth stage: the survivors' poses and feature-bank ranges stand in _geo_poses / _geo_ranges
        keep = self._depth_stage(camera, camera10, sensor)
        if ev:
            ev[4].record(stream)
        G = M = self.n_geometric
        last = None
        if last_pose is not None:  # the tracker's last accepted pose, scored with its nearest view's points
            R, t = last_pose.numpy()
            vi = self.nearest_view(R)
            v = self.views[vi]
            last = (np.concatenate([np.asarray(R).reshape(-1), np.asarray(t).reshape(-1)]).astype(np.float32), vi)
            self._geo_poses[G].copy_(torch.from_numpy(last[0].copy()).pin_memory(), non_blocking=True)
            self._geo_ranges[G].copy_(torch.tensor([v.begin, v.count], dtype=torch.int32).pin_memory(), non_blocking=True)
            keep = torch.cat([keep, self._geo_last])
            M += 1
        # 5. the feature stage as ever: one unmasked UNet pass, one scoring launch, ranking, top-K host read, batched LM
        refiner.feature_extractor.unstage()
        maps_q, scales_q = refiner.dense_feature_extraction(query_image, "relocalize", 1, mask=None, normalize=True)
        if ev:
            ev[1].record(stream)
        lvl = self.score_level
        cam_l = camera.scale(scales_q[lvl])
        p3d, fref, valid = self.bank
        out = self._geo_out[:M]
        ops.score_pose_hypotheses(maps_q[lvl], int(OUTPUT_DIMS[lvl]), [float(x) for x in cam_l.as10().tolist()],
                                  int(cam_l._data.shape[-1] - 6), p3d, fref, valid, self._geo_poses[:M],
                                  self._geo_ranges[:M], int(self.conf.pad), int(self.conf.loss), float(self.conf.loss_alpha),
                                  float(self.conf.loss_scale), out)
        score = rank_scores(out, self._geo_ranges[:M, 1], self.rho2, self.min_valid)
        top = top_candidates(score, self.top_k)
        self.last_feature_scores = (keep, score)  # (device tensors: the survivors' placement indices and feature scores)
        if ev:
            ev[2].record(stream)
        pair = torch.stack([keep[top].double(), score[top].double()]).cpu()  # host read 1: placement indices, scores
        idx, scores = [int(x) for x in pair[0].tolist()], pair[1].tolist()
        hyp = [(last if h == self.n_placed else (self.place_poses[h], int(self.place_entry[h]))) for h in idx]
        results = self._refine_candidates(maps_q, scales_q, camera, hyp)
        if ev:
            ev[3].record(stream)
        results = [p.result() for p in results]  # host read 2: the K results
        self.last_events = ev
        res = self._result(idx, scores, [self.views[e] for _, e in hyp], results, self.n_placed + (last is not None))
        res.n_placed, res.n_geometric = self.n_placed, G
        return res

    def _refine_candidates(self, maps_q, scales_q, camera, hyp):
        """The candidates ``hyp`` = [(pose12 float32, bank entry)] refined in one batched LM launch, each with its own
        entry's features -> the pending results."""
        refiner = self.refiner
        if self._ws is None:
            n = int(_lib.lib().pxt_lm_workspace_bytes())
            self._ws = [torch.zeros(n, dtype=torch.uint8, device=self.device) for _ in range(_lib.PXT_LM_MAX_BATCH)]
            self._batch_ws = torch.empty(int(_lib.lib().pxt_lm_batch_workspace_bytes(_lib.PXT_LM_MAX_BATCH)),
                                         dtype=torch.uint8, device=self.device)
        saved_cam = getattr(refiner, "lm_camera", None)
        refiner.lm_camera = None
        try:
            problems = []
            for k, (pose12, entry) in enumerate(hyp):
                prob = refiner.lm_problem(maps_q, scales_q, camera, Pose(torch.from_numpy(np.array(pose12, np.float32))),
                                          self.views[entry].ref)
                prob["workspace"] = self._ws[k]
                problems.append(prob)
        finally:
            refiner.lm_camera = saved_cam
        conf = problems[0]["conf"]
        return PixTrackOptimizer.refine_levels_batch(problems, conf, self._batch_ws, want_log=True, pool_key="relocalize")

    @staticmethod
    def _result(idx, scores, views, results, n_hypotheses) -> RelocResult:
        cands = []
        for h, s, view, res in zip(idx, scores, views, results):
            final = res.costs[-1][-1] if res.costs and res.costs[-1] else float("nan")
            cost = float("inf") if res.failed or not math.isfinite(final) else float(final)
            cands.append({"hypothesis": int(h), "view_id": view.dbid, "score": float(s), "cost": cost,
                          "failed": bool(res.failed), "pose": None if res.failed else Pose(res.T.as12().clone())})
        best = min(cands, key=lambda c: c["cost"])
        if best["pose"] is None:
            return RelocResult(None, float("inf"), None, n_hypotheses, cands)
        return RelocResult(best["pose"], best["cost"], best["view_id"], n_hypotheses, cands)

    def timings_ms(self) -> Optional[Dict[str, float]]:
        """Device times of the last localize (timing = True): UNet pass, scoring + ranking, batched LM."""
        ev = self.last_events
        if not ev:
            return None
        ev[3].synchronize()
        ms = {"unet": ev[0].elapsed_time(ev[1]), "score": ev[1].elapsed_time(ev[2]), "lm": ev[2].elapsed_time(ev[3]),
              "total": ev[0].elapsed_time(ev[3])}
        if len(ev) > 4:  # with the depth stage: its launch, ranking and gathers come first ("unet" then begins behind it)
            ms["depth"], ms["unet"] = ev[0].elapsed_time(ev[4]), ev[4].elapsed_time(ev[1])
        return ms
