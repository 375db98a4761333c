"""Occlusion handling from the frame's sensor depth image (``pxt_occlusion_mask`` / ``pxt_points_visible``,
include/pixtrack_hip.h; opt-in).

On a steady frame the tracker multiplies the query by the dilated NeRF silhouette at the previous pose and refines on
every reference point that projects into the image.  A hand or a neighbouring object in front of the tracked one sits
inside that silhouette, and every point that projects onto it contributes a residual against the wrong surface.  Where
the data set keeps a depth image beside every colour frame, the pixels that show something in FRONT of the object can
be told - the ``bop19`` visibility rule of ``sensor_evaluation``, turned round:

    sil = alpha >= min_alpha and depth > 0;  q = depth / alpha;  d_s = float(raw) * sensor_q
    O   = sil and raw != 0 and q - d_s > delta_q
    E   = erosion of O, (2 r_open + 1)^2 box, pixels outside the image ignored      (specks go)
    G   = dilation of E, (2 r_grow + 1)^2 box, inside the image                      (the occluder's rim goes too)
    mask_out = mask_in and not G

and a reference point whose projection's nearest texel lies in G leaves the LM's point mask (``points_visible``).

* ``occlusion_mask`` / ``points_visible``: the device wrappers of ``torch.ops.pixtrack.occlusion_mask`` /
  ``points_visible``; both only enqueue.
* ``occlusion_mask_views``: the same pass for up to 16 image pairs of different sizes in one chain of two launches
  (``pxt_occlusion_mask_views``) - the mesh objects of one RGB-D frame; ``mesh_quanta``: the quanta of a mesh template's
  float depth plane.
* ``mask_exclude`` / ``mask_exclude_reference``: a mask minus an occluder plane that some other call made - the lock-step
  tracker's mutual occlusion takes the plane from the other tracked meshes (``pxt_mesh_render_scene_batch``).
* ``occlusion_mask_reference`` / ``points_visible_reference``: the numpy float32 restatements - the oracles of the
  tests.  The mask rules are single IEEE operations and are restated exactly; the projection is not (the kernel's FMA
  contraction), so a point within 1e-3 px of a texel boundary is *fragile* (``points_visible_reference`` marks it).
* ``OcclusionConf`` / ``OcclusionMask``: the tracker option (``PixLocPoseTrackerR9(occlusion=...)``).

``delta`` is a FRACTION of the SfM model's extent by default (an SfM model has no metric scale).  The defaults - delta
0.1, r_open 1, r_grow 3, min_alpha 0.5 - are untuned starting values: nobody has run this on real depth frames.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from .depth_refinement import _camera10, _project
from .sensor_evaluation import MAX_RESIDUAL_PX, sensor_alignment, shifted_sensor

RECORD = 16          # PXT_OCCLUSION_RECORD
MAX_RADIUS = 16      # PXT_OCCLUSION_MAX_RADIUS: r_open + r_grow
MAX_VIEWS = 16       # PXT_OCCLUSION_MAX_VIEWS: image pairs of one occlusion_mask_views call
RECORD_NAMES = ("n_sil", "n_measured", "n_occluded", "n_opened", "n_occluder", "n_mask_in", "n_mask_out",
                "n_sil_occluder", "n_points", "n_points_in", "n_points_out")
FRAGILE_PX = 1e-3


def check_radii(r_open, r_grow) -> Tuple[int, int]:
    ro, rg = int(r_open), int(r_grow)
    if ro != r_open or rg != r_grow or ro < 0 or rg < 0 or ro + rg > MAX_RADIUS:
        raise ValueError(f"r_open, r_grow are integers >= 0 with r_open + r_grow <= {MAX_RADIUS} (got {r_open}, {r_grow})")
    return ro, rg


@dataclass(frozen=True)
class OcclusionConf:
    """``delta``: how much closer than the object the sensor's surface must be for a pixel to show an occluder - with
    ``relative`` (the default) a fraction of the SfM model's extent, ``resolve(extent)`` gives the absolute conf.
    ``r_open`` / ``r_grow``: the box radii of the opening and the growth.  Untuned starting values (module docstring)."""
    delta: float = 0.1
    relative: bool = True
    r_open: int = 1
    r_grow: int = 3
    min_alpha: float = 0.5
    allow_misaligned: bool = False

    def __post_init__(self):
        check_radii(self.r_open, self.r_grow)
        if not (float(self.delta) >= 0.0 and np.isfinite(self.delta)):
            raise ValueError(f"delta must be finite and >= 0 (got {self.delta})")

    def resolve(self, extent: float) -> "OcclusionConf":
        if not self.relative:
            return self
        e = float(extent)
        if not (e > 0.0 and np.isfinite(e)):
            raise ValueError(f"the point set's extent must be positive and finite (got {extent})")
        return replace(self, delta=self.delta * e, relative=False)


@dataclass
class OcclusionMask:
    """The tracker option: ``lookup(frame_name) -> uint16 [H, W]`` (None: the frame has no depth image and runs as
    without the option), the sensor's scale in SfM units per count, and a conf (relative: resolved once with the SfM
    model's extent)."""
    lookup: Callable[[str], Optional[np.ndarray]]
    sensor_depth_scale: float
    conf: OcclusionConf = OcclusionConf()


HISTORY_KEYS = ("occluded_fraction", "n_occluder_pixels", "n_points_gated", "occlusion_applied")


def quantize(delta: float, sensor_depth_scale: float, z_scale: float) -> Tuple[float, float]:
    """``(sensor_q, delta_q)``: the distance of one raw count and the tolerance in units of ``q = depth / alpha``, each
    formed in float64 and rounded once to float32 (as ``sensor_evaluation`` does with ``render_evaluation.z_scale``)."""
    zs = float(z_scale)
    if not (zs > 0.0 and np.isfinite(zs)) or not float(sensor_depth_scale) > 0.0:
        raise ValueError(f"z_scale and sensor_depth_scale must be positive (got {z_scale}, {sensor_depth_scale})")
    return float(np.float32(float(sensor_depth_scale) / zs)), float(np.float32(float(delta) / zs))


def mesh_quanta(delta: float, sensor_depth_scale: float, view_record) -> Tuple[float, float]:
    """``(sensor_q, delta_q)`` for the float depth plane of a MESH template's frame call (``MeshTemplate.frame(...,
    want_depth=True)``: ``(d, d, d, 1)`` on covered pixels, d = z * depth_q).  One unit of ``q = v.x / v.w`` is
    ``1 / depth_q`` SfM units, ``depth_q`` being the float32 word [17] of the view record the plane was drawn with, taken
    to float64: ``quantize(delta, sensor_depth_scale, 1.0 / depth_q)``.  ``depth_q`` changes with every frame, so the
    quanta are formed per frame.  The view is drawn with the camera's true cx, cy, so the shift is (0, 0)."""
    rec = np.asarray(view_record.detach().cpu().numpy() if hasattr(view_record, "detach") else view_record).reshape(-1)
    if rec.size < 18:
        raise ValueError(f"a mesh view record holds 20 floats (got {rec.size})")
    depth_q = float(np.float32(rec[17]))
    if not (depth_q > 0.0 and np.isfinite(depth_q)):
        raise ValueError(f"the view record's depth_q must be positive and finite (got {depth_q})")
    return quantize(delta, sensor_depth_scale, 1.0 / depth_q)


def alignment(camera, allow_misaligned: bool = False) -> Tuple[int, int, float]:
    """``sensor_evaluation.sensor_alignment`` of the query camera; a residual above 1.0 px raises ValueError unless
    ``allow_misaligned``."""
    sx, sy, residual = sensor_alignment(camera)
    if residual > MAX_RESIDUAL_PX and not allow_misaligned:
        raise ValueError(f"the sensor image stays {residual:.2f} px off the renders at the border (> {MAX_RESIDUAL_PX}); "
                         "pass allow_misaligned=True to mask anyway")
    return sx, sy, residual


# --------------------------------------------------------------------------------------------------- reference
def _box(plane: np.ndarray, r: int, erode: bool) -> np.ndarray:
    """Erosion (AND) / dilation (OR) of a bool [H, W] plane with the (2 r + 1)^2 box; a position outside the image is
    ignored - it neither clears an erosion nor sets a dilation."""
    H, W = plane.shape
    neutral = erode
    pad = np.full((H + 2 * r, W + 2 * r), neutral, dtype=bool)
    pad[r:r + H, r:r + W] = plane
    rows = pad.copy()
    for d in range(1, 2 * r + 1):  # along x: columns c .. c + 2 r of the padded plane
        shifted = pad[:, d:]
        rows[:, :shifted.shape[1]] = (rows[:, :shifted.shape[1]] & shifted) if erode else (rows[:, :shifted.shape[1]] | shifted)
    rows = rows[:, :W]
    out = rows.copy()
    for d in range(1, 2 * r + 1):
        shifted = rows[d:, :]
        out[:shifted.shape[0]] = (out[:shifted.shape[0]] & shifted) if erode else (out[:shifted.shape[0]] | shifted)
    return out[:H]


def occlusion_mask_reference(depth, sensor, mask_in, shift, min_alpha, sensor_q, delta_q, r_open, r_grow) -> Dict:
    """numpy float32 restatement of ``pxt_occlusion_mask`` on a ``[H, W, 4]`` Depth image, uint16 ``[H, W]`` sensor
    counts and a uint8 ``[H, W]`` mask.  Every quotient, product and difference is one float32 operation.

    -> dict(mask uint8 [H, W], occluder uint8 [H, W], record int32 [16], sil, occluded, opened: bool planes)."""
    v = np.asarray(depth, np.float32)
    s = np.asarray(sensor)
    m = np.asarray(mask_in)
    if v.ndim != 3 or v.shape[2] != 4:
        raise ValueError(f"depth must be [H, W, 4] (got {v.shape})")
    H, W = v.shape[:2]
    if s.dtype != np.uint16 or s.shape != (H, W):
        raise ValueError(f"sensor must be a uint16 {(H, W)} array (got {s.dtype} {s.shape})")
    if m.shape != (H, W):
        raise ValueError(f"mask_in must be {(H, W)} (got {m.shape})")
    ro, rg = check_radii(r_open, r_grow)
    ma, sq, dq = np.float32(min_alpha), np.float32(sensor_q), np.float32(delta_q)
    raw = shifted_sensor(s, shift)
    with np.errstate(all="ignore"):
        sil = (v[..., 3] >= ma) & (v[..., 0] > 0)
        q = v[..., 0] / v[..., 3]
        d_s = raw.astype(np.float32) * sq
        diff = q - d_s
        assert q.dtype == np.float32 and d_s.dtype == np.float32 and diff.dtype == np.float32
        measured = sil & (raw != 0)
        occluded = measured & (diff > dq)
    opened = _box(occluded, ro, erode=True)
    grown = _box(opened, rg, erode=False)
    mi = m != 0
    mo = mi & ~grown
    rec = np.zeros(RECORD, np.int32)
    rec[:8] = [sil.sum(), measured.sum(), occluded.sum(), opened.sum(), grown.sum(), mi.sum(), mo.sum(), (sil & grown).sum()]
    return {"mask": mo.astype(np.uint8), "occluder": grown.astype(np.uint8), "record": rec, "sil": sil,
            "occluded": occluded, "opened": opened}


def points_visible_reference(p3d, valid_in, T12, camera, occluder, dtype=np.float32) -> Dict:
    """numpy restatement of ``pxt_points_visible``: ``camera`` is a geometry.Camera or (10 floats, ndist), ``T12`` the
    pose (row-major R, then t), ``occluder`` the uint8 [H, W] plane.

    -> dict(valid uint8 [N], counts (n_points, n_points_in, n_points_out), u, v, projects (project_point's answer),
    texel int64 [N, 2] (x, y), gated (the points whose bit the plane cleared), fragile: the points within 1e-3 px of a
    texel boundary (a half-integer coordinate), which another rounding of the projection may place in the neighbouring
    texel; near_edge: those within 1e-3 px of the edge of project_point's image test)."""
    dt = np.dtype(dtype).type
    X = np.asarray(p3d, dtype=dt).reshape(-1, 3)
    N = len(X)
    occ = np.asarray(occluder)
    H, W = occ.shape
    cam10, ndist = _camera10(camera)
    if (float(cam10[0]), float(cam10[1])) != (float(W), float(H)):
        raise ValueError(f"the camera is {cam10[0]:g} x {cam10[1]:g}, the occluder plane {W} x {H}")
    T = np.asarray(T12.as12().detach().cpu().numpy() if hasattr(T12, "as12") else T12, dtype=dt).reshape(12)
    vin = np.ones(N, bool) if valid_in is None else np.asarray(valid_in).reshape(N) != 0
    px = T[0] * X[:, 0] + T[1] * X[:, 1] + T[2] * X[:, 2] + T[9]
    py = T[3] * X[:, 0] + T[4] * X[:, 1] + T[5] * X[:, 2] + T[10]
    pz = T[6] * X[:, 0] + T[7] * X[:, 1] + T[8] * X[:, 2] + T[11]
    with np.errstate(all="ignore"):
        u, v, _, projectable, in_img = _project(cam10, ndist, px, py, pz, dt)
        projects = projectable & in_img
        xt, yt = np.floor(u + dt(0.5)), np.floor(v + dt(0.5))
        inside = projects & (xt >= 0) & (yt >= 0) & (xt < W) & (yt < H)
        xi = np.where(inside, xt, 0).astype(np.int64)
        yi = np.where(inside, yt, 0).astype(np.int64)
        hit = inside & (occ[yi, xi] != 0)
        # distance to the nearest texel boundary (half-integers) and to the image test's edges
        fu, fv = u + dt(0.5), v + dt(0.5)
        cell = np.minimum(np.minimum(fu - np.floor(fu), np.ceil(fu) - fu), np.minimum(fv - np.floor(fv), np.ceil(fv) - fv))
        edge = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.minimum(np.abs(u - dt(W - 1)), np.abs(v - dt(H - 1))))
        finite = np.isfinite(u) & np.isfinite(v)
        fragile = projectable & finite & (cell < FRAGILE_PX)
        near_edge = projectable & finite & (edge < FRAGILE_PX)
    out = vin & ~hit
    return {"valid": out.astype(np.uint8), "counts": (N, int(vin.sum()), int(out.sum())), "u": u, "v": v,
            "projects": projects, "texel": np.stack([xi, yi], 1), "gated": vin & hit, "fragile": fragile,
            "near_edge": near_edge}


def mask_exclude_reference(mask_in, occluder) -> Dict:
    """numpy restatement of ``pxt_mask_exclude``: uint8 [H, W] planes -> dict(mask uint8 [H, W] = ``(mask_in != 0) &
    (occluder == 0)``, record (n_mask_in, n_mask_out))."""
    m, g = np.asarray(mask_in), np.asarray(occluder)
    if m.ndim != 2 or m.shape != g.shape:
        raise ValueError(f"mask_in and occluder are [H, W] planes of one size (got {m.shape}, {g.shape})")
    mi = m != 0
    mo = mi & (g == 0)
    return {"mask": mo.astype(np.uint8), "record": (int(mi.sum()), int(mo.sum()))}


def decode_record(rec) -> Dict[str, int]:
    """The 16-word record -> {name: count} (``RECORD_NAMES``)."""
    r = np.asarray(rec.detach().cpu().numpy() if hasattr(rec, "detach") else rec).reshape(-1)
    return {name: int(r[i]) for i, name in enumerate(RECORD_NAMES)}


def pass_frame(depth, sensor, mask_in, mask, occluder, shift, min_alpha, quanta, radii, record_buffer, done, view) -> Dict:
    """What a tracker keeps of one occlusion pass (one ``occlusion_mask`` call, or one view of an
    ``occlusion_mask_views`` call): its inputs, its two planes, the pinned record its launches count in and the event
    recorded behind them.  The point gate appends to ``gates`` and counts in the same record; the frame's policy adds
    ``record`` (the decoded words) and exposes the dict as ``last_occlusion``.  ``view``: the view record a mesh
    template's ``depth`` plane was drawn with (None for a NeRF Depth render)."""
    return {"depth": depth, "sensor": sensor, "mask_in": mask_in, "mask": mask, "occluder": occluder, "shift": shift,
            "min_alpha": min_alpha, "sensor_q": quanta[0], "delta_q": quanta[1], "radii": radii, "gates": [],
            "record_buffer": record_buffer, "done": done, "view": view}


# --------------------------------------------------------------------------------------------------------- GPU
def occlusion_mask(depth, sensor, mask_in, shift, min_alpha: float, sensor_q: float, delta_q: float, r_open: int,
                   r_grow: int, mask=None, occluder=None, record=None, workspace=None) -> Dict:
    """Enqueue ``torch.ops.pixtrack.occlusion_mask`` on the current stream: ``depth`` float32 [H, W, 4], ``sensor`` uint16
    (or int16) [H, W] and ``mask_in`` uint8 [H, W] device tensors (a numpy sensor image is uploaded).  ``mask`` /
    ``occluder`` / ``record`` (int32 [16], device or pinned) / ``workspace``: buffers a caller keeps across frames
    (default: fresh ones, the record on the device).  Nothing is awaited.

    -> dict(mask, occluder, record, workspace)."""
    import torch

    from . import _lib
    from .ops import ops

    ro, rg = check_radii(r_open, r_grow)
    dev = depth.device
    if not torch.is_tensor(sensor):
        sensor = torch.from_numpy(np.ascontiguousarray(np.asarray(sensor, dtype=np.uint16)).view(np.int16)).to(dev)
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if mask is None:
        mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    if occluder is None:
        occluder = torch.empty(H, W, dtype=torch.uint8, device=dev)
    if record is None:
        record = torch.zeros(RECORD, dtype=torch.int32, device=dev)
    if workspace is None:
        need = int(_lib.lib().pxt_occlusion_mask_workspace_bytes(W, H))
        if need <= 0:
            raise ValueError(f"{W} x {H} images are not supported (1..2^28 pixels)")
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ops.occlusion_mask(depth, sensor, mask_in, [int(shift[0]), int(shift[1])], float(min_alpha), float(sensor_q),
                       float(delta_q), [ro, rg], mask, occluder, record, workspace)
    return {"mask": mask, "occluder": occluder, "record": record, "workspace": workspace}


def occlusion_mask_views(depth, sensors, masks_in, shifts, min_alpha: float, quanta, r_open: int, r_grow: int,
                         masks=None, occluders=None, records=None, workspace=None) -> Dict:
    """Enqueue ``torch.ops.pixtrack.occlusion_mask_views`` on the current stream: ``occlusion_mask`` for K <= 16 image
    pairs of different sizes in one chain of two launches (the K mesh objects of one RGB-D frame).  Per view: ``depth``
    float32 [H_k, W_k, 4], ``sensors`` uint16 (or int16) [H_k, W_k] (several views may name ONE tensor) and ``masks_in``
    uint8 [H_k, W_k] device tensors, ``shifts[k]`` = (shift_x, shift_y), ``quanta[k]`` = (sensor_q, delta_q);
    ``min_alpha`` and the radii hold for the call.  ``masks`` / ``occluders`` (lists) / ``records`` (int32 [K, 16],
    device or pinned) / ``workspace``: buffers a caller keeps across frames (default: fresh ones, the records on the
    device).  View k's planes and record are bit for bit what ``occlusion_mask`` gives for that pair alone.  Nothing is
    awaited.

    -> dict(masks, occluders, records, workspace)."""
    import ctypes as C

    import torch

    from . import _lib
    from .ops import ops

    ro, rg = check_radii(r_open, r_grow)
    K = len(depth)
    if not (1 <= K <= MAX_VIEWS):
        raise ValueError(f"occlusion_mask_views takes 1..{MAX_VIEWS} views (got {K})")
    if not (len(sensors) == len(masks_in) == len(shifts) == len(quanta) == K):
        raise ValueError(f"sensors, masks_in, shifts and quanta hold one entry per view ({K}; got {len(sensors)}, "
                         f"{len(masks_in)}, {len(shifts)}, {len(quanta)})")
    for name, given in (("masks", masks), ("occluders", occluders)):
        if given is not None and len(given) != K:
            raise ValueError(f"{name} holds one plane per view ({K}; got {len(given)})")
    for k, (sh, qu) in enumerate(zip(shifts, quanta)):
        if len(sh) != 2 or len(qu) != 2:
            raise ValueError(f"shifts[{k}] is (shift_x, shift_y) and quanta[{k}] (sensor_q, delta_q)")
    dev = depth[0].device
    sizes = []
    for d in depth:
        if d.dim() != 3 or int(d.shape[2]) != 4:
            raise ValueError(f"every depth plane is [H, W, 4] (got {tuple(d.shape)})")
        sizes += [int(d.shape[1]), int(d.shape[0])]
    if masks is None:
        masks = [torch.empty(h, w, dtype=torch.uint8, device=dev) for w, h in zip(sizes[0::2], sizes[1::2])]
    if occluders is None:
        occluders = [torch.empty(h, w, dtype=torch.uint8, device=dev) for w, h in zip(sizes[0::2], sizes[1::2])]
    if records is None:
        records = torch.zeros(K, RECORD, dtype=torch.int32, device=dev)
    if workspace is None:
        need = int(_lib.lib().pxt_occlusion_mask_views_workspace_bytes(K, (C.c_int32 * (2 * K))(*sizes)))
        if need <= 0:
            raise ValueError(f"planes of {list(zip(sizes[0::2], sizes[1::2]))} are not supported (1..2^28 pixels)")
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ops.occlusion_mask_views(list(depth), list(sensors), list(masks_in), [int(v) for sh in shifts for v in sh],
                             float(min_alpha), [float(v) for qu in quanta for v in qu], [ro, rg], list(masks),
                             list(occluders), records, workspace)
    return {"masks": masks, "occluders": occluders, "records": records, "workspace": workspace}


def mask_exclude(mask_in, occluder, mask=None, record=None):
    """Enqueue ``torch.ops.pixtrack.mask_exclude`` on the current stream: ``mask_in`` minus an ``occluder`` plane that
    another call made (uint8 [H, W] device tensors) -> (mask uint8 [H, W] - ``mask`` may be ``mask_in``; default: a fresh
    plane -, record: int32, words 0 and 1 = n_mask_in, n_mask_out; default: a fresh one on the device)."""
    import torch

    from .ops import ops

    if mask is None:
        mask = torch.empty_like(mask_in)
    if record is None:
        record = torch.zeros(2, dtype=torch.int32, device=mask_in.device)
    ops.mask_exclude(mask_in, occluder, mask, record)
    return mask, record


def points_visible(p3d, valid_in, pose, camera, occluder, record=None, valid=None):
    """Enqueue ``torch.ops.pixtrack.points_visible`` on the current stream: ``p3d`` float32 [N, 3] and ``valid_in`` (uint8
    [N] or None) on the device, ``pose`` a Pose or 12 floats, ``camera`` the UNSCALED query camera (a geometry.Camera or
    (10 floats, ndist)), ``occluder`` the plane ``occlusion_mask`` wrote.  ``record``: the int32 [16] record of that call
    (words 8..10 are written; default: a fresh one).  -> (valid uint8 [N], record)."""
    import torch

    from .ops import ops

    dev = occluder.device
    p3d = p3d.to(dev, torch.float32).contiguous()
    n = int(p3d.shape[0])
    if valid is None:
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
    if record is None:
        record = torch.zeros(RECORD, dtype=torch.int32, device=dev)
    T = pose.as12() if hasattr(pose, "as12") else pose
    T = [float(x) for x in np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, dtype=np.float64).reshape(-1)]
    cam10, ndist = _camera10(camera)
    vin = None if valid_in is None else valid_in.to(dev, torch.uint8).contiguous()
    ops.points_visible(p3d, vin, T, cam10, int(ndist), occluder, valid, record)
    return valid, record
