"""BOP's Visible Surface Discrepancy with the frame's sensor depth image: occlusion-aware, and the visible fraction.

``render_evaluation.py`` scores a run from the NeRF's Depth renders alone, and says what that leaves out: without a
sensor depth image the visibility masks are the bare silhouettes, there is no ``delta`` tolerance and the depth is
camera-axis depth.  A tracked object is often occluded - held in a hand, standing in clutter - and a pixel an occluder
hides should count neither for nor against the estimate.  Where the data set keeps a 16-bit depth image beside every
colour frame (YCB-Video does), the figure can be computed as published (Hodan et al., ECCV 2018 / BOP 2019,
``visib_mode = bop19``, step cost):

  * ``d_e``, ``d_g``, ``d_s``: the LENGTH OF THE PIXEL'S RAY to the estimated render, the ground-truth render and the
    sensor's surface (``ray_factors`` turns the renders' axis depth and the sensor's z into it);
  * ``vis(d) = on the silhouette and (d - d_s <= delta or the sensor measured nothing)``; ``vis_g = vis(d_g)``;
    ``vis_e = vis(d_e) or (vis_g and on the estimate's silhouette)``;
  * ``vsd = (pixels of vis_g | vis_e that are not in both, or whose |d_e - d_g| >= tau) / (pixels of vis_g | vis_e)``;
  * ``visib_fract = |vis_g| / |silhouette of the ground truth|``: BOP scores a frame only when this is >= 0.1.

The comparison of three images per frame runs on the device (``torch.ops.pixtrack.sensor_vsd``, csrc/pxt_eval_vsd.hip)
and one 32-word record per frame is downloaded.  Nothing on the tracking path calls any of this, and
``render_evaluation.py`` / ``evaluation.py`` print what they printed before.

Alignment.  The renders ignore ``cx``, ``cy`` and ``fy`` (the principal point is the image centre, the focal length
``fx`` on both axes), the sensor image does not: it is read shifted by the rounded principal-point offset
(``sensor_alignment``).  What remains - the rounding remainder plus ``|fy / fx - 1| * H / 2`` at the image border - is
reported, and above 1.0 px the evaluation raises unless ``allow_misaligned`` is set.  The image is not resampled.

The host functions (``sensor_vsd_reference``, ``ray_factors``, ``sensor_alignment``, ``read_sensor_depth``,
``sensor_frame_figures``, ``summarize_sensor``) need no GPU; everything that renders has no CPU path.

    python -m pixtrack_amd.sensor_evaluation --poses poses.pkl --object_path P --sensor_depth_dir D
        --sensor_depth_scale S [--sensor_depth_template "{stem}.png"] [--sensor_depth_sub OLD NEW] [--delta 0.015]
        [--min_visib_fract 0.1] [--allow_misaligned] [every argument of render_evaluation]

prints ``render_evaluation``'s summary with ``vsd_sensor_mean``, ``visib_fract_mean``, ``n_below_visibility`` and
``ar_vsd_sensor`` added; ``--bop`` also adds ``ar_bop_sensor = (ar_vsd_sensor + ar_mssd + ar_mspd) / 3``.
"""
from __future__ import annotations

import argparse
import json
import math
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .evaluation import _poses_4x4
from .render_evaluation import (CHUNK_BYTES, DEFAULT_MIN_ALPHA, MAX_PAIRS_PER_CALL, THETAS, _render_depth, _require_device,
                                _thresholds, average_recall, z_scale)

MAX_TAUS = 16                         # PXT_SENSOR_VSD_MAX_TAUS
RECORD = 32                           # PXT_SENSOR_VSD_RECORD
WITHIN = 16                           # first n_within word of a record
MAX_SHIFT = 32767
DEFAULT_DELTA = 0.015                 # BOP: 15 mm; here in SfM units, like the taus
DEFAULT_MIN_VISIB_FRACT = 0.1         # BOP: a frame is scored when at least a tenth of the object is visible
MAX_RESIDUAL_PX = 1.0


# ------------------------------------------------------------------------------------------------------------------
# Host: the kernel's per-pixel rules restated, the camera's part, the figures made of the counts.
# ------------------------------------------------------------------------------------------------------------------
def shifted_sensor(sensor, shift) -> np.ndarray:
    """``out[..., y, x] = sensor[..., y + shift_y, x + shift_x]``, 0 where that position is outside the image."""
    s = np.asarray(sensor)
    sx, sy = int(shift[0]), int(shift[1])
    H, W = s.shape[-2:]
    out = np.zeros_like(s)
    x0, x1, y0, y1 = max(0, -sx), min(W, W - sx), max(0, -sy), min(H, H - sy)
    if x0 < x1 and y0 < y1:
        out[..., y0:y1, x0:x1] = s[..., y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def sensor_vsd_reference(depth_est, depth_gt, sensor, ray, shift, min_alpha, sensor_q, delta_q, tq):
    """numpy float32 restatement of pxt_sensor_vsd's per-pixel rules (include/pixtrack_hip.h) on ``[P, H, W, 4]`` (or
    ``[H, W, 4]``) Depth images, ``[P, H, W]`` uint16 sensor counts, a float32 ``[H, W]`` ray plane (None: 1.0) and
    ``shift = (shift_x, shift_y)``.  Every product and difference is one float32 operation.

    Returns ``(records, sums)``: ``records`` uint32 ``[P, 32]`` - the kernel's words, word 4 being the bits of the float32
    rounding of the sum - and ``sums`` float64 ``[P]``, the sum of the float32 ``dd`` values in float64."""
    e, g, s = np.asarray(depth_est, np.float32), np.asarray(depth_gt, np.float32), np.asarray(sensor)
    if e.ndim == 3:
        e, g, s = e[None], g[None], s[None]
    if e.ndim != 4 or e.shape[3] != 4 or g.shape != e.shape:
        raise ValueError(f"depth images must be two [P, H, W, 4] arrays of one shape (got {e.shape}, {g.shape})")
    if s.dtype != np.uint16 or s.shape != e.shape[:3]:
        raise ValueError(f"sensor must be a uint16 {e.shape[:3]} array (got {s.dtype} {s.shape})")
    tq = np.asarray(tq, np.float32).reshape(-1)
    if not (1 <= len(tq) <= MAX_TAUS):
        raise ValueError(f"{len(tq)} thresholds (1..{MAX_TAUS})")
    P, H, W = e.shape[:3]
    r = np.ones((H, W), np.float32) if ray is None else np.asarray(ray, np.float32)
    if r.shape != (H, W):
        raise ValueError(f"ray must be [{H}, {W}] (got {r.shape})")
    ma, sq, dq = np.float32(min_alpha), np.float32(sensor_q), np.float32(delta_q)
    raw = shifted_sensor(s, shift)
    with np.errstate(all="ignore"):
        sil_e = (e[..., 3] >= ma) & (e[..., 0] > 0)
        sil_g = (g[..., 3] >= ma) & (g[..., 0] > 0)
        d_e = (e[..., 0] / e[..., 3]) * r
        d_g = (g[..., 0] / g[..., 3]) * r
        d_s = (raw.astype(np.float32) * sq) * r
        none = raw == 0
        vis_g = sil_g & (((d_g - d_s) <= dq) | none)
        vis_e = (sil_e & (((d_e - d_s) <= dq) | none)) | (vis_g & sil_e)
        inter = vis_g & vis_e
        dd = np.abs(d_e - d_g)
        assert dd.dtype == np.float32 and d_s.dtype == np.float32
        finite = inter & np.isfinite(dd)
        flat = lambda m: m.reshape(P, -1)
        rec = np.zeros((P, RECORD), np.uint32)
        rec[:, 0], rec[:, 1], rec[:, 2] = flat(vis_e).sum(axis=1), flat(vis_g).sum(axis=1), flat(inter).sum(axis=1)
        rec[:, 3] = rec[:, 0] + rec[:, 1] - rec[:, 2]
        terms = flat(np.where(finite, dd, np.float32(0)))
        sums = terms.astype(np.float64).sum(axis=1)
        rec[:, 4] = sums.astype(np.float32).view(np.uint32)
        rec[:, 5] = terms.max(axis=1).astype(np.float32).view(np.uint32)
        rec[:, 6], rec[:, 7] = len(tq), 1
        rec[:, 8], rec[:, 9], rec[:, 10] = flat(sil_e).sum(axis=1), flat(sil_g).sum(axis=1), flat(~none).sum(axis=1)
        for k, t in enumerate(tq):
            rec[:, WITHIN + k] = flat(inter & (dd < t)).sum(axis=1)
    return rec, sums


def _intrinsics(camera) -> Tuple[int, int, float, float, float, float]:
    """(W, H, fx, fy, cx, cy) of a Camera, the principal point in COLMAP's convention (pixel centres at +0.5)."""
    W, H = (int(x) for x in camera.size)
    fx, fy = (float(x) for x in camera.f)
    cx, cy = (float(x) + 0.5 for x in camera.c)
    return W, H, fx, fy, cx, cy


def ray_factors(camera) -> np.ndarray:
    """float32 ``[H, W]``: ``sqrt(1 + xn^2 + yn^2)`` of every pixel under the renderer's own pixel rule (``make_ray``,
    which ``get_nerf_image_device`` uses too): pixel centre at +0.5, focal ``camera.f[0]`` on both axes, principal point
    at the image centre.  Computed in float64 and rounded once.  Camera-axis depth times this is the length of the ray."""
    W, H, fx = _intrinsics(camera)[:3]
    xn = (np.arange(W, dtype=np.float64) + 0.5 - W / 2.0) / fx
    yn = (np.arange(H, dtype=np.float64) + 0.5 - H / 2.0) / fx
    return np.sqrt(1.0 + xn[None, :] ** 2 + yn[:, None] ** 2).astype(np.float32)


def sensor_alignment(camera) -> Tuple[int, int, float]:
    """``(shift_x, shift_y, residual_px)``: the renders put the principal point at the image centre and use ``fx`` on both
    axes, so the sensor pixel that sees what render pixel (x, y) shows is (x + cx - W/2, y + cy - H/2) - the shift is that
    offset rounded (half up).  ``residual_px`` is the worst misalignment that remains, at the image border: the rounding
    remainder, plus ``|fy / fx - 1| * H / 2`` along y."""
    W, H, fx, fy, cx, cy = _intrinsics(camera)
    off_x, off_y = cx - W / 2.0, cy - H / 2.0
    sx, sy = int(math.floor(off_x + 0.5)), int(math.floor(off_y + 0.5))
    if abs(sx) > MAX_SHIFT or abs(sy) > MAX_SHIFT:
        raise ValueError(f"principal point offset ({off_x}, {off_y}) is beyond {MAX_SHIFT} px")
    residual = max(abs(off_x - sx), abs(off_y - sy) + abs(fy / fx - 1.0) * H / 2.0)
    return sx, sy, float(residual)


def check_alignment(camera, allow_misaligned: bool = False) -> Tuple[int, int, float]:
    """``sensor_alignment``, refusing a residual above 1.0 px unless ``allow_misaligned``."""
    sx, sy, residual = sensor_alignment(camera)
    if residual > MAX_RESIDUAL_PX and not allow_misaligned:
        raise ValueError(f"the sensor image stays {residual:.2f} px off the renders at the border (> {MAX_RESIDUAL_PX}: "
                         "fy differs too much from fx); pass allow_misaligned=True to evaluate anyway")
    return sx, sy, residual


def read_sensor_depth(path, size: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The raw counts of a sensor depth image, uint16 ``[H, W]``: a 16-bit single-channel PNG (read through PIL) or a
    ``.npy``.  Any other dtype - an 8-bit or a float image - is refused, and so is a size other than ``size`` = (W, H)."""
    path = str(path)
    if path.endswith(".npy"):
        a = np.load(path)
    else:
        from PIL import Image

        with Image.open(path) as im:
            if im.mode not in ("I;16", "I;16B", "I;16L"):
                raise ValueError(f"{path}: expected a 16-bit single-channel image (got mode {im.mode})")
            a = np.array(im)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise ValueError(f"{path}: expected uint16 [H, W] (got {a.dtype} {a.shape})")
    if size is not None and (a.shape[1], a.shape[0]) != (int(size[0]), int(size[1])):
        raise ValueError(f"{path}: expected {int(size[0])} x {int(size[1])} (got {a.shape[1]} x {a.shape[0]})")
    return np.ascontiguousarray(a)


def sensor_frame_figures(records, z_scale: float, n_taus: Optional[int] = None, finite_slot: Optional[int] = None,
                         sums=None) -> Dict[str, np.ndarray]:
    """Per-frame figures from pxt_sensor_vsd's records (uint32 ``[F, 32]``): ``vsd`` ``[F, n_taus]`` =
    ``(n_inter - n_within_k + n_union - n_inter) / n_union`` (BOP's step cost: an intersection pixel beyond tau and a
    pixel of one mask only cost 1), 1 when ``n_union == 0``; ``visib_fract`` = ``n_vis_gt / n_sil_gt``, 0 when the
    ground truth's silhouette is empty; ``n_vis_est``, ``n_vis_gt``, ``n_inter``, ``n_union``, ``n_sil_est``,
    ``n_sil_gt``, ``n_measured``; ``mean_abs_dd`` = ``z_scale * sum / (inter pixels with a finite dd)``, ``max_abs_dd``
    and ``ok`` (word 7 == 1).  ``n_taus``, ``finite_slot`` and ``sums`` as in ``render_evaluation.frame_figures``."""
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, RECORD)
    F = len(rec)
    if n_taus is None:
        n_taus = int(rec[0, 6]) if F else 0
    col = lambda i: rec[:, i].astype(np.int64)
    n_vis_est, n_vis_gt, n_inter, n_union, n_sil_est, n_sil_gt = col(0), col(1), col(2), col(3), col(8), col(9)
    within = rec[:, WITHIN:WITHIN + n_taus].astype(np.int64)
    seen = n_union > 0
    cost = (n_inter[:, None] - within) + (n_union - n_inter)[:, None]
    vsd = np.where(seen[:, None], cost / np.where(seen, n_union, 1)[:, None].astype(np.float64), 1.0)
    visib = np.where(n_sil_gt > 0, n_vis_gt / np.maximum(n_sil_gt, 1).astype(np.float64), 0.0)
    n_finite = n_inter if finite_slot is None else col(WITHIN + finite_slot)
    total = rec[:, 4].copy().view(np.float32).astype(np.float64) if sums is None else np.asarray(sums, np.float64)
    with np.errstate(all="ignore"):
        mean_abs_dd = np.where(n_finite > 0, float(z_scale) * total / np.maximum(n_finite, 1), np.nan)
    max_abs_dd = float(z_scale) * rec[:, 5].copy().view(np.float32).astype(np.float64)
    return dict(vsd=vsd, visib_fract=visib, n_vis_est=n_vis_est, n_vis_gt=n_vis_gt, n_inter=n_inter, n_union=n_union,
                n_sil_est=n_sil_est, n_sil_gt=n_sil_gt, n_measured=col(10), mean_abs_dd=mean_abs_dd,
                max_abs_dd=max_abs_dd, ok=rec[:, 7] == 1)


def summarize_sensor(vsd, visib_fract, evaluated, known, min_visib_fract: float = DEFAULT_MIN_VISIB_FRACT,
                     thetas: Sequence[float] = THETAS) -> Dict:
    """Summary over ALL frames of a run.  ``vsd`` ``[F, n_taus]`` holds 1 at every tau for a frame that was not
    evaluated (lost, a non-finite pose, no ground truth); ``known`` marks the frames whose ``visib_fract`` could be
    computed (ground truth, camera and sensor image present).  BOP's rule: a frame whose visible fraction is known and
    below ``min_visib_fract`` is left out of ``ar_vsd_sensor`` and counted in ``n_below_visibility``; every other frame
    counts, a lost one as a miss.  The means are over the evaluated frames."""
    vf = np.asarray(visib_fract, np.float64)
    vsd = np.asarray(vsd, np.float64).reshape(len(vf), -1)
    ev, kn = np.asarray(evaluated, bool), np.asarray(known, bool)
    below = kn & (vf < float(min_visib_fract))
    out = {"n_below_visibility": int(below.sum()), "min_visib_fract": float(min_visib_fract)}
    out["vsd_sensor_mean"] = ([float(x) for x in vsd[ev].mean(axis=0)] if ev.any() else [float("nan")] * vsd.shape[1])
    out["visib_fract_mean"] = float(vf[kn].mean()) if kn.any() else float("nan")
    out["ar_vsd_sensor"] = average_recall(vsd[~below], thetas)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Device: the renders and the comparison, a whole run.
# ------------------------------------------------------------------------------------------------------------------
def _camera_key(camera):
    return tuple(float(x) for x in camera._data[..., :6].reshape(-1))


def sensor_pose_errors(testbed, nerf2sfm, camera, T_est, T_gt, sensor_images, sensor_depth_scale: float, diameter: float,
                       delta: float = DEFAULT_DELTA, taus: Optional[Sequence[float]] = None,
                       min_alpha: float = DEFAULT_MIN_ALPHA, spp: int = 8, device=None,
                       allow_misaligned: bool = False) -> Dict[str, np.ndarray]:
    """BOP's sensor-depth VSD and the visible fraction of F (estimated, ground-truth) world-to-camera poses (``[F, 4, 4]``,
    or lists of matrices / Pose objects) of the object ``testbed`` renders, seen by ``camera`` (one Camera, or one per
    frame, all with the same intrinsics), against ``sensor_images``: F uint16 ``[H, W]`` arrays of raw counts (0 = no
    measurement).  ``sensor_depth_scale``: SfM units per raw count; ``delta`` and ``taus`` in SfM units, the taus
    defaulting to BOP's 5 % ... 50 % of ``diameter`` (at most 15 of them).

    Rendering and chunking are ``render_pose_errors``': both Depth images of every frame go straight into two
    ``[chunk, H, W, 4]`` device buffers, the chunk's sensor images are uploaded beside them, and each chunk is compared in
    one ``sensor_vsd`` call; one record per frame is downloaded at the end.  The thresholds are ``tq = tau / z_scale``,
    ``delta_q = delta / z_scale`` and ``sensor_q = sensor_depth_scale / z_scale``, each formed in float64 and rounded once.

    Returns ``sensor_frame_figures``' arrays per frame (a frame with a non-finite pose is not rendered: ``ok`` False,
    ``vsd = 1``, ``visib_fract = 0``), ``taus``, ``shift`` and ``residual_px``.  A residual above 1.0 px raises
    ValueError unless ``allow_misaligned``."""
    import torch

    from . import _lib
    from .ops import ops

    dev = _require_device(testbed.device if device is None else device)
    A, B = _poses_4x4(T_est), _poses_4x4(T_gt)
    if A.shape != B.shape:
        raise ValueError(f"{A.shape[0]} estimated and {B.shape[0]} ground-truth poses")
    F = len(A)
    cams = list(camera) if isinstance(camera, (list, tuple)) else [camera] * F
    if len(cams) != F or len(sensor_images) != F:
        raise ValueError(f"{len(cams)} cameras and {len(sensor_images)} sensor images for {F} frames")
    zs = z_scale(testbed, nerf2sfm)
    taus, tq = _thresholds(diameter, taus, zs)
    delta_q, sensor_q = float(np.float32(float(delta) / zs)), float(np.float32(float(sensor_depth_scale) / zs))
    usable = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2))
    idx = np.nonzero(usable)[0]
    rec = np.zeros((F, RECORD), np.uint32)
    shift, residual = (0, 0), 0.0
    if len(idx):
        if len({_camera_key(cams[i]) for i in idx}) != 1:
            raise ValueError("the frames of one call share one camera (size, focal lengths, principal point)")
        cam = cams[idx[0]]
        W, H = (int(x) for x in cam.size)
        sx, sy, residual = check_alignment(cam, allow_misaligned)
        shift = (sx, sy)
        ray = torch.from_numpy(ray_factors(cam)).to(dev)
        chunk = int(max(1, min(len(idx), MAX_PAIRS_PER_CALL, CHUNK_BYTES // (H * W * (2 * 16 + 2)))))
        buf_e = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        buf_g = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        records = torch.zeros(len(idx), RECORD, dtype=torch.int32, device=dev)
        need = int(_lib.lib().pxt_sensor_vsd_workspace_bytes(chunk, W, H))
        if need <= 0:
            raise ValueError(f"{W} x {H} images are not supported (1..2^28 pixels)")
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        keep = (testbed.fov, testbed._cam_ngp)
        try:
            for s in range(0, len(idx), chunk):
                part = idx[s:s + chunk]
                host = np.empty((len(part), H, W), np.uint16)
                for j, i in enumerate(part):
                    img = np.asarray(sensor_images[i])
                    if img.dtype != np.uint16 or img.shape != (H, W):
                        raise ValueError(f"sensor image {i}: expected uint16 [{H}, {W}] (got {img.dtype} {img.shape})")
                    host[j] = img
                    _render_depth(testbed, nerf2sfm, A[i], cams[i], spp, buf_e[j])
                    _render_depth(testbed, nerf2sfm, B[i], cams[i], spp, buf_g[j])
                n = len(part)
                sensor = torch.from_numpy(host.view(np.int16)).to(dev)
                ops.sensor_vsd(buf_e[:n], buf_g[:n], sensor, ray, [sx, sy], float(min_alpha), sensor_q, delta_q, tq,
                               records[s:s + n], workspace)
        finally:
            testbed.fov, testbed._cam_ngp = keep
        rec[idx] = records.cpu().numpy().view(np.uint32)
    out = sensor_frame_figures(rec, zs, n_taus=len(taus), finite_slot=len(taus))
    out["ok"] = out["ok"] & usable
    out["taus"] = np.asarray(taus, np.float64)
    out["shift"] = shift
    out["residual_px"] = float(residual)
    return out


def _lookup(sensor_lookup, name, size):
    img = sensor_lookup(name) if callable(sensor_lookup) else sensor_lookup.get(name)
    if img is None:
        return None
    return read_sensor_depth(img, size) if isinstance(img, (str, Path)) else np.asarray(img)


def evaluate_poses_sensor(poses_file: Dict, testbed, nerf2sfm, diameter: float, sensor_lookup,
                          sensor_depth_scale: float, delta: float = DEFAULT_DELTA,
                          taus: Optional[Sequence[float]] = None, min_alpha: float = DEFAULT_MIN_ALPHA, spp: int = 8,
                          device=None, min_visib_fract: float = DEFAULT_MIN_VISIB_FRACT,
                          allow_misaligned: bool = False) -> Dict:
    """The sensor-depth scoreboard of a run: ``poses_file`` as for ``evaluate_poses_rendered``; ``sensor_lookup`` maps a
    frame name to its sensor depth image (a callable or a mapping; a uint16 ``[H, W]`` array or a file for
    ``read_sensor_depth``; None: the frame has none).

    The frames that are scored are ``evaluate_poses_rendered``': ``success``, ``gt_pose``, ``T_refined`` and ``camera``
    present, both poses finite.  Any other frame is a miss, ``vsd_sensor = 1`` at every tau.  The visible fraction needs
    the ground truth only, so it is computed for every frame with ``gt_pose``, ``camera`` and a sensor image - a lost frame
    is rendered at its ground-truth pose alone for that.  BOP's rule: a frame whose ``visib_fract < min_visib_fract`` is
    left out of ``ar_vsd_sensor`` and counted in ``n_below_visibility``; a lost frame above the cut is a miss.

    Returns ``frames`` (frame name -> ``vsd_sensor`` list, ``visib_fract`` (NaN: unknown), ``n_vis_gt``, ``n_sil_gt``,
    ``mean_abs_dd``, ``max_abs_dd``, ``ok``) and the summary: ``n_frames``, ``n_evaluated``, ``vsd_sensor_mean`` (one per
    tau), ``visib_fract_mean``, ``n_below_visibility``, ``min_visib_fract``, ``ar_vsd_sensor``, ``taus``, ``diameter``,
    ``delta``, ``sensor_shift`` and ``sensor_residual_px`` (the largest over the run's cameras)."""
    dev = _require_device(testbed.device if device is None else device)
    names = list(poses_file)
    n = len(names)
    taus_used, _ = _thresholds(diameter, taus, 1.0)
    K = len(taus_used)
    scored = [bool(poses_file[k].get("success")) and poses_file[k].get("gt_pose") is not None
              and poses_file[k].get("T_refined") is not None and poses_file[k].get("camera") is not None for k in names]
    images = {}
    for i, k in enumerate(names):
        r = poses_file[k]
        if r.get("gt_pose") is not None and r.get("camera") is not None:
            img = _lookup(sensor_lookup, k, tuple(int(x) for x in r["camera"].size))
            if img is not None:
                images[i] = img
            elif scored[i]:
                raise ValueError(f"frame {k} has no sensor depth image")
    vsd, visib = np.ones((n, K)), np.full(n, np.nan)
    cols = {k: np.zeros(n, np.int64) for k in ("n_vis_gt", "n_sil_gt")}
    dd = {k: np.full(n, np.nan) for k in ("mean_abs_dd", "max_abs_dd")}
    ok, known = np.zeros(n, bool), np.zeros(n, bool)
    idx = sorted(images)
    key_of = {i: _camera_key(poses_file[names[i]]["camera"]) for i in idx}
    shift, residual = (0, 0), 0.0
    s = 0
    while s < len(idx):  # runs of consecutive frames of one camera
        e = s + 1
        while e < len(idx) and key_of[idx[e]] == key_of[idx[s]]:
            e += 1
        run = idx[s:e]
        T_gt = [_poses_4x4([poses_file[names[i]]["gt_pose"]])[0] for i in run]
        T_est = [_poses_4x4([poses_file[names[i]]["T_refined"]])[0] if scored[i] else T_gt[j] for j, i in enumerate(run)]
        res = sensor_pose_errors(testbed, nerf2sfm, [poses_file[names[i]]["camera"] for i in run], T_est, T_gt,
                                 [images[i] for i in run], sensor_depth_scale, diameter, delta=delta, taus=taus_used,
                                 min_alpha=min_alpha, spp=spp, device=dev, allow_misaligned=allow_misaligned)
        sc = np.array([scored[i] for i in run], bool) & res["ok"]
        vsd[run] = np.where(sc[:, None], res["vsd"], 1.0)
        ok[run], known[run] = sc, res["ok"]
        visib[run] = np.where(res["ok"], res["visib_fract"], np.nan)
        for k in cols:
            cols[k][run] = res[k]
        for k in dd:
            dd[k][run] = np.where(sc, res[k], np.nan)
        if res["residual_px"] >= residual:
            shift, residual = res["shift"], res["residual_px"]
        s = e
    out = {"frames": {name: dict(vsd_sensor=[float(x) for x in vsd[i]], visib_fract=float(visib[i]),
                                 n_vis_gt=int(cols["n_vis_gt"][i]), n_sil_gt=int(cols["n_sil_gt"][i]),
                                 mean_abs_dd=float(dd["mean_abs_dd"][i]), max_abs_dd=float(dd["max_abs_dd"][i]),
                                 ok=bool(ok[i])) for i, name in enumerate(names)}}
    out["n_frames"] = n
    out["n_evaluated"] = int(ok.sum())
    out.update(summarize_sensor(vsd, np.where(known, visib, 0.0), ok, known, min_visib_fract))
    out["taus"] = [float(t) for t in taus_used]
    out["diameter"] = float(diameter)
    out["delta"] = float(delta)
    out["sensor_shift"] = [int(shift[0]), int(shift[1])]
    out["sensor_residual_px"] = float(residual)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Command line.
# ------------------------------------------------------------------------------------------------------------------
def sensor_file_name(frame_name: str, template: str = "{stem}.png", sub: Optional[Sequence[str]] = None) -> str:
    """The file name of a frame's sensor depth image: ``template`` with ``{stem}`` = the frame name without its
    directory and extension, after replacing ``sub[0]`` by ``sub[1]`` in it (YCB-Video: ``color`` -> ``depth``), and
    ``{name}`` = the frame name as it is."""
    stem = Path(str(frame_name)).stem
    if sub:
        stem = stem.replace(str(sub[0]), str(sub[1]))
    return template.format(stem=stem, name=str(frame_name))


def build_parser() -> argparse.ArgumentParser:
    from .render_evaluation import build_parser as render_parser

    ap = render_parser()
    ap.prog = "python -m pixtrack_amd.sensor_evaluation"
    ap.description = ("render_evaluation's figures plus BOP's sensor-depth VSD (occlusion-aware) and the visible fraction "
                      "per frame, from the data set's 16-bit depth images")
    ap.add_argument("--sensor_depth_dir", required=True, help="directory of the frames' 16-bit depth images")
    ap.add_argument("--sensor_depth_template", default="{stem}.png",
                    help="file name of a frame's depth image; {stem}: the frame name without extension, {name}: as it is")
    ap.add_argument("--sensor_depth_sub", nargs=2, metavar=("OLD", "NEW"), default=None,
                    help="replace OLD by NEW in the stem first (YCB-Video: color depth)")
    ap.add_argument("--sensor_depth_scale", type=float, required=True, help="SfM units per raw count of the depth images")
    ap.add_argument("--delta", type=float, default=DEFAULT_DELTA, help="visibility tolerance in SfM units (BOP: 15 mm)")
    ap.add_argument("--min_visib_fract", type=float, default=DEFAULT_MIN_VISIB_FRACT,
                    help="a frame with a smaller visible fraction is left out of ar_vsd_sensor (BOP: 0.1)")
    ap.add_argument("--allow_misaligned", action="store_true",
                    help="evaluate although the sensor image stays more than 1 px off the renders at the border")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    import ast

    args = build_parser().parse_args(argv)
    _require_device(args.device)
    from .model3d import Model3D
    from .render_evaluation import bounding_box_diagonal, evaluate_poses_rendered
    from .utils.ingp_utils import get_nerf_aabb_from_sfm, initialize_ingp, load_nerf2sfm
    from .utils.io import load_reference_pickle

    obj = Path(args.object_path)
    model3d = Model3D(str(obj / "pixtrack/aug_nerf_sfm/aug_sfm"))
    nerf2sfm = load_nerf2sfm(str(obj / "pixtrack/pixsfm/dataset/nerf2sfm.pkl"))
    aabb = ast.literal_eval(args.obj_aabb) if args.obj_aabb else get_nerf_aabb_from_sfm(model3d, nerf2sfm)
    testbed = initialize_ingp(str(obj / "pixtrack/instant-ngp/snapshots/weights.msgpack"), aabb, device=args.device)
    poses = load_reference_pickle(args.poses)
    diameter = bounding_box_diagonal(model3d) if args.diameter is None else float(args.diameter)
    res = evaluate_poses_rendered(poses, testbed, nerf2sfm, diameter, min_alpha=args.min_alpha, spp=args.spp,
                                  device=args.device)

    def lookup(name):
        p = Path(args.sensor_depth_dir) / sensor_file_name(name, args.sensor_depth_template, args.sensor_depth_sub)
        return str(p) if p.exists() else None

    sen = evaluate_poses_sensor(poses, testbed, nerf2sfm, diameter, lookup, args.sensor_depth_scale, delta=args.delta,
                                min_alpha=args.min_alpha, spp=args.spp, device=args.device,
                                min_visib_fract=args.min_visib_fract, allow_misaligned=args.allow_misaligned)
    from .evaluation import merge_bop

    merge_bop(res, sen)  # the sensor keys beside render_evaluation's; keys both hold keep render_evaluation's values
    if args.bop:
        from .evaluation import bop_symmetries, evaluate_poses_bop, read_vertices

        vertices = (read_vertices(args.vertices) if args.vertices else
                    np.stack([p.xyz for p in model3d.points3D.values()]).astype(np.float64))
        merge_bop(res, evaluate_poses_bop(poses, vertices, args.device, diameter, symmetries=bop_symmetries(args),
                                          ar_vsd=res["ar_vsd"]))
        res["ar_bop_sensor"] = (res["ar_vsd_sensor"] + res["ar_mssd"] + res["ar_mspd"]) / 3.0
    summary = {k: v for k, v in res.items() if k != "frames"}
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f)
    return res


if __name__ == "__main__":
    main()
