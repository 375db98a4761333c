"""Pose evaluation from depth renders of the object's MESH: BOP's VSD as published, and the extracted mesh held against
its NeRF.

``render_evaluation.py`` and ``sensor_evaluation.py`` render the NeRF: an alpha-composited expected depth under a
``min_alpha`` convention, through a camera that ignores ``cx``, ``cy`` and ``fy`` (the sensor image has to be read shifted),
two spp-8 marches per frame, and a NeRF snapshot is needed at all.  BOP's VSD compares depth renders of the model's mesh
at the estimated and the ground-truth pose through the camera's real intrinsics (Hodan et al., ECCV 2018 / BOP 2019);
the reference project renders meshes for this kind of work (``pixtrack/utils/pytorch3d_render_utils.py:55-93``).  With the
rasteriser (``mesh_render.MeshRenderer``, csrc/pxt_raster.hip) a user who has the data set's mesh and a ``poses.pkl``
gets the figure without a snapshot:

  * a chunk's estimated and ground-truth views are drawn in two ``mesh_raster`` calls straight into the two device
    buffers that the existing ``ops.depth_agreement`` / ``ops.sensor_vsd`` compare; one record per frame is downloaded;
  * ``depth_q = 1``: the images hold camera-axis depth in the mesh's units, ``z_scale`` is 1 and ``min_alpha`` is moot
    (alpha is 0 or 1);
  * the rasteriser honours ``fx, fy, cx, cy``, so the sensor image needs no shift and no alignment check, and the ray
    factor is ``sqrt(1 + xn^2 + yn^2)`` under those intrinsics (``mesh_ray_factors``);
  * frame selection, the miss rule, the figures and the JSON keys are ``render_evaluation``'s and
    ``sensor_evaluation``'s own functions.

    python -m pixtrack_amd.mesh_evaluation --poses poses.pkl --mesh FILE [--mesh_scale S]
        [--diameter D | --models_info models_info.json [--obj_id N] [--models_info_scale X]] [--json OUT] [--bop]
        [--sensor_depth_dir D --sensor_depth_scale S [--sensor_depth_template ...] [--sensor_depth_sub OLD NEW]
         [--delta 0.015] [--min_visib_fract 0.1]] [--device cuda:0]

``mesh_nerf_agreement`` draws a mesh in the ``ngp`` frame through the NeRF renderer's own camera rule
(``mesh_render.ngp_view_record``) beside the NeRF's Depth render of the same views and reports silhouette IoU and mean
depth error per view: the check of ``mesh.extract_mesh``'s ``thresh`` that DESIGN 3.14 left open
(``python -m pixtrack_amd.mesh ... --check_render N``).
"""
from __future__ import annotations

import argparse
import json
import math
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from .evaluation import _poses_4x4
from .mesh_render import VIEW, MeshRenderer, icosphere, ngp_view_record, read_mesh, view_record
from .render_evaluation import (CHUNK_BYTES, MAX_PAIRS_PER_CALL, RECORD, _require_device, _thresholds, frame_figures,
                                summarize)
from .sensor_evaluation import (DEFAULT_DELTA, DEFAULT_MIN_VISIB_FRACT, _camera_key, _lookup, sensor_file_name,
                                sensor_frame_figures, summarize_sensor)
from .sensor_evaluation import RECORD as SENSOR_RECORD

MAX_VIEWS_PER_CALL = 4096             # pxt_mesh_raster's bound on P
MIN_ALPHA = 0.5                       # the rasteriser's alpha is 0 or 1: any value in (0, 1] says the same
DEFAULT_NEAR = 1e-6                   # a triangle with a vertex at or behind this camera-axis depth is dropped whole


def mesh_ray_factors(camera) -> np.ndarray:
    """float32 ``[H, W]``: ``sqrt(1 + xn^2 + yn^2)`` of every pixel under the camera's own intrinsics in the Camera
    convention (pixel centres at integer coordinates): ``xn = (i - cx) / fx``, ``yn = (j - cy) / fy``.  Computed in
    float64 and rounded once.  Camera-axis depth times this is the length of the pixel's ray."""
    W, H = (int(x) for x in camera.size)
    fx, fy = (float(x) for x in camera.f)
    cx, cy = (float(x) for x in camera.c)
    xn = (np.arange(W, dtype=np.float64) - cx) / fx
    yn = (np.arange(H, dtype=np.float64) - cy) / fy
    return np.sqrt(1.0 + xn[None, :] ** 2 + yn[:, None] ** 2).astype(np.float32)


def _frames(camera, T_est, T_gt):
    A, B = _poses_4x4(T_est), _poses_4x4(T_gt)
    if A.shape != B.shape:
        raise ValueError(f"{A.shape[0]} estimated and {B.shape[0]} ground-truth poses")
    F = len(A)
    cams = list(camera) if isinstance(camera, (list, tuple)) else [camera] * F
    if len(cams) != F:
        raise ValueError(f"{len(cams)} cameras for {F} frames")
    usable = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2))
    return A, B, cams, usable, np.nonzero(usable)[0]


def _views(cams, T, part, near):
    import torch

    return torch.from_numpy(np.stack([view_record(cams[i], T[i], near, 1.0) for i in part]))


def mesh_pose_errors(renderer: MeshRenderer, camera, T_est, T_gt, diameter: float,
                     taus: Optional[Sequence[float]] = None, near: float = DEFAULT_NEAR) -> Dict[str, np.ndarray]:
    """``render_evaluation.render_pose_errors`` with the object's mesh in place of its NeRF: VSD, silhouette IoU and depth
    error of F (estimated, ground-truth) world-to-camera poses seen by ``camera`` (one Camera, or one per frame, all of
    one image size; each frame's own ``fx, fy, cx, cy`` are honoured; lens terms are refused).

    A chunk's estimated views and its ground-truth views are drawn in two ``mesh_raster`` calls into two
    ``[chunk, H, W, 4]`` device buffers that stay under 256 MB together, and compared in one ``depth_agreement`` call;
    the records are downloaded once at the end.  Same returns as ``render_pose_errors``; ``diameter``, ``taus`` and the
    depth figures are in the mesh's units."""
    import torch

    from . import _lib
    from .ops import ops

    dev = _require_device(renderer.device)
    A, B, cams, usable, idx = _frames(camera, T_est, T_gt)
    taus, tq = _thresholds(diameter, taus, 1.0)
    rec = np.zeros((len(A), RECORD), np.uint32)
    if len(idx):
        sizes = {tuple(int(x) for x in cams[i].size) for i in idx}
        if len(sizes) != 1:
            raise ValueError(f"the frames of one call share one image size (got {sorted(sizes)})")
        (W, H), = sizes
        chunk = int(max(1, min(len(idx), MAX_PAIRS_PER_CALL, MAX_VIEWS_PER_CALL, CHUNK_BYTES // (2 * H * W * 16))))
        buf_e = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        buf_g = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        records = torch.zeros(len(idx), RECORD, dtype=torch.int32, device=dev)
        need = int(_lib.lib().pxt_depth_agreement_workspace_bytes(chunk, W, H))
        if need <= 0:
            raise ValueError(f"{W} x {H} images are not supported (1..2^28 pixels)")
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        for s in range(0, len(idx), chunk):
            part = idx[s:s + chunk]
            n = len(part)
            renderer.render_depth(_views(cams, A, part, near), W, H, out=buf_e[:n], download_records=False)
            renderer.render_depth(_views(cams, B, part, near), W, H, out=buf_g[:n], download_records=False)
            ops.depth_agreement(buf_e[:n], buf_g[:n], MIN_ALPHA, tq, records[s:s + n], workspace)
        rec[idx] = records.cpu().numpy().view(np.uint32)
    out = frame_figures(rec, 1.0, n_taus=len(taus), finite_slot=len(taus))
    out["ok"] = out["ok"] & usable
    out["taus"] = np.asarray(taus, np.float64)
    return out


def mesh_sensor_pose_errors(renderer: MeshRenderer, camera, T_est, T_gt, sensor_images, sensor_depth_scale: float,
                            diameter: float, delta: float = DEFAULT_DELTA, taus: Optional[Sequence[float]] = None,
                            near: float = DEFAULT_NEAR) -> Dict[str, np.ndarray]:
    """``sensor_evaluation.sensor_pose_errors`` with the object's mesh in place of its NeRF: BOP's sensor-depth VSD and the
    visible fraction against ``sensor_images`` (F uint16 ``[H, W]`` arrays of raw counts, 0 = no measurement;
    ``sensor_depth_scale``: mesh units per count).  The frames of one call share one camera; the sensor image is read
    where it is (shift 0: the rasteriser honours the intrinsics) and the ray factor is ``mesh_ray_factors``.  Same
    returns as ``sensor_pose_errors`` (``shift`` (0, 0), ``residual_px`` 0)."""
    import torch

    from . import _lib
    from .ops import ops

    dev = _require_device(renderer.device)
    A, B, cams, usable, idx = _frames(camera, T_est, T_gt)
    if len(sensor_images) != len(A):
        raise ValueError(f"{len(sensor_images)} sensor images for {len(A)} frames")
    taus, tq = _thresholds(diameter, taus, 1.0)
    delta_q, sensor_q = float(np.float32(float(delta))), float(np.float32(float(sensor_depth_scale)))
    rec = np.zeros((len(A), SENSOR_RECORD), np.uint32)
    if len(idx):
        if len({_camera_key(cams[i]) for i in idx}) != 1:
            raise ValueError("the frames of one call share one camera (size, focal lengths, principal point)")
        cam = cams[idx[0]]
        W, H = (int(x) for x in cam.size)
        ray = torch.from_numpy(mesh_ray_factors(cam)).to(dev)
        chunk = int(max(1, min(len(idx), MAX_PAIRS_PER_CALL, MAX_VIEWS_PER_CALL, CHUNK_BYTES // (H * W * (2 * 16 + 2)))))
        buf_e = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        buf_g = torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev)
        records = torch.zeros(len(idx), SENSOR_RECORD, dtype=torch.int32, device=dev)
        need = int(_lib.lib().pxt_sensor_vsd_workspace_bytes(chunk, W, H))
        if need <= 0:
            raise ValueError(f"{W} x {H} images are not supported (1..2^28 pixels)")
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        for s in range(0, len(idx), chunk):
            part = idx[s:s + chunk]
            n = len(part)
            host = np.empty((n, H, W), np.uint16)
            for j, i in enumerate(part):
                img = np.asarray(sensor_images[i])
                if img.dtype != np.uint16 or img.shape != (H, W):
                    raise ValueError(f"sensor image {i}: expected uint16 [{H}, {W}] (got {img.dtype} {img.shape})")
                host[j] = img
            renderer.render_depth(_views(cams, A, part, near), W, H, out=buf_e[:n], download_records=False)
            renderer.render_depth(_views(cams, B, part, near), W, H, out=buf_g[:n], download_records=False)
            sensor = torch.from_numpy(host.view(np.int16)).to(dev)
            ops.sensor_vsd(buf_e[:n], buf_g[:n], sensor, ray, [0, 0], MIN_ALPHA, sensor_q, delta_q, tq, records[s:s + n],
                           workspace)
        rec[idx] = records.cpu().numpy().view(np.uint32)
    out = sensor_frame_figures(rec, 1.0, n_taus=len(taus), finite_slot=len(taus))
    out["ok"] = out["ok"] & usable
    out["taus"] = np.asarray(taus, np.float64)
    out["shift"] = (0, 0)
    out["residual_px"] = 0.0
    return out


def _scored(poses_file, names):
    return [bool(poses_file[k].get("success")) and poses_file[k].get("gt_pose") is not None
            and poses_file[k].get("T_refined") is not None and poses_file[k].get("camera") is not None for k in names]


def evaluate_poses_mesh(poses_file: Dict, renderer: MeshRenderer, diameter: float,
                        taus: Optional[Sequence[float]] = None, near: float = DEFAULT_NEAR) -> Dict:
    """``render_evaluation.evaluate_poses_rendered`` over mesh renders: the same frame selection (``success``, ``gt_pose``,
    ``T_refined`` and ``camera`` present, both poses finite; consecutive frames of one image size share a call), the same
    miss rule (``vsd = 1`` at every tau, ``iou = 0``; a miss counts in ``ar_vsd`` and is left out of the means) and the
    same keys."""
    names = list(poses_file)
    usable = _scored(poses_file, names)
    n = len(names)
    taus_used, _ = _thresholds(diameter, taus, 1.0)
    K = len(taus_used)
    vsd, iou = np.ones((n, K)), np.zeros(n)
    cols = {k: np.zeros(n, np.int64) for k in ("n_est", "n_gt")}
    dz = {k: np.full(n, np.nan) for k in ("mean_abs_dz", "max_abs_dz")}
    ok = np.zeros(n, bool)
    idx = [i for i, u in enumerate(usable) if u]
    size_of = {i: tuple(int(x) for x in poses_file[names[i]]["camera"].size) for i in idx}
    s = 0
    while s < len(idx):  # runs of consecutive usable frames of one image size
        e = s + 1
        while e < len(idx) and size_of[idx[e]] == size_of[idx[s]]:
            e += 1
        run = idx[s:e]
        res = mesh_pose_errors(renderer, [poses_file[names[i]]["camera"] for i in run],
                               [_poses_4x4([poses_file[names[i]]["T_refined"]])[0] for i in run],
                               [_poses_4x4([poses_file[names[i]]["gt_pose"]])[0] for i in run], diameter, taus=taus_used,
                               near=near)
        vsd[run], iou[run], ok[run] = res["vsd"], res["iou"], res["ok"]
        for k in cols:
            cols[k][run] = res[k]
        for k in dz:
            dz[k][run] = res[k]
        s = e
    out = {"frames": {name: dict(vsd=[float(x) for x in vsd[i]], iou=float(iou[i]), n_est=int(cols["n_est"][i]),
                                 n_gt=int(cols["n_gt"][i]), mean_abs_dz=float(dz["mean_abs_dz"][i]),
                                 max_abs_dz=float(dz["max_abs_dz"][i]), ok=bool(ok[i])) for i, name in enumerate(names)}}
    out["n_frames"] = n
    out["n_success"] = int(sum(bool(poses_file[k].get("success")) for k in names))
    if any("tracked" in poses_file[k] for k in names):
        out["n_tracked"] = int(sum(bool(poses_file[k].get("tracked")) for k in names))
    out.update(summarize(vsd, iou, dz["mean_abs_dz"], ok))
    out["taus"] = [float(t) for t in taus_used]
    out["diameter"] = float(diameter)
    return out


def evaluate_poses_mesh_sensor(poses_file: Dict, renderer: MeshRenderer, diameter: float, sensor_lookup,
                               sensor_depth_scale: float, delta: float = DEFAULT_DELTA,
                               taus: Optional[Sequence[float]] = None,
                               min_visib_fract: float = DEFAULT_MIN_VISIB_FRACT, near: float = DEFAULT_NEAR) -> Dict:
    """``sensor_evaluation.evaluate_poses_sensor`` over mesh renders: the same scored frames, the visible fraction for
    every frame with ``gt_pose``, ``camera`` and a sensor image (a lost frame is drawn at its ground-truth pose alone for
    that), BOP's visibility cut, and the same keys (``sensor_shift`` [0, 0], ``sensor_residual_px`` 0)."""
    names = list(poses_file)
    n = len(names)
    taus_used, _ = _thresholds(diameter, taus, 1.0)
    K = len(taus_used)
    scored = _scored(poses_file, names)
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
    s = 0
    while s < len(idx):  # runs of consecutive frames of one camera
        e = s + 1
        while e < len(idx) and key_of[idx[e]] == key_of[idx[s]]:
            e += 1
        run = idx[s:e]
        T_gt = [_poses_4x4([poses_file[names[i]]["gt_pose"]])[0] for i in run]
        T_est = [_poses_4x4([poses_file[names[i]]["T_refined"]])[0] if scored[i] else T_gt[j] for j, i in enumerate(run)]
        res = mesh_sensor_pose_errors(renderer, [poses_file[names[i]]["camera"] for i in run], T_est, T_gt,
                                      [images[i] for i in run], sensor_depth_scale, diameter, delta=delta, taus=taus_used,
                                      near=near)
        sc = np.array([scored[i] for i in run], bool) & res["ok"]
        vsd[run] = np.where(sc[:, None], res["vsd"], 1.0)
        ok[run], known[run] = sc, res["ok"]
        visib[run] = np.where(res["ok"], res["visib_fract"], np.nan)
        for k in cols:
            cols[k][run] = res[k]
        for k in dd:
            dd[k][run] = np.where(sc, res[k], np.nan)
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
    out["sensor_shift"] = [0, 0]
    out["sensor_residual_px"] = 0.0
    return out


# ------------------------------------------------------------------------------------------------------------------
# The extracted mesh against the NeRF it came from.
# ------------------------------------------------------------------------------------------------------------------
def look_at_cameras(centre, distance: float, n_views: int) -> np.ndarray:
    """``[n_views, 3, 4]`` camera-to-world matrices in the renderer's convention (columns: image right, image down,
    forward, position) that look at ``centre`` from the directions of an icosphere's first vertices."""
    sub = 0
    while len(icosphere(sub)[0]) < n_views:
        sub += 1
    dirs = icosphere(sub)[0][:n_views]
    centre = np.asarray(centre, np.float64)
    out = np.empty((n_views, 3, 4))
    for k, d in enumerate(dirs):
        fwd = -d / np.linalg.norm(d)
        up = np.eye(3)[int(np.argmin(np.abs(fwd)))]  # the world axis the view direction is least along
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        out[k] = np.stack([right, down, fwd, centre + distance * d], axis=1)
    return out


def _turned(C, centre, degrees: float) -> np.ndarray:
    """The camera ``C`` turned about the axis through ``centre`` along its image-down direction."""
    a = math.radians(degrees)
    k = C[:, 1]
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rot = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    return np.concatenate([Rot @ C[:, :3], (centre + Rot @ (C[:, 3] - centre))[:, None]], axis=1)


def mesh_nerf_agreement(testbed, V, F, n_views: int = 12, width: int = 160, height: int = 120, spp: int = 8,
                        min_alpha: float = 0.5, fov: float = 40.0, turn_mesh_view_deg: float = 0.0,
                        near: float = DEFAULT_NEAR) -> Dict:
    """A mesh in the ``ngp`` frame against the NeRF it was extracted from: from ``n_views`` look-at views around the
    render box (icosphere directions, the box's circumsphere filling the narrower side of the image), the NeRF's Depth
    render (``spp`` samples, silhouette ``alpha >= min_alpha``) and the rasteriser's image of the mesh through
    ``ngp_view_record`` with ``depth_q`` = the model's depth scale go through ``pxt_depth_agreement``.

    Returns ``iou`` and ``mean_abs_dz`` (ngp units; NaN without an overlap) per view, their means ``iou_mean`` /
    ``mean_abs_dz_mean``, ``n_nerf`` / ``n_mesh`` (silhouette pixels) and ``n_views``.  ``turn_mesh_view_deg`` draws the
    mesh from views turned about the box centre by that angle: a wrong answer on purpose, to see the figures move."""
    import torch

    from . import _lib
    from .ngp import RenderMode
    from .ops import ops

    dev = _require_device(testbed.device)
    n_views, W, H = int(n_views), int(width), int(height)
    if not (1 <= n_views <= MAX_VIEWS_PER_CALL):
        raise ValueError(f"{n_views} views (1..{MAX_VIEWS_PER_CALL})")
    lo, hi = np.asarray(testbed.render_aabb.min, np.float64), np.asarray(testbed.render_aabb.max, np.float64)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    depth_scale = 1.0 / float(testbed._snap.scale)
    renderer = MeshRenderer(V, F, dev)
    nerf = torch.empty(n_views, H, W, 4, dtype=torch.float32, device=dev)
    keep = (testbed.fov, testbed._cam_ngp)
    views = np.empty((n_views, VIEW), np.float32)
    try:
        testbed.fov = float(fov)
        testbed._check_renderable()
        focal = float(testbed._view_for(W, H)[12])
        distance = 1.05 * radius / math.sin(math.atan(0.5 * min(W, H) / focal))
        cams = look_at_cameras(centre, distance, n_views)
        for k, C in enumerate(cams):
            testbed._cam_ngp = C
            view = testbed._view_for(W, H)
            ops.ngp_render(testbed._ctx_int(), view, W, H, int(spp), int(RenderMode.Depth), nerf[k], testbed.stats_accum)
            testbed.n_renders += 1
            Cf = np.asarray(view[:12], np.float64).reshape(3, 4)  # the float32 camera the renderer used
            views[k] = ngp_view_record(_turned(Cf, centre, turn_mesh_view_deg) if turn_mesh_view_deg else Cf, focal, W, H,
                                       near, depth_scale)
    finally:
        testbed.fov, testbed._cam_ngp = keep
    mesh_img, _, _ = renderer.render_depth(views, W, H, download_records=False)
    records = torch.zeros(n_views, RECORD, dtype=torch.int32, device=dev)
    need = int(_lib.lib().pxt_depth_agreement_workspace_bytes(n_views, W, H))
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ops.depth_agreement(mesh_img, nerf, float(min_alpha), [math.inf], records, workspace)
    fig = frame_figures(records.cpu().numpy().view(np.uint32), 1.0 / depth_scale, n_taus=0, finite_slot=0)
    dz = fig["mean_abs_dz"]
    return {"iou": fig["iou"], "mean_abs_dz": dz, "n_mesh": fig["n_est"], "n_nerf": fig["n_gt"], "n_views": n_views,
            "iou_mean": float(fig["iou"].mean()),
            "mean_abs_dz_mean": float(np.nanmean(dz)) if np.isfinite(dz).any() else float("nan")}


# ------------------------------------------------------------------------------------------------------------------
# Command line.
# ------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .evaluation import add_bop_arguments

    ap = argparse.ArgumentParser(prog="python -m pixtrack_amd.mesh_evaluation",
                                 description="VSD, silhouette IoU and depth error of a poses.pkl from depth renders of the "
                                             "object's mesh (no NeRF snapshot); with sensor depth images, BOP's VSD as published")
    ap.add_argument("--poses", required=True, help="poses.pkl of a run (frames need gt_pose and camera)")
    ap.add_argument("--mesh", required=True, help="the object's mesh in the poses' object frame: .obj or .ply")
    ap.add_argument("--mesh_scale", type=float, default=1.0, help="factor from the mesh file's units to the poses' units")
    ap.add_argument("--diameter", type=float, default=None,
                    help="object diameter in the poses' units (default: --models_info's, else the mesh's largest vertex distance)")
    ap.add_argument("--json", default=None, help="write the summary and the per-frame figures to this file")
    ap.add_argument("--device", default="cuda:0")
    add_bop_arguments(ap)
    ap.add_argument("--sensor_depth_dir", default=None, help="directory of the frames' 16-bit depth images: adds the sensor-depth VSD")
    ap.add_argument("--sensor_depth_template", default="{stem}.png",
                    help="file name of a frame's depth image; {stem}: the frame name without extension, {name}: as it is")
    ap.add_argument("--sensor_depth_sub", nargs=2, metavar=("OLD", "NEW"), default=None,
                    help="replace OLD by NEW in the stem first (YCB-Video: color depth)")
    ap.add_argument("--sensor_depth_scale", type=float, default=None, help="the poses' units per raw count of the depth images")
    ap.add_argument("--delta", type=float, default=DEFAULT_DELTA, help="visibility tolerance in the poses' units (BOP: 15 mm)")
    ap.add_argument("--min_visib_fract", type=float, default=DEFAULT_MIN_VISIB_FRACT,
                    help="a frame with a smaller visible fraction is left out of ar_vsd_sensor (BOP: 0.1)")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    ap = build_parser()
    args = ap.parse_args(argv)
    _require_device(args.device)
    if args.sensor_depth_dir and args.sensor_depth_scale is None:
        ap.error("--sensor_depth_dir needs --sensor_depth_scale")
    from .evaluation import bop_symmetries, evaluate_poses_bop, merge_bop
    from .utils.io import load_reference_pickle

    V, F = read_mesh(args.mesh)
    V = V * float(args.mesh_scale)
    poses = load_reference_pickle(args.poses)
    renderer = MeshRenderer(V, F, args.device)
    diameter = args.diameter
    if diameter is None and args.models_info:
        from .symmetry import read_models_info

        diameter = read_models_info(args.models_info, args.obj_id).get("diameter")
        diameter = None if diameter is None else float(diameter) * float(args.models_info_scale)
    if diameter is None:
        from .mesh import max_pairwise_distance

        diameter = max_pairwise_distance(renderer.vertices)[0]
    res = evaluate_poses_mesh(poses, renderer, float(diameter))
    if args.sensor_depth_dir:
        def lookup(name):
            p = Path(args.sensor_depth_dir) / sensor_file_name(name, args.sensor_depth_template, args.sensor_depth_sub)
            return str(p) if p.exists() else None

        merge_bop(res, evaluate_poses_mesh_sensor(poses, renderer, float(diameter), lookup, args.sensor_depth_scale,
                                                  delta=args.delta, min_visib_fract=args.min_visib_fract))
    if args.bop:  # MSSD / MSPD over the mesh's vertices
        merge_bop(res, evaluate_poses_bop(poses, V, args.device, float(diameter), symmetries=bop_symmetries(args),
                                          ar_vsd=res["ar_vsd"]))
        if args.sensor_depth_dir:
            res["ar_bop_sensor"] = (res["ar_vsd_sensor"] + res["ar_mssd"] + res["ar_mspd"]) / 3.0
    summary = {k: v for k, v in res.items() if k != "frames"}
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f)
    return res


if __name__ == "__main__":
    main()
