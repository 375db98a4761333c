"""Trajectory metrics of the reference's evaluation notebook (reference
notebooks/GetMetrics.ipynb: ``similarity_transform``, ``get_pose_offset``, ``get_metrics``).

The notebook aligns the estimated camera-translation track to the ground-truth one with a
similarity (Umeyama) fit, then reports per-frame mean vertex distance (the ADD figure it
calls ``average_error_vertices``), translation error in cm, and the share of frames inside a
(cm, degree) threshold.  Host-side numpy on a few hundred 4x4 matrices: not hot-path work.

Below those, the scoreboard of a whole run on the device (``pose_errors``, ``evaluate_poses`` and the command line
``python -m pixtrack_amd.evaluation``): ADD and ADD-S of every frame in one call of ``torch.ops.pixtrack.pose_errors``
(csrc/pxt_eval.hip: F * V^2 distance evaluations), accuracy under a threshold and the area under that curve.  That part
has no CPU path: ``get_metrics`` / ``adds_distance`` remain the host functions.

Below that, BOP's symmetry-aware errors (``symmetric_pose_errors``, ``evaluate_poses_bop``, ``--bop`` on the command
line): MSSD and MSPD of every frame over the object's symmetry set (``symmetry.py``) in calls of
``torch.ops.pixtrack.symmetric_pose_errors`` (csrc/pxt_eval_sym.hip: F * S * V point pairs), their average recalls and,
given ``ar_vsd`` (``render_evaluation``), BOP's headline ``AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3``.  Device only as well.
"""
from __future__ import annotations

import argparse
import json
from typing import Dict, Optional, Sequence

import numpy as np

from .utils.pose_utils import geodesic_distance_for_rotations


def get_pose_mat_from_tensor(pose) -> np.ndarray:
    """Pose -> 4x4 (notebook cell ``get_pose_mat_from_tensor``)."""
    T = np.eye(4)
    T[:3, :3] = pose.R.cpu().numpy()
    T[:3, 3] = pose.t.cpu().numpy()
    return T


def similarity_transform(from_points: np.ndarray, to_points: np.ndarray):
    """Least-squares (R, c, t) with ``to ~ c R from + t`` (Umeyama 1991, as in the notebook,
    including its reflection rule and the collinearity error)."""
    assert from_points.ndim == 2, "from_points must be a m x n array"
    assert from_points.shape == to_points.shape, "from_points and to_points must have the same shape"
    N, m = from_points.shape
    mean_from, mean_to = from_points.mean(axis=0), to_points.mean(axis=0)
    d_from, d_to = from_points - mean_from, to_points - mean_to
    sigma_from = (d_from * d_from).sum(axis=1).mean()
    cov = d_to.T.dot(d_from) / N
    U, d, Vt = np.linalg.svd(cov, full_matrices=True)
    rank = np.linalg.matrix_rank(cov)
    S = np.eye(m)
    if rank >= m - 1 and np.linalg.det(cov) < 0:
        S[m - 1, m - 1] = -1
    elif rank < m - 1:
        raise ValueError("colinearility detected in covariance matrix:\n{}".format(cov))
    R = U.dot(S).dot(Vt)
    c = (d * S.diagonal()).sum() / sigma_from
    t = mean_to - c * R.dot(mean_from)
    return R, c, t


def get_pose_offset(poses_file: Dict) -> np.ndarray:
    """4x4 rigid part (scale dropped, as the notebook does) of the similarity that maps the
    ground-truth translations onto the refined ones, over successful frames."""
    from_trs, to_trs = [], []
    for key in poses_file:
        if not poses_file[key]["success"]:
            continue
        to_trs.append(poses_file[key]["T_refined"].t.cpu().numpy())
        from_trs.append(poses_file[key]["gt_pose"].t.cpu().numpy())
    R, _, t = similarity_transform(np.array(from_trs, dtype=np.float64), np.array(to_trs, dtype=np.float64))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def get_metrics(poses_file: Dict, vertices: np.ndarray, tr_threshold: float, rot_threshold: float) -> Dict:
    """``vertices``: [V, 4] homogeneous model points in the object frame (the notebook's global
    of that name).  Distances in cm (x100), rotations in degrees; a frame is bad when either
    exceeds its threshold.  Frames with ``success == False`` are skipped, so - as in the
    notebook - they stay in ``total_frames`` but are never counted bad."""
    offset = get_pose_offset(poses_file)
    distances, pose_dists, bad = [], [], 0
    for key in poses_file:
        if not poses_file[key]["success"]:
            continue
        res = get_pose_mat_from_tensor(poses_file[key]["T_refined"])
        gt = get_pose_mat_from_tensor(poses_file[key]["gt_pose"])
        aligned = offset @ res
        tr = np.linalg.norm(gt[:3, 3] - aligned[:3, 3]) * 100
        rot = geodesic_distance_for_rotations(gt[:3, :3], aligned[:3, :3]) * 180 / np.pi
        res_v = (offset @ (res @ vertices.T)).T[:, :3] * 100
        gt_v = (gt @ vertices.T).T[:, :3] * 100
        distances.append(np.mean(np.linalg.norm(gt_v - res_v, axis=1)))
        pose_dists.append(tr)
        if tr > tr_threshold or rot > rot_threshold:
            bad += 1
    n = len(poses_file)
    return {
        "average_error_vertices": float(np.mean(distances)),
        "max_error": float(np.max(distances)),
        "max_translation_error": float(np.max(pose_dists)),
        "average_translation_error_pose": float(np.mean(pose_dists)),
        "bad_count": bad,
        "total_frames": n,
        "accuracy": (1.0 * (n - bad)) / (1.0 * n),
    }


def adds_distance(T_est: np.ndarray, T_gt: np.ndarray, vertices: np.ndarray) -> float:
    """ADD-S (symmetric average closest-point distance, Xiang et al. 2018) between the model
    under two 4x4 poses; ``vertices`` [V, 3|4].  BASELINE config 3 reports it against the
    synthetic ground truth.  O(V^2) in blocks: V is a few thousand."""
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    a = v @ T_est[:3, :3].T + T_est[:3, 3]
    b = v @ T_gt[:3, :3].T + T_gt[:3, 3]
    best = np.empty(len(b))
    for s in range(0, len(b), 1024):
        d = np.linalg.norm(b[s:s + 1024, None, :] - a[None, :, :], axis=-1)
        best[s:s + 1024] = d.min(axis=1)
    return float(best.mean())


# ------------------------------------------------------------------------------------------------------------------
# A whole run on the device: ADD / ADD-S per frame (torch.ops.pixtrack.pose_errors), AUC, accuracy, command line.
# ------------------------------------------------------------------------------------------------------------------
MAX_FRAMES_PER_CALL = 65535  # pxt_pose_errors' bound on F (one grid row per frame)


def _poses_4x4(T) -> np.ndarray:
    """[F, 4, 4] float64 from an array, a list of 4x4 matrices or a list of Pose objects."""
    if isinstance(T, (list, tuple)):
        T = [get_pose_mat_from_tensor(x) if hasattr(x, "R") else np.asarray(x, dtype=np.float64) for x in T]
    T = np.asarray(T, dtype=np.float64)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError(f"poses must be [F, 4, 4] (got {T.shape})")
    return T


def relative_poses(T_est, T_gt, centroid, dtype=np.float32) -> np.ndarray:
    """float32 [F, 12] (R row-major, then t) of ``T_rel = T_gt^-1 T_est`` re-expressed for vertices with ``centroid``
    subtracted: with ``u = v - c``, ``T_rel v - v = R u + t' - u`` where ``t' = R c + t - c``.  ``T_gt`` is taken to be
    rigid (its inverse is ``[R^T | -R^T t]``).  Everything in float64, rounded once (``dtype=np.float64``: not at all);
    a frame whose two matrices are the same bits gives R = I, t' = 0 exactly (``R_gt^T R_gt`` alone would be I only to
    rounding)."""
    A, B = _poses_4x4(T_est), _poses_4x4(T_gt)
    if A.shape != B.shape:
        raise ValueError(f"{A.shape[0]} estimated and {B.shape[0]} ground-truth poses")
    c = np.asarray(centroid, dtype=np.float64).reshape(3)
    RgT = np.transpose(B[:, :3, :3], (0, 2, 1))
    R = RgT @ A[:, :3, :3]
    t = np.einsum("fij,fj->fi", RgT, A[:, :3, 3] - B[:, :3, 3])
    tc = np.einsum("fij,j->fi", R, c) + t - c
    same = np.all(A == B, axis=(1, 2))
    R[same], tc[same] = np.eye(3), 0.0
    return np.concatenate([R.reshape(-1, 9), tc], axis=1).astype(dtype)


def _require_device(device):
    import torch

    from . import _lib

    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PxtError(f"pose-error evaluation runs on a ROCm device (got {dev}); no CPU path exists - "
                            "get_metrics / adds_distance are the host functions")
    return dev


def pose_errors(T_est, T_gt, vertices, device, adds: bool = True) -> Dict[str, np.ndarray]:
    """ADD and ADD-S of F frames: ``add`` = mean_i |T_est v_i - T_gt v_i|, ``add_max`` its max over i, ``adds`` =
    mean_i min_j |T_est v_j - T_gt v_i| (``adds_distance``'s direction), ``adds_max``, and ``ok`` (False where a pose
    holds a non-finite value; that frame's distances are NaN).  ``vertices`` [V, 3|4] are centred in float64 and uploaded
    once; the frames go through ``torch.ops.pixtrack.pose_errors`` in chunks of at most 65535, one download at the end.
    ``adds=False`` skips the O(V^2) part (``adds`` / ``adds_max`` come back NaN)."""
    import torch

    from . import ops as _ops

    dev = _require_device(device)
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] not in (3, 4) or len(v) < 1:
        raise ValueError(f"vertices must be [V >= 1, 3|4] (got {v.shape})")
    v = v[:, :3]
    c = v.mean(axis=0)
    rel = relative_poses(T_est, T_gt, c)
    F, V = len(rel), len(v)
    nan = np.full(F, np.nan)
    if F == 0:
        return dict(add=nan, add_max=nan.copy(), adds=nan.copy(), adds_max=nan.copy(), ok=np.zeros(0, bool))
    verts = torch.from_numpy((v - c).astype(np.float32)).to(dev)
    poses = torch.from_numpy(rel).to(dev)
    records = torch.full((F, 8), float("nan"), dtype=torch.float32, device=dev)
    need = int(_ops._lib.lib().pxt_pose_errors_workspace_bytes(min(F, MAX_FRAMES_PER_CALL), V))
    if need <= 0:
        raise _ops._lib.PxtError(f"pose_errors: {V} vertices are not supported (1..2^20)")
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    for s in range(0, F, MAX_FRAMES_PER_CALL):
        e = min(F, s + MAX_FRAMES_PER_CALL)
        _ops.ops.pose_errors(verts, poses[s:e], bool(adds), records[s:e], workspace)
    rec = records.cpu().numpy().astype(np.float64)
    out = dict(add=rec[:, 0], add_max=rec[:, 1], adds=rec[:, 2], adds_max=rec[:, 3], ok=rec[:, 7] == 1.0)
    if not adds:
        out["adds"], out["adds_max"] = nan, nan.copy()
    return out


def _distances(distances) -> np.ndarray:
    d = np.array([np.nan if x is None else x for x in np.asarray(distances, dtype=object).reshape(-1)], dtype=np.float64)
    return np.where(np.isfinite(d), d, np.inf)


def auc(distances, max_distance: float) -> float:
    """Area under the accuracy-threshold curve on [0, max_distance], normalised to [0, 1]: with acc(x) the share of
    frames whose distance is <= x, ``(1 / max) * integral_0^max acc(x) dx = mean_k max(0, 1 - d_k / max)``.  A
    non-finite or missing (None) distance counts as inf and contributes 0.  This is the EXACT area of the step curve,
    not PoseCNN's ``VOCap`` (which integrates an interpolated, monotone envelope of sampled thresholds and comes out
    slightly different).  No distances: NaN."""
    d = _distances(distances)
    if d.size == 0:
        return float("nan")
    return float(np.mean(np.maximum(0.0, 1.0 - d / float(max_distance))))


def accuracy_under(distances, threshold: float) -> float:
    """Share of frames whose distance is below ``threshold`` (non-finite / missing: never below).  No distances: NaN."""
    d = _distances(distances)
    if d.size == 0:
        return float("nan")
    return float(np.mean(d < float(threshold)))


def evaluate_poses(poses_file: Dict, vertices, device, symmetric: bool = False, max_distance: float = 0.1,
                   threshold: Optional[float] = None, offset: bool = False) -> Dict:
    """The scoreboard of a run: ``poses_file`` is a ``poses.pkl``-style dict (frame name -> ``T_refined``, ``gt_pose``,
    ``success`` and, where present, ``tracked``), ``vertices`` [V, 3|4] the model points in the object frame.

    Returns ``frames`` (frame name -> ``add``, ``add_max``, ``adds``, ``adds_max``, ``ok``) and, beside it, the summary:
    ``n_frames``, ``n_success`` (``n_tracked`` where the run has that key), ``n_evaluated``, ``add_mean``, ``adds_mean``,
    ``auc_add``, ``auc_adds``, ``auc_add_s`` (the "ADD(-S)" column: ADD-S when ``symmetric``, else ADD), ``max_distance``
    and, when ``threshold`` is given, ``acc_add``, ``acc_adds``, ``acc_add_s`` at it.

    A frame with ``success == False``, without a ``gt_pose`` or with a non-finite pose has distance inf: it counts
    against AUC and accuracy and is left out of the means.  (The notebook's ``get_metrics`` SKIPS failed frames: they
    stay in its ``total_frames`` but are never bad.  A lost frame is a miss here.)

    ``offset=True`` first aligns the estimates with ``get_pose_offset``'s similarity (the notebook's convention), so
    that ``add_mean * 100`` is ``get_metrics(...)["average_error_vertices"]``."""
    _require_device(device)
    names = list(poses_file)
    usable = [bool(poses_file[k].get("success")) and poses_file[k].get("gt_pose") is not None
              and poses_file[k].get("T_refined") is not None for k in names]
    T_est = [_poses_4x4([poses_file[k]["T_refined"]])[0] for k, u in zip(names, usable) if u]
    T_gt = [_poses_4x4([poses_file[k]["gt_pose"]])[0] for k, u in zip(names, usable) if u]
    if offset and T_est:
        off = get_pose_offset(poses_file)
        T_est = [off @ T for T in T_est]
    n = len(names)
    cols = {k: np.full(n, np.inf) for k in ("add", "add_max", "adds", "adds_max")}
    ok = np.zeros(n, bool)
    if T_est:
        res = pose_errors(np.stack(T_est), np.stack(T_gt), vertices, device, adds=True)
        idx = np.nonzero(usable)[0]
        ok[idx] = res["ok"]
        for k in cols:
            cols[k][idx] = np.where(res["ok"], res[k], np.inf)
    out = {"frames": {name: dict({k: float(cols[k][i]) for k in cols}, ok=bool(ok[i])) for i, name in enumerate(names)}}
    out["n_frames"] = n
    out["n_success"] = int(sum(bool(poses_file[k].get("success")) for k in names))
    if any("tracked" in poses_file[k] for k in names):
        out["n_tracked"] = int(sum(bool(poses_file[k].get("tracked")) for k in names))
    out["n_evaluated"] = int(ok.sum())
    out["add_mean"] = float(cols["add"][ok].mean()) if ok.any() else float("nan")
    out["adds_mean"] = float(cols["adds"][ok].mean()) if ok.any() else float("nan")
    out["max_distance"] = float(max_distance)
    out["symmetric"] = bool(symmetric)
    out["auc_add"], out["auc_adds"] = auc(cols["add"], max_distance), auc(cols["adds"], max_distance)
    out["auc_add_s"] = out["auc_adds"] if symmetric else out["auc_add"]
    if threshold is not None:
        out["threshold"] = float(threshold)
        out["acc_add"], out["acc_adds"] = accuracy_under(cols["add"], threshold), accuracy_under(cols["adds"], threshold)
        out["acc_add_s"] = out["acc_adds"] if symmetric else out["acc_add"]
    return out


# ------------------------------------------------------------------------------------------------------------------
# BOP's symmetry-aware errors: MSSD / MSPD per frame (torch.ops.pixtrack.symmetric_pose_errors), their average recalls.
# ------------------------------------------------------------------------------------------------------------------
BOP_THETAS = tuple(0.05 * k for k in range(1, 11))     # MSSD: correct when mssd < theta * diameter
BOP_THETAS_PX = tuple(5.0 * k for k in range(1, 11))   # MSPD: correct when mspd < theta * r pixels, r = width / 640
SYM_WORKSPACE_BYTES = 256 << 20                        # the frames of one call share a workspace of at most this size


def _intrinsics(cameras, F: int):
    """(``[F, 4]`` float64 fx, fy, cx, cy; ``[F]`` image widths or None) from a Camera, one Camera per frame, ``[4]`` or
    ``[F, 4]``.  A Camera's principal point is taken as stored (pixel centres at integers); MSPD is a difference of two
    projections, so the principal point cancels in it.  Lens terms are ignored: BOP projects with a pinhole."""
    def one(cam):
        data = cam._data.detach().cpu().numpy().astype(np.float64).reshape(-1)
        return data[2:6], data[0]

    if hasattr(cameras, "_data"):
        k, w = one(cameras)
        return np.tile(k, (F, 1)), np.full(F, w)
    if isinstance(cameras, (list, tuple)) and len(cameras) and hasattr(cameras[0], "_data"):
        if len(cameras) != F:
            raise ValueError(f"{len(cameras)} cameras for {F} frames")
        ks, ws = zip(*(one(c) for c in cameras))
        return np.stack(ks), np.array(ws, np.float64)
    K = np.asarray(cameras, dtype=np.float64)
    if K.shape == (4,):
        K = np.tile(K, (F, 1))
    if K.shape != (F, 4):
        raise ValueError(f"cameras must be a Camera, one per frame, [4] or [{F}, 4] intrinsics (got {K.shape})")
    return K, None


def symmetric_frames(T_est, T_gt, centroid, intrinsics, dtype=np.float32) -> np.ndarray:
    """float32 ``[F, 40]``, the per-frame input of pxt_symmetric_pose_errors: ``relative_poses`` (12), then the
    estimated and the ground-truth world-to-camera pose re-expressed for vertices with ``centroid`` subtracted
    (``T v = R u + t'`` with ``t' = R c + t``; 12 each), then fx, fy, cx, cy.  Everything in float64, rounded once."""
    A, B = _poses_4x4(T_est), _poses_4x4(T_gt)
    rel = relative_poses(A, B, centroid, dtype=np.float64)
    c = np.asarray(centroid, dtype=np.float64).reshape(3)
    K = np.asarray(intrinsics, dtype=np.float64).reshape(-1, 4)
    if len(K) != len(A):
        raise ValueError(f"{len(K)} intrinsics for {len(A)} frames")

    def centred(T):
        return np.concatenate([T[:, :3, :3].reshape(-1, 9), np.einsum("fij,j->fi", T[:, :3, :3], c) + T[:, :3, 3]], axis=1)

    return np.concatenate([rel, centred(A), centred(B), K], axis=1).astype(dtype)


def symmetric_pose_errors(T_est, T_gt, vertices, cameras, symmetries=None, device="cuda:0") -> Dict[str, np.ndarray]:
    """BOP's symmetry-aware errors of F frames: ``mssd`` = min_s max_i |T_est v_i - T_gt S_s v_i| (the units of the
    vertices), ``mspd`` = min_s max_i |pi(T_est v_i) - pi(T_gt S_s v_i)| (pixels; +inf when a point is not in front of
    the camera), ``mssd_sym`` / ``mspd_sym`` the index of the symmetry that gave each (-1 where not ok), and ``ok``
    (False where a pose or a camera holds a non-finite value; that frame's distances are NaN).

    ``vertices`` [V, 3|4]; ``cameras``: a Camera, one per frame, or ``[4]`` / ``[F, 4]`` fx, fy, cx, cy; ``symmetries``
    ``[S, 4, 4]`` in the units of the vertices (``symmetry.symmetry_transforms``), None: the identity only.  Vertices
    and set are centred in float64 and uploaded once with the frames; the frames go through
    ``torch.ops.pixtrack.symmetric_pose_errors`` in calls of at most 65535 (fewer when the workspace would pass 256 MB),
    one download at the end."""
    import torch

    from . import ops as _ops
    from .symmetry import centred_12, symmetry_transforms

    dev = _require_device(device)
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] not in (3, 4) or len(v) < 1:
        raise ValueError(f"vertices must be [V >= 1, 3|4] (got {v.shape})")
    v = v[:, :3]
    c = v.mean(axis=0)
    A = _poses_4x4(T_est)
    F, V = len(A), len(v)
    sym = symmetry_transforms() if symmetries is None else np.asarray(symmetries, dtype=np.float64).reshape(-1, 4, 4)
    S = len(sym)
    K, _ = _intrinsics(cameras, F)
    frames = symmetric_frames(A, T_gt, c, K)
    nan = np.full(F, np.nan)
    if F == 0:
        none = np.zeros(0, np.int64)
        return dict(mssd=nan, mspd=nan.copy(), mssd_sym=none, mspd_sym=none.copy(), ok=np.zeros(0, bool))
    L = _ops._lib.lib()
    per_frame = int(L.pxt_symmetric_pose_errors_workspace_bytes(1, S, V))
    if per_frame <= 0:
        raise _ops._lib.PxtError(f"symmetric_pose_errors: {S} symmetries x {V} vertices are not supported "
                                 "(1..1024 symmetries, 1..2^20 vertices)")
    step = int(max(1, min(F, MAX_FRAMES_PER_CALL, SYM_WORKSPACE_BYTES // per_frame)))
    verts = torch.from_numpy((v - c).astype(np.float32)).to(dev)
    syms = torch.from_numpy(centred_12(sym, c).astype(np.float32)).to(dev)
    frames_d = torch.from_numpy(frames).to(dev)
    records = torch.full((F, 8), float("nan"), dtype=torch.float32, device=dev)
    workspace = torch.empty(int(L.pxt_symmetric_pose_errors_workspace_bytes(step, S, V)), dtype=torch.uint8, device=dev)
    for s in range(0, F, step):
        e = min(F, s + step)
        _ops.ops.symmetric_pose_errors(verts, syms, frames_d[s:e], records[s:e], workspace)
    rec = records.cpu().numpy().astype(np.float64)
    ok = rec[:, 7] == 1.0
    which = np.where(ok[:, None], np.nan_to_num(rec[:, [1, 3]], nan=-1.0), -1.0).astype(np.int64)
    return dict(mssd=np.where(ok, rec[:, 0], np.nan), mspd=np.where(ok, rec[:, 2], np.nan), mssd_sym=which[:, 0],
                mspd_sym=which[:, 1], ok=ok)


def symmetric_pose_errors_host(T_est, T_gt, vertices, intrinsics, symmetries=None, chunk: int = 16):
    """The host function beside ``symmetric_pose_errors``: float64 numpy straight from BOP's definitions, in the
    camera frame (no relative form, no centring).  ``intrinsics`` ``[F, 4]`` or ``[4]``.  -> ``(e3, e2)``, each
    ``[F, S]``: the maximum over the vertices for every symmetry; MSSD and MSPD are their minima over the set.
    Symmetries are taken ``chunk`` at a time (a ``[chunk, V, 3]`` block).  Measured: 11.5 s per frame at V = 65536, S = 630."""
    from .symmetry import symmetry_transforms

    A, B = _poses_4x4(T_est), _poses_4x4(T_gt)
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    sym = symmetry_transforms() if symmetries is None else np.asarray(symmetries, dtype=np.float64).reshape(-1, 4, 4)
    K = np.broadcast_to(np.asarray(intrinsics, dtype=np.float64), (len(A), 4))

    def project(p, k):
        with np.errstate(all="ignore"):
            px = np.stack([k[0] * p[..., 0] / p[..., 2] + k[2], k[1] * p[..., 1] / p[..., 2] + k[3]], axis=-1)
        return px, (p[..., 2] > 0) & np.isfinite(p[..., 2])

    e3, e2 = np.empty((len(A), len(sym))), np.empty((len(A), len(sym)))
    for f in range(len(A)):
        a = v @ A[f, :3, :3].T + A[f, :3, 3]
        pa, oka = project(a, K[f])
        for s in range(0, len(sym), chunk):
            M = B[f][None] @ sym[s:s + chunk]
            g = np.einsum("sij,vj->svi", M[:, :3, :3], v) + M[:, None, :3, 3]
            e3[f, s:s + chunk] = np.linalg.norm(a[None] - g, axis=-1).max(axis=1)
            pg, okg = project(g, K[f])
            e2[f, s:s + chunk] = np.where(oka[None] & okg, np.linalg.norm(pa[None] - pg, axis=-1), np.inf).max(axis=1)
    return e3, e2


def recall_mssd(mssd, diameter: float, thetas: Sequence[float] = BOP_THETAS) -> float:
    """BOP's average recall of MSSD: the mean over frames x thetas of ``[mssd < theta * diameter]`` (strict; a
    non-finite or missing distance is a miss).  No frames: NaN."""
    d = _distances(mssd)
    if d.size == 0:
        return float("nan")
    return float(np.mean(d[:, None] < np.asarray(thetas, np.float64)[None, :] * float(diameter)))


def recall_mspd(mspd, widths, thetas_px: Sequence[float] = BOP_THETAS_PX) -> float:
    """BOP's average recall of MSPD: the mean over frames x thetas of ``[mspd < theta * r]`` with ``r = width / 640`` of
    the frame's image (``widths``: one number or one per frame), theta = 5 ... 50 px (strict; non-finite: a miss)."""
    d = _distances(mspd)
    if d.size == 0:
        return float("nan")
    r = np.broadcast_to(np.asarray(widths, np.float64), d.shape) / 640.0
    return float(np.mean(d[:, None] < np.asarray(thetas_px, np.float64)[None, :] * r[:, None]))


def evaluate_poses_bop(poses_file: Dict, vertices, device, diameter: float, symmetries=None, offset: bool = False,
                       ar_vsd: Optional[float] = None) -> Dict:
    """The BOP part of a run's scoreboard: ``poses_file`` as for ``evaluate_poses``, every record also holding the
    frame's ``camera``; ``diameter`` and ``symmetries`` ([S, 4, 4], None: identity only) in the units of ``vertices``.

    Returns ``frames`` (frame name -> ``mssd``, ``mspd``, ``mssd_sym``, ``mspd_sym``, ``ok``) and the summary:
    ``n_frames``, ``n_evaluated``, ``n_symmetries``, ``diameter``, ``mssd_mean``, ``mspd_mean`` (over the evaluated
    frames with a finite figure), ``ar_mssd`` (``recall_mssd``), ``ar_mspd`` (``recall_mspd`` with every frame's own
    image width) and, when ``ar_vsd`` is given, ``ar_vsd`` and ``ar_bop``, the mean of the three.

    Frame selection and misses are ``evaluate_poses``' (``success``, ``gt_pose``, ``T_refined``) plus ``camera``: any
    other frame, and a frame with a non-finite pose, has ``mssd = mspd = inf`` and is below no threshold."""
    _require_device(device)
    names = list(poses_file)
    usable = [bool(poses_file[k].get("success")) and poses_file[k].get("gt_pose") is not None
              and poses_file[k].get("T_refined") is not None and poses_file[k].get("camera") is not None for k in names]
    T_est = [_poses_4x4([poses_file[k]["T_refined"]])[0] for k, u in zip(names, usable) if u]
    T_gt = [_poses_4x4([poses_file[k]["gt_pose"]])[0] for k, u in zip(names, usable) if u]
    cams = [poses_file[k]["camera"] for k, u in zip(names, usable) if u]
    if offset and T_est:
        off = get_pose_offset(poses_file)
        T_est = [off @ T for T in T_est]
    n = len(names)
    cols = {k: np.full(n, np.inf) for k in ("mssd", "mspd")}
    which = {k: np.full(n, -1, np.int64) for k in ("mssd_sym", "mspd_sym")}
    ok = np.zeros(n, bool)
    widths = np.full(n, 640.0)
    n_syms = 1 if symmetries is None else len(np.asarray(symmetries).reshape(-1, 4, 4))
    if T_est:
        res = symmetric_pose_errors(np.stack(T_est), np.stack(T_gt), vertices, cams, symmetries, device)
        idx = np.nonzero(usable)[0]
        ok[idx] = res["ok"]
        widths[idx] = _intrinsics(cams, len(cams))[1]
        for k in cols:
            cols[k][idx] = np.where(res["ok"], res[k], np.inf)
        for k in which:
            which[k][idx] = res[k]
    out = {"frames": {name: dict(mssd=float(cols["mssd"][i]), mspd=float(cols["mspd"][i]),
                                 mssd_sym=int(which["mssd_sym"][i]), mspd_sym=int(which["mspd_sym"][i]), ok=bool(ok[i]))
                      for i, name in enumerate(names)}}
    out["n_frames"] = n
    out["n_evaluated"] = int(ok.sum())
    out["n_symmetries"] = int(n_syms)
    out["diameter"] = float(diameter)
    for k in cols:
        finite = cols[k][ok & np.isfinite(cols[k])]
        out[k + "_mean"] = float(finite.mean()) if finite.size else float("nan")
    out["ar_mssd"] = recall_mssd(cols["mssd"], diameter)
    out["ar_mspd"] = recall_mspd(cols["mspd"], widths)
    if ar_vsd is not None:
        out["ar_vsd"] = float(ar_vsd)
        out["ar_bop"] = (out["ar_vsd"] + out["ar_mssd"] + out["ar_mspd"]) / 3.0
    return out


def merge_bop(res: Dict, bop: Dict) -> Dict:
    """``res`` (``evaluate_poses`` / ``evaluate_poses_rendered``) with ``bop``'s (``evaluate_poses_bop``) summary keys and
    per-frame figures added; keys that ``res`` already holds keep its values."""
    for k, v in bop.items():
        if k != "frames":
            res.setdefault(k, v)
    for name, figures in bop["frames"].items():
        frame = res["frames"].setdefault(name, {})
        for k, v in figures.items():
            frame.setdefault(k, v)
    return res


def read_vertices(path) -> np.ndarray:
    """Model points [V, 3] from a ``.npy`` array [V, 3|4] or a whitespace text file of ``x y z`` rows (the shape of
    YCB's ``points.xyz``; further columns are ignored).  No mesh parsers."""
    path = str(path)
    v = np.load(path) if path.endswith(".npy") else np.loadtxt(path, ndmin=2)
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] < 3 or len(v) < 1 or (path.endswith(".npy") and v.shape[1] > 4):
        raise ValueError(f"{path}: expected [V, 3|4] points (got {v.shape})")
    return np.ascontiguousarray(v[:, :3])


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m pixtrack_amd.evaluation",
                                 description="ADD / ADD-S per frame, accuracy and AUC of a poses.pkl on the GPU")
    ap.add_argument("--poses", required=True, help="poses.pkl of a run (frames need gt_pose)")
    ap.add_argument("--vertices", required=True, help=".npy [V, 3|4] or a text file of x y z rows")
    ap.add_argument("--symmetric", action="store_true", help="the ADD(-S) column is ADD-S")
    ap.add_argument("--max_distance", type=float, default=0.1, help="upper end of the AUC's threshold range")
    ap.add_argument("--threshold", type=float, default=None, help="also report the accuracy under this distance")
    ap.add_argument("--offset", action="store_true", help="align the estimates with the notebook's similarity fit first")
    ap.add_argument("--json", default=None, help="write the summary and the per-frame figures to this file")
    ap.add_argument("--device", default="cuda:0")
    add_bop_arguments(ap)
    ap.add_argument("--diameter", type=float, default=None,
                    help="with --bop: the object's diameter in the units of the vertices (required)")
    return ap


def add_bop_arguments(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--bop", action="store_true",
                    help="also score BOP's MSSD / MSPD (frames need camera): mssd_mean, mspd_mean, ar_mssd, ar_mspd")
    ap.add_argument("--models_info", default=None,
                    help="with --bop: a BOP models_info.json (whole file or one object's dict) whose symmetries are "
                         "minimised over; default: the identity only")
    ap.add_argument("--obj_id", type=int, default=None, help="the object's key in a whole models_info.json")
    ap.add_argument("--models_info_scale", type=float, default=1.0,
                    help="factor from the units of models_info.json to the units of the vertices (BOP: 0.001 for metres)")


def bop_symmetries(args) -> Optional[np.ndarray]:
    """The symmetry set that ``--models_info`` / ``--obj_id`` name, translations scaled by ``--models_info_scale``."""
    if not args.models_info:
        return None
    from .symmetry import read_models_info

    sym = read_models_info(args.models_info, args.obj_id)["symmetries"].copy()
    sym[:, :3, 3] *= float(args.models_info_scale)
    return sym


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.bop and args.diameter is None:
        ap.error("--bop needs --diameter")
    from .utils.io import load_reference_pickle

    poses = load_reference_pickle(args.poses)
    vertices = read_vertices(args.vertices)
    res = evaluate_poses(poses, vertices, args.device, symmetric=args.symmetric,
                         max_distance=args.max_distance, threshold=args.threshold, offset=args.offset)
    if args.bop:
        merge_bop(res, evaluate_poses_bop(poses, vertices, args.device, args.diameter, symmetries=bop_symmetries(args),
                                          offset=args.offset))
    summary = {k: v for k, v in res.items() if k != "frames"}
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f)
    return res


if __name__ == "__main__":
    main()
