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
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    args = build_parser().parse_args(argv)
    from .utils.io import load_reference_pickle

    poses = load_reference_pickle(args.poses)
    res = evaluate_poses(poses, read_vertices(args.vertices), args.device, symmetric=args.symmetric,
                         max_distance=args.max_distance, threshold=args.threshold, offset=args.offset)
    summary = {k: v for k, v in res.items() if k != "frames"}
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f)
    return res


if __name__ == "__main__":
    main()
