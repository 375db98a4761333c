"""Pose information and covariance from the record of ``pxt_lm_information`` (include/pixtrack_hip.h): float64 numpy
on 48 host floats, no device work.

The record holds the LM's normal equations at one pose, undamped: g = sum w J^T r, H = sum w J^T J over the valid
points, w = rho' * conf_query * conf_ref, parameters in the LM's order (translation 3, rotation 3) for the LEFT update
exp(xi) T (a perturbation in the camera frame).  The reference has no counterpart (pixloc drops H after each step).

Nothing here feeds back into tracking: the cost gate, the pose update and ``tracked`` never read these values.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from .geometry import Pose, to_object_frame

RECORD_FLOATS = 48
INFO_KEYS = ("pose_info", "pose_cov", "observability", "info_level", "info_n_valid")

# H is summed in float32: a pivot of the unit-diagonal (Jacobi-scaled) Cholesky factor whose square falls below a few
# float32 roundings of the diagonal cannot be told from zero in those sums.
SINGULAR_PIVOT2 = 6 * float(np.finfo(np.float32).eps)

_IU = np.triu_indices(6)


def record_ok(rec) -> bool:
    return float(np.asarray(rec).reshape(-1)[47]) == 1.0


def information_from_record(rec) -> Tuple[np.ndarray, np.ndarray]:
    """-> (g [6], H [6, 6] symmetric) in float64."""
    r = np.asarray(rec, np.float64).reshape(-1)
    if r.size < RECORD_FLOATS:
        raise ValueError(f"an information record holds {RECORD_FLOATS} floats (got {r.size})")
    H = np.zeros((6, 6))
    H[_IU] = r[10:31]
    H = H + np.triu(H, 1).T
    return r[4:10].copy(), H


def _cholesky_spd(H: np.ndarray) -> Optional[np.ndarray]:
    """The lower Cholesky factor of H, or None when H is not positive definite beyond float32 rounding of its sums."""
    d = np.diag(H)
    if not np.all(np.isfinite(H)) or np.any(d <= 0):
        return None
    s = 1.0 / np.sqrt(d)
    try:
        Ls = np.linalg.cholesky(H * np.outer(s, s))
    except np.linalg.LinAlgError:
        return None
    if np.min(np.diag(Ls)) ** 2 < SINGULAR_PIVOT2:
        return None
    return Ls / s[:, None]


def covariance_from_record(rec, C: int):
    """-> (Sigma [6, 6] or None, flag).  sigma0^2 = rec[2] / (C * n_valid - 6) (the weighted squared residual per degree
    of freedom, the C descriptor channels counted as independent), Sigma = sigma0^2 H^-1 through a Cholesky factor.
    flag: "ok"; "skipped" (word 47 = -1: the record was not evaluated); "too_few_points" (word 47 = -2: evaluated with
    fewer valid points than the LM accepts); "dof" (no degrees of freedom left); "singular" (H singular or indefinite: never regularised, never an exception)."""
    r = np.asarray(rec, np.float64).reshape(-1)
    if not record_ok(r):
        return None, "too_few_points" if r[47] == -2.0 else "skipped"
    dof = int(C) * r[1] - 6.0
    if dof <= 0:
        return None, "dof"
    _, H = information_from_record(r)
    L = _cholesky_spd(H)
    if L is None:
        return None, "singular"
    Li = np.linalg.solve(L, np.eye(6))
    return (r[2] / dof) * (Li.T @ Li), "ok"


def sigma0_squared(rec, C: int) -> float:
    r = np.asarray(rec, np.float64).reshape(-1)
    dof = int(C) * r[1] - 6.0
    return float(r[2] / dof) if dof > 0 else float("nan")


def observability(H, pose: Pose, p3d, sigma0: float = 1.0) -> Dict:
    """How well the six degrees of freedom are constrained, read in the OBJECT's frame (to_object_frame) on S H S with
    S = diag(l, l, l, 1, 1, 1), l = the median distance of the points from their centroid: a translation by l and a
    rotation by one radian then move the points by comparable amounts, which makes the two comparable.
    -> {"condition": lambda_max / lambda_min of S H S (inf when lambda_min <= 0),
        "weakest_direction": unit 6-vector (translation, rotation; object frame, unscaled units) of lambda_min,
        "weakest_sigma": sigma0 / sqrt(lambda_min), the standard deviation along it in the scaled units (inf likewise),
        "scale": l}."""
    pts = np.asarray(p3d, np.float64).reshape(-1, 3)
    l = float(np.median(np.linalg.norm(pts - pts.mean(0), axis=1))) if len(pts) else 1.0
    if not np.isfinite(l) or l <= 0:
        l = 1.0
    S = np.diag([l, l, l, 1.0, 1.0, 1.0])
    Hs = S @ to_object_frame(H, pose) @ S
    lam, vec = np.linalg.eigh(0.5 * (Hs + Hs.T))
    d = S @ vec[:, 0]  # back to a twist in metres / radians
    d = d / np.linalg.norm(d)
    lo, hi = float(lam[0]), float(lam[-1])
    return {"condition": hi / lo if lo > 0 else float("inf"), "weakest_direction": d,
            "weakest_sigma": float(sigma0) / np.sqrt(lo) if lo > 0 else float("inf"), "scale": l}


def frame_entries(rec, C: int, level: int, pose: Pose, p3d) -> Dict:
    """The keys a tracker adds to a frame's history entry (INFO_KEYS) from the frame's information record; all None for
    a record that was skipped."""
    if rec is None or not record_ok(rec):
        return {k: None for k in INFO_KEYS}
    _, H = information_from_record(rec)
    cov, _flag = covariance_from_record(rec, C)
    s0 = sigma0_squared(rec, C)
    obs = observability(H, pose, p3d, np.sqrt(s0) if np.isfinite(s0) and s0 >= 0 else 1.0)
    return {"pose_info": H, "pose_cov": cov, "observability": obs, "info_level": int(level),
            "info_n_valid": int(np.asarray(rec).reshape(-1)[1])}
