"""The per-point residual report of ``pxt_lm_point_report`` (include/pixtrack_hip.h) on the host: a 16-float summary
per refinement -> the keys a tracker adds to a frame's history entry, an ``[N, 8]`` points tensor -> numpy arrays.

The reference's only health signal is one masked-mean cost (DebugTracker.log_optim_iter, pixtrack/localization/
tracker.py:32-46); its point set is kept at debug >= 2 (tracker.py:26-30).  What is decoded here says which points
carried a pose: where each projects, whether the LM counted it, its residual, its robust weight rho' and its confidence
weight.  Nothing on the policy path reads any of it.

``inlier_ratio`` counts the valid points whose robust weight is at least ``point_report_inlier_weight`` (refiner conf,
default 0.5).  For the default loss (barron, alpha 0, scale 0.1: rho' = 2 / (|r|^2 / scale^2 + 2)) that is the residual
at which the loss has halved a point's weight, |r| = sqrt(2) scale.  It is a convention, not a tuned value.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

POINT_FLOATS = 8     # PXT_LM_POINT_RECORD
SUMMARY_FLOATS = 16  # PXT_LM_REPORT_SUMMARY
MODES = (False, "summary", "full")
DEFAULT_INLIER_WEIGHT = 0.5
REJECT_NAMES = ("masked", "projection", "border")  # reject codes 1, 2, 3
SUMMARY_KEYS = ("n_valid_points", "n_inliers", "inlier_ratio", "mean_robust_weight", "rejected_points")
POINT_KEYS = ("p2d", "valid", "cost", "rho", "robust_weight", "confidence", "reject")


def parse_mode(value):
    """False / None / "off" -> False, "summary", "full"; anything else is a ValueError."""
    if value is None or value is False or value == "off":
        return False
    if value in ("summary", "full"):
        return value
    raise ValueError(f"point_report must be False ('off'), 'summary' or 'full' (got {value!r})")


def decode_summary(summary) -> Dict:
    """-> {"n_valid_points", "n_inliers", "inlier_ratio", "mean_robust_weight", "rejected": {"masked", "projection",
    "border"}, "cost_sum", "status"}.  ``mean_robust_weight`` is the confidence-weighted mean of rho' over the valid
    points, summary[3] / summary[4]; both ratios are None when no point is valid (or the confidences sum to zero)."""
    s = np.asarray(summary, np.float64).reshape(-1)
    if s.size != SUMMARY_FLOATS:
        raise ValueError(f"a point-report summary holds {SUMMARY_FLOATS} floats (got {s.size})")
    n_valid, n_inl = int(s[1]), int(s[2])
    return {"n_valid_points": n_valid, "n_inliers": n_inl,
            "inlier_ratio": n_inl / n_valid if n_valid > 0 else None,
            "mean_robust_weight": float(s[3] / s[4]) if n_valid > 0 and s[4] > 0 else None,
            "rejected": {name: int(s[5 + k]) for k, name in enumerate(REJECT_NAMES)},
            "cost_sum": float(s[0]), "status": float(s[15])}


def decode_points(points) -> Dict[str, np.ndarray]:
    """[N, 8] point records (tensor or array) -> {"p2d" [N, 2] float32, "valid" bool, "cost" (|r|^2), "rho",
    "robust_weight" (rho'), "confidence" (w_unc), "reject" uint8 (0 valid, 1 masked, 2 projection, 3 border)}."""
    if hasattr(points, "detach"):
        points = points.detach().cpu().numpy()
    p = np.asarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != POINT_FLOATS:
        raise ValueError(f"point records are [N, {POINT_FLOATS}] (got {p.shape})")
    return {"p2d": p[:, 1:3].copy(), "valid": p[:, 0] != 0, "cost": p[:, 3].copy(), "rho": p[:, 4].copy(),
            "robust_weight": p[:, 5].copy(), "confidence": p[:, 6].copy(), "reject": p[:, 7].astype(np.uint8)}


def frame_entries(summary, points: Optional[Dict[str, np.ndarray]] = None, full: bool = False) -> Dict:
    """The keys a tracker adds to a frame's history entry: SUMMARY_KEYS, plus ``point_report`` in "full" mode; all None
    for a frame that ran no (successful) refinement."""
    if summary is None:
        out = {k: None for k in SUMMARY_KEYS}
    else:
        d = decode_summary(summary)
        out = {"n_valid_points": d["n_valid_points"], "n_inliers": d["n_inliers"], "inlier_ratio": d["inlier_ratio"],
               "mean_robust_weight": d["mean_robust_weight"], "rejected_points": d["rejected"]}
    if full:
        out["point_report"] = points
    return out
