"""Sensor-depth pose refinement behind the LM (``pxt_depth_refine``, include/pixtrack_hip.h; opt-in).

The feature-metric LM fixes a pose from image gradients and leaves the translation along the viewing ray weakly
determined (``observability``).  Where the data set keeps a depth image beside every colour frame
(YCB-Video), that image measures exactly this direction.  Starting at the LM's pose, a damped Gauss-Newton minimises

    r_n(T) = D(project(T X_n)) - (T X_n).z

over the frame's 3-D points X_n: D is the sensor image (raw uint16 counts x ``sensor_scale``) read through the LM's
bilinear footprint.  Points over a hole (raw 0), across a depth edge or too far from the measured surface are rejected
per evaluation; damping and an optional 6 x 6 prior on the accumulated update keep the pose where the depth does not
constrain it.

* ``depth_refine``: the GPU path - K problems, all iterations, one launch of ``torch.ops.pixtrack.depth_refine``; the
  start pose may be the record of an LM launch queued ahead on the same stream (no host wait in between).
* ``depth_step_reference`` / ``depth_refine_reference``: the numpy restatement, float32 in the kernel's order of
  operations or float64 - the oracle of the tests (as ``sensor_vsd_reference`` is for its kernel).  What it cannot
  restate is the kernel's FMA contraction and its summation order over lanes and waves.

The length-valued defaults of ``DepthRefineConf`` (Huber scale, ``max_residual``, ``max_edge``, ``dt_stop``) are
FRACTIONS of the point set's extent - its bounding-box diagonal - because an SfM model has no metric scale.  They are
starting values from a CPU prototype on an analytic scene (two ellipsoids in front of a plane); nobody has tuned them
on real depth frames.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

RECORD = 32
LOG_STRIDE = 20
MAX_POINTS = 4096
MAX_ITERS = 32
MAX_PROBLEMS = 16
CODE_NAMES = ("valid", "masked", "projection", "outside", "no_measurement", "depth_edge", "residual")
CAM_EPS = 1e-3  # pxt_common.h kCamEps


@dataclass(frozen=True)
class DepthRefineConf:
    """``pxt_depth_conf``.  With ``relative`` (the default) ``loss_scale``, ``max_residual``, ``max_edge`` and
    ``dt_stop`` are fractions of the point set's extent; ``resolve(extent)`` gives the absolute conf the kernel takes.
    The defaults are untuned starting values (module docstring)."""
    num_iters: int = 10
    pad: int = 2
    loss: int = 1                 # 0 squared, 1 huber, 2 barron(alpha): the LM's robust_loss on r * r
    loss_alpha: float = 0.0
    loss_scale: float = 0.02
    lambda_: Tuple[float, ...] = (1e-2,) * 6
    max_residual: float = 0.1
    max_edge: float = 0.05
    grad_stop: float = 0.0        # |g| mixes lengths and angles at the model's scale: off unless the caller sets it
    dt_stop: float = 1e-4
    dR_stop: float = 1e-2         # degrees
    min_valid: int = 10
    relative: bool = True

    def resolve(self, extent: float) -> "DepthRefineConf":
        if not self.relative:
            return self
        e = float(extent)
        if not (e > 0.0 and np.isfinite(e)):
            raise ValueError(f"the point set's extent must be positive and finite (got {extent})")
        return replace(self, loss_scale=self.loss_scale * e, max_residual=self.max_residual * e,
                       max_edge=self.max_edge * e, dt_stop=self.dt_stop * e, relative=False)

    @classmethod
    def from_sfm_scale(cls, extent: float, **overrides) -> "DepthRefineConf":
        """The absolute conf for a point set of the given extent (SfM units); ``overrides`` are fractions as well."""
        return cls(**overrides).resolve(extent)


def points_extent(points) -> float:
    """The bounding-box diagonal of a point set [N, 3] (numpy or tensor)."""
    p = points.detach().cpu().numpy() if hasattr(points, "detach") else np.asarray(points)
    p = p.reshape(-1, 3).astype(np.float64)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def prior_upper(prior) -> np.ndarray:
    """None, a diagonal (w_t, w_r), 6 diagonal entries, a 6 x 6 symmetric matrix or its 21 upper entries -> the 21
    upper-triangle entries (row-major, (t, w) order) of ``pxt_depth_problem.prior``."""
    if prior is None:
        return np.zeros(21)
    p = np.asarray(prior, dtype=np.float64)
    if p.shape == (2,):
        p = np.diag([p[0]] * 3 + [p[1]] * 3)
    elif p.shape == (6,):
        p = np.diag(p)
    if p.shape == (21,):
        return p.copy()
    if p.shape != (6, 6) or not np.allclose(p, p.T):
        raise ValueError("prior: (w_t, w_r), 6 diagonal entries, a symmetric 6 x 6 matrix or its 21 upper entries")
    return p[np.triu_indices(6)].copy()


def _prior_matrix(prior21, dt) -> np.ndarray:
    P = np.zeros((6, 6), dtype=dt)
    P[np.triu_indices(6)] = np.asarray(prior21, dtype=dt)
    return P + np.triu(P, 1).T


# --------------------------------------------------------------------------------------------------- reference
def _robust_loss(kind: int, alpha, scale, x, dt):
    """pxt_lm_point.h robust_loss on an array x -> (loss, weight)."""
    x = np.asarray(x, dtype=dt)
    if kind == 0:
        return x.copy(), np.ones_like(x)
    one, two = dt(1), dt(2)
    a2 = dt(scale) * dt(scale)
    y = x / a2
    if kind == 1:
        sy = np.sqrt(np.maximum(y, dt(1e-30)))
        l = np.where(y <= one, y, two * sy - one)
        d = np.where(y <= one, one, np.maximum(dt(1.1920929e-07), one / sy))
    else:
        alpha = dt(alpha)
        if alpha == 0:
            l = two * np.log1p(np.minimum(dt(0.5) * y, dt(33e37)))
            d = two / (y + two)
        elif alpha == 2:
            l, d = y, np.ones_like(y)
        else:
            beta = max(abs(alpha - two), dt(1e-7))
            as_ = (one if alpha >= 0 else -one) * max(abs(alpha), dt(1e-7))
            l = two * (beta / as_) * (np.power(y / beta + one, dt(0.5) * alpha) - one)
            d = np.power(y / beta + one, dt(0.5) * alpha - one)
    return (l * a2).astype(dt), np.asarray(d, dtype=dt)


def _project(cam10, ndist: int, px, py, pz, dt):
    """pxt_common.h project_point on arrays -> u, v, Jw [N, 6], projectable (in front, inside the distortion model's
    range), in_img."""
    w, h, fx, fy, cx, cy, k1, k2, p1, p2 = (dt(c) for c in np.asarray(cam10, dtype=dt))
    eps = dt(CAM_EPS)
    visible = pz > eps
    iz = dt(1) / np.maximum(pz, eps)
    xn, yn = px * iz, py * iz
    xd, yd = xn, yn
    dist_ok = np.ones_like(visible)
    Jd00, Jd01, Jd10, Jd11 = np.ones_like(xn), np.zeros_like(xn), np.zeros_like(xn), np.ones_like(xn)
    if ndist > 0:
        r2 = xn * xn + yn * yn
        radial = k1 * r2 + k2 * r2 * r2
        xd = xn + xn * radial
        yd = yn + yn * radial
        disc = dt(9) * k1 * k1 - dt(20) * k2
        if (k2 > 0 and disc > 0) or (k2 <= 0 and k1 > 0):
            limit = (np.sqrt(max(disc, dt(0))) - dt(3) * k1) / (dt(10) * k2) if k2 > 0 else dt(1) / (dt(3) * k1)
            dist_ok = r2 < abs(limit)
        uv = xn * yn
        d_radial = dt(2) * k1 + dt(4) * k2 * r2
        Jd00 = Jd00 + (radial + xn * xn * d_radial)
        Jd11 = Jd11 + (radial + yn * yn * d_radial)
        Jd01 = Jd01 + uv * d_radial
        Jd10 = Jd10 + uv * d_radial
        if ndist > 2:
            xd = xd + (dt(2) * p1 * uv + p2 * (r2 + dt(2) * xn * xn))
            yd = yd + (dt(2) * p2 * uv + p1 * (r2 + dt(2) * yn * yn))
            Jd00 = Jd00 + (dt(2) * p1 * yn + dt(6) * p2 * xn)
            Jd11 = Jd11 + (dt(2) * p2 * xn + dt(6) * p1 * yn)
            Jd01 = Jd01 + (dt(2) * p1 * xn + dt(2) * p2 * yn)
            Jd10 = Jd10 + (dt(2) * p2 * yn + dt(2) * p1 * xn)
    u = xd * fx + cx
    v = yd * fy + cy
    with np.errstate(invalid="ignore"):
        in_img = (u >= 0) & (v >= 0) & (u <= w - dt(1)) & (v <= h - dt(1))
    a, bx, by = iz, -px * iz * iz, -py * iz * iz
    m00, m01, m10, m11 = fx * Jd00, fx * Jd01, fy * Jd10, fy * Jd11
    Jw = np.stack([m00 * a, m01 * a, m00 * bx + m01 * by, m10 * a, m11 * a, m10 * bx + m11 * by], axis=1)
    return u, v, Jw.astype(dt), visible & dist_ok, in_img


def footprint_values(sensor, ix0, iy0):
    """The raw counts of the 4 x 4 neighbourhood whose row 1, column 1 is texel (ix0, iy0), as int64 [N, 4, 4]; a
    position outside the image counts as 0.  (The cross uses rows 0, 3 x columns 1, 2 and rows 1, 2 x columns 0..3.)"""
    sensor = np.asarray(sensor)
    H, W = sensor.shape
    out = np.zeros((len(ix0), 4, 4), dtype=np.int64)
    for r in range(4):
        for c in range(4):
            x, y = ix0 + (c - 1), iy0 + (r - 1)
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            out[:, r, c] = np.where(inside, sensor[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0)
    return out


_CROSS = np.zeros((4, 4), dtype=bool)
_CROSS[0, 1:3] = _CROSS[3, 1:3] = True
_CROSS[1:3, :] = True


def depth_step_reference(points, mask, sensor, sensor_scale: float, cam10, ndist: int, T12, conf: DepthRefineConf,
                         dtype=np.float64, codes: Optional[np.ndarray] = None) -> Dict:
    """One evaluation at pose ``T12`` (12 values: row-major R, then t) in ``dtype``: the per-point terms and the sums of
    ``pxt_depth_refine`` WITHOUT the prior.  ``codes``: take these reject codes instead of the own ones (a replay that
    must follow another evaluation's decisions on points at a gate).  ``conf`` is absolute (``resolve``d).

    -> dict: codes [N] (the own ones), used [N] (the codes that decided), u, v, p [N, 3], F, r, w, rho, gx, gy, J0, J1
    (point_jacobian's rows of d(u, v)/d(delta)), Jz (the p.z row), J = gx J0 + gy J1 - Jz [N, 6], cost, n_valid, g [6], H [6, 6], counts [6] (codes 1..6), and the distances from the gates: border (pixels inside
    the padded window, negative outside), edge and residual (relative to their thresholds), cell (pixels from the
    nearest texel boundary)."""
    if conf.relative:
        raise ValueError("depth_step_reference takes an absolute conf: DepthRefineConf.resolve(extent)")
    dt = np.dtype(dtype).type
    X = np.asarray(points, dtype=dt).reshape(-1, 3)
    N = len(X)
    T = np.asarray(T12, dtype=dt).reshape(12)
    sensor = np.asarray(sensor)
    H, W = sensor.shape
    scale = dt(sensor_scale)
    kept = np.ones(N, dtype=bool) if mask is None else np.asarray(mask).reshape(N) != 0
    px = T[0] * X[:, 0] + T[1] * X[:, 1] + T[2] * X[:, 2] + T[9]
    py = T[3] * X[:, 0] + T[4] * X[:, 1] + T[5] * X[:, 2] + T[10]
    pz = T[6] * X[:, 0] + T[7] * X[:, 1] + T[8] * X[:, 2] + T[11]
    u, v, Jw, projectable, in_img = _project(cam10, ndist, px, py, pz, dt)
    pad = dt(conf.pad)
    with np.errstate(invalid="ignore"):
        border = np.minimum(np.minimum(u - pad, v - pad), np.minimum(dt(W - 1) - pad - u, dt(H - 1) - pad - v))
        window = (u >= pad) & (v >= pad) & (u <= dt(W - 1) - pad) & (v <= dt(H - 1) - pad)
    own = np.zeros(N, dtype=np.uint8)
    own[~(projectable & in_img & window)] = 3
    own[~projectable] = 2
    own[~kept] = 1
    # the footprint of every point that has one (u, v finite); the others keep zeros and a code 1..3
    finite = np.isfinite(u) & np.isfinite(v)
    us, vs = np.where(finite, u, dt(0)), np.where(finite, v, dt(0))
    fu, fv = np.floor(us), np.floor(vs)
    ix0, iy0 = fu.astype(np.int64), fv.astype(np.int64)
    ax, ay = us - fu, vs - fv
    one = dt(1)
    w00, w10, w01, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    raw = footprint_values(sensor, ix0, iy0)
    cross = raw[:, _CROSS]
    lo, hi = cross.min(1), cross.max(1)
    spread = (hi - lo).astype(dt) * scale
    a = raw.astype(dt) * scale
    F = w00 * a[:, 1, 1] + w10 * a[:, 1, 2] + w01 * a[:, 2, 1] + w11 * a[:, 2, 2]
    Fxp = w00 * a[:, 1, 2] + w10 * a[:, 1, 3] + w01 * a[:, 2, 2] + w11 * a[:, 2, 3]
    Fxm = w00 * a[:, 1, 0] + w10 * a[:, 1, 1] + w01 * a[:, 2, 0] + w11 * a[:, 2, 1]
    Fyp = w00 * a[:, 2, 1] + w10 * a[:, 2, 2] + w01 * a[:, 3, 1] + w11 * a[:, 3, 2]
    Fym = w00 * a[:, 0, 1] + w10 * a[:, 0, 2] + w01 * a[:, 1, 1] + w11 * a[:, 1, 2]
    gx, gy = dt(0.5) * (Fxp - Fxm), dt(0.5) * (Fyp - Fym)
    r = F - pz
    ok = own == 0
    own[ok & (lo == 0)] = 4
    own[ok & (lo != 0) & (spread > dt(conf.max_edge))] = 5
    with np.errstate(invalid="ignore"):
        own[(own == 0) & (np.abs(r) > dt(conf.max_residual))] = 6
    used = own if codes is None else np.asarray(codes, dtype=np.uint8).reshape(N)
    valid = used == 0
    rho, wl = _robust_loss(conf.loss, conf.loss_alpha, conf.loss_scale, r * r, dt)
    # point_jacobian: Jw (2 x 3) [I | -[p]x]
    J0 = np.stack([Jw[:, 0], Jw[:, 1], Jw[:, 2], -Jw[:, 1] * pz + Jw[:, 2] * py, Jw[:, 0] * pz - Jw[:, 2] * px,
                   -Jw[:, 0] * py + Jw[:, 1] * px], axis=1)
    J1 = np.stack([Jw[:, 3], Jw[:, 4], Jw[:, 5], -Jw[:, 4] * pz + Jw[:, 5] * py, Jw[:, 3] * pz - Jw[:, 5] * px,
                   -Jw[:, 3] * py + Jw[:, 4] * px], axis=1)
    zero = np.zeros_like(pz)
    Jz = np.stack([zero, zero, zero + one, py, -px, zero], axis=1)
    J = (gx[:, None] * J0 + gy[:, None] * J1 - Jz).astype(dt)
    Jv, rv, wv = J[valid], r[valid], wl[valid]
    g = ((wv * rv)[:, None] * Jv).sum(0, dtype=dt)
    Hm = np.einsum("n,nk,nl->kl", wv, Jv, Jv).astype(dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_edge = np.abs(spread - dt(conf.max_edge)) / dt(conf.max_edge) if conf.max_edge > 0 else np.full(N, np.inf)
        rel_res = np.abs(np.abs(r) - dt(conf.max_residual)) / dt(conf.max_residual) if conf.max_residual > 0 \
            else np.full(N, np.inf)
    cell = np.minimum(np.minimum(ax, one - ax), np.minimum(ay, one - ay))
    return {"codes": own, "used": used, "u": u, "v": v, "p": np.stack([px, py, pz], 1), "r": r, "w": wl, "rho": rho,
            "gx": gx, "gy": gy, "F": F, "J": J, "J0": J0, "J1": J1, "Jz": Jz, "cost": dt(rho[valid].sum(dtype=dt)), "n_valid": int(valid.sum()),
            "g": g, "H": Hm, "counts": np.array([int((used == c).sum()) for c in range(1, 7)]),
            "border": border, "edge": rel_edge, "residual": rel_res, "cell": cell}


def fragile_points(step: Dict, px_tol: float = 1e-3, rel_tol: float = 1e-4, cell_tol: float = 1e-4) -> np.ndarray:
    """The points of an evaluation whose reject code another rounding may decide differently: within ``px_tol`` pixels
    of the padded border, ``rel_tol`` (relative) of the edge or residual gate, ``cell_tol`` pixels of a texel boundary
    (where the footprint, and with it the hole and edge tests, changes), or with a depth at the camera's epsilon."""
    codes = step["codes"]
    with np.errstate(invalid="ignore"):
        near_border = np.abs(step["border"]) < px_tol
        near_eps = np.abs(step["p"][:, 2] - CAM_EPS) < 1e-6
        in_window = (codes == 0) | (codes >= 4)
        near_gate = in_window & ((step["edge"] < rel_tol) | (step["residual"] < rel_tol) | (step["cell"] < cell_tol))
    return (codes != 1) & (near_border | near_eps | near_gate)


def solve6_reference(g, Hm, lam, dtype=np.float64):
    """The LM's damped solve in ``dtype``: H_kk += max(H_kk * lambda_k, 1e-6); Cholesky, pivoted LU on [H | g] when a
    pivot is not positive.  -> (delta, lu_flag)"""
    dt = np.dtype(dtype).type
    Hd = np.array(Hm, dtype=dt)
    g = np.asarray(g, dtype=dt)
    for k in range(6):
        Hd[k, k] = Hd[k, k] + max(Hd[k, k] * dt(lam[k]), dt(1e-6))
    L = np.zeros((6, 6), dtype=dt)
    ok = True
    for j in range(6):
        d = Hd[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not d > 0:
            ok = False
            break
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            s = Hd[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    if ok:
        y = np.zeros(6, dtype=dt)
        for i in range(6):
            s = g[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        x = np.zeros(6, dtype=dt)
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
        return -x, False
    A = np.concatenate([Hd, g[:, None]], axis=1)
    for c in range(6):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
        for r in range(c + 1, 6):
            f = A[r, c] / A[c, c]
            A[r, c:] = A[r, c:] - f * A[c, c:]
    x = np.zeros(6, dtype=dt)
    for i in range(5, -1, -1):
        s = A[i, 6]
        for k in range(i + 1, 6):
            s = s - A[i, k] * x[k]
        x[i] = s / A[i, i]
    return -x, True


def apply_delta_reference(delta, T12, dtype=np.float64):
    """T <- (so3exp(dw), dt) T in ``dtype`` -> (T12, dR in degrees, dt): pxt_lm.hip's apply_delta."""
    dt = np.dtype(dtype).type
    d = np.asarray(delta, dtype=dt)
    T = np.asarray(T12, dtype=dt).reshape(12)
    wx, wy, wz = d[3], d[4], d[5]
    theta = np.sqrt(wx * wx + wy * wy + wz * wz)
    if theta < dt(1e-7):
        Rd = np.array([[1, -wz, wy], [wz, 1, -wx], [-wy, wx, 1]], dtype=dt)
    else:
        x, y, z = wx / theta, wy / theta, wz / theta
        s, c1 = np.sin(theta), dt(1) - np.cos(theta)
        if dt is np.float32 and theta < 0.25:  # (1 - cos cancels in float32: the kernel's series, summed in float64)
            c1 = dt(2.0 * np.sin(0.5 * float(theta)) ** 2)
        Rd = np.array([[1 + c1 * (x * x - 1), -s * z + c1 * (x * y), s * y + c1 * (x * z)],
                       [s * z + c1 * (x * y), 1 + c1 * (y * y - 1), -s * x + c1 * (y * z)],
                       [-s * y + c1 * (x * z), s * x + c1 * (y * z), 1 + c1 * (z * z - 1)]], dtype=dt)
    R, t = T[:9].reshape(3, 3), T[9:]
    Rn = (Rd @ R).astype(dt)
    tn = (Rd @ t + d[:3]).astype(dt)
    cs = min(max((np.trace(Rd) - dt(1)) * dt(0.5), dt(-1)), dt(1))
    dR = abs(np.arccos(cs)) / dt(np.pi) * dt(180)
    return np.concatenate([Rn.reshape(9), tn]).astype(dt), dt(dR), dt(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def depth_refine_reference(points, mask, sensor, sensor_scale: float, cam10, ndist: int, T12, conf: DepthRefineConf,
                           prior=None, dtype=np.float64) -> Dict:
    """The whole refinement of ``pxt_depth_refine`` in ``dtype`` -> dict(record [32], log [iterations, 20], codes
    [iterations + 1, N], T [12], failed, iterations, steps: the evaluations' ``depth_step_reference`` results)."""
    if conf.relative:
        raise ValueError("depth_refine_reference takes an absolute conf: DepthRefineConf.resolve(extent)")
    dt = np.dtype(dtype).type
    P = _prior_matrix(prior_upper(prior), dt)
    T = np.asarray(T12, dtype=dt).reshape(12).copy()
    a = np.zeros(6, dtype=dt)
    rec = np.zeros(RECORD, dtype=dt)
    log, codes, steps = [], [], []
    stop = False
    ev = 0
    while True:
        st = depth_step_reference(points, mask, sensor, sensor_scale, cam10, ndist, T, conf, dtype)
        steps.append(st)
        codes.append(st["codes"])
        n_valid = st["n_valid"]
        mean = st["cost"] / dt(max(n_valid, 1))
        if ev == 0:
            rec[14], rec[15] = mean, n_valid
        fail = n_valid < conf.min_valid
        if fail or stop or ev == conf.num_iters:
            rec[12], rec[13], rec[16], rec[17] = float(fail), ev, mean, n_valid
            rec[18:24] = st["counts"]
            break
        g = (st["g"] + P @ a).astype(dt)
        Hm = (st["H"] + P).astype(dt)
        delta, lu = solve6_reference(g, Hm, conf.lambda_, dtype)
        T, dR, dtr = apply_delta_reference(delta, T, dtype)
        a = (a + delta).astype(dt)
        gn = dt(np.sqrt((g * g).sum(dtype=dt)))
        stop = bool((dtr < dt(conf.dt_stop) and dR < dt(conf.dR_stop)) or gn < dt(conf.grad_stop))
        line = np.zeros(LOG_STRIDE, dtype=dt)
        line[:6] = [mean, n_valid, dR, dtr, gn, float(lu)]
        line[8:] = T
        log.append(line)
        ev += 1
    rec[:12] = T
    rec[24:30] = a
    rec[31] = -2.0 if rec[12] else 1.0
    return {"record": rec, "log": np.array(log, dtype=dt).reshape(-1, LOG_STRIDE), "codes": np.array(codes, dtype=np.uint8),
            "T": T, "failed": bool(rec[12]), "iterations": ev, "steps": steps}


def decode_record(rec) -> Dict:
    """A 32-float record -> dict(status, ok, T (12), failed, iterations, cost_before, n_valid_before, cost_after,
    n_valid_after, counts {name: n}, update [6])."""
    r = np.asarray(rec.detach().cpu().numpy() if hasattr(rec, "detach") else rec, dtype=np.float64).reshape(-1)
    status = float(r[31])
    if status == -1.0:  # skipped: nothing but the status word was written
        return {"status": status, "ok": False, "T": None, "failed": True, "iterations": 0, "cost_before": None,
                "n_valid_before": 0, "cost_after": None, "n_valid_after": 0, "counts": {}, "update": None}
    return {"status": status, "ok": status == 1.0 and r[12] == 0.0, "T": r[:12].copy(), "failed": bool(r[12] != 0.0),
            "iterations": int(r[13]), "cost_before": float(r[14]), "n_valid_before": int(r[15]),
            "cost_after": float(r[16]), "n_valid_after": int(r[17]),
            "counts": {CODE_NAMES[c]: int(r[17 + c]) for c in range(1, 7)}, "update": r[24:30].copy()}


# --------------------------------------------------------------------------------------------------------- GPU
class PendingDepth:
    """Result handle of an enqueued ``pxt_depth_refine`` launch: ``result()`` waits and returns the float64 records
    (32 each); ``logs`` / ``codes`` are the device tensors asked for (or None)."""

    def __init__(self, recs, keep, done, logs, codes):
        self.recs, self._keep, self._done, self.logs, self.codes = recs, keep, done, logs, codes

    def result(self):
        self._done.synchronize()
        return [r[:RECORD].double().cpu().numpy().copy() for r in self.recs]


def _camera10(camera):
    """A geometry.Camera or (10 floats, ndist) -> ([10 floats], ndist)."""
    if hasattr(camera, "as10"):
        return [float(x) for x in camera.as10().tolist()], int(camera._data.shape[-1] - 6)
    cam, ndist = camera
    vals = [float(x) for x in np.asarray(cam, dtype=np.float64).reshape(-1)]
    if len(vals) != 10:
        raise ValueError("camera: a geometry.Camera or (10 floats, ndist)")
    return vals, int(ndist)


def depth_refine_batch(problems: Sequence[Dict], conf: DepthRefineConf, workspace=None, want_log: bool = False,
                       want_codes: bool = False, records=None) -> PendingDepth:
    """Enqueue ONE ``pxt_depth_refine`` launch on the current stream.  ``problems[k]`` = dict(points [N, 3] device
    float32, mask (uint8 [N] or None), sensor (uint16 / int16 [H, W] device tensor), sensor_scale, camera (Camera or
    (10 floats, ndist)), pose, prior (``prior_upper``'s forms or None)); ``pose`` is 12 floats (a Pose, array or
    tensor; staged in pinned memory) or an optimizer.PendingLM / a 16+-float record tensor of an LM launch queued ahead
    - all K poses of one kind.  ``conf`` is absolute, or relative and then resolved PER LAUNCH with problem 0's extent
    (a device-to-host read: pass an absolute conf on a hot path).  ``records``: K pinned float32 [32] tensors the
    launch writes its records to (a caller that keeps them across calls; default: fresh ones)."""
    import torch

    from . import _lib
    from .ops import ops

    K = len(problems)
    if not (1 <= K <= MAX_PROBLEMS):
        raise ValueError(f"{K} problems (1..{MAX_PROBLEMS})")
    if conf.relative:
        conf = conf.resolve(points_extent(problems[0]["points"]))
    pts = [p["points"].to(torch.float32).contiguous() for p in problems]
    dev = pts[0].device
    masks = [None if p.get("mask") is None else p["mask"].to(dev, torch.uint8).contiguous() for p in problems]
    sensors, scales, cams, ndist, poses, priors, keep = [], [], [], [], [], [], []
    first = problems[0]["pose"]
    from_lm = hasattr(first, "buf") or (torch.is_tensor(first) and first.numel() >= 16)
    for p in problems:
        sen = p["sensor"]
        if not torch.is_tensor(sen):
            sen = torch.from_numpy(np.ascontiguousarray(np.asarray(sen, dtype=np.uint16)).view(np.int16))
        sensors.append(sen.to(dev).contiguous())
        scales.append(float(p["sensor_scale"]))
        c10, nd = _camera10(p["camera"])
        if (int(sensors[-1].shape[1]), int(sensors[-1].shape[0])) != (int(round(c10[0])), int(round(c10[1]))):
            raise ValueError(f"the sensor image is {tuple(sensors[-1].shape)[::-1]}, the camera {c10[0]:g} x {c10[1]:g}")
        cams += c10
        ndist.append(nd)
        priors += [float(x) for x in prior_upper(p.get("prior"))]
        pose = p["pose"]
        if from_lm:
            poses.append(pose.buf if hasattr(pose, "buf") else pose)
            keep.append(pose)
        else:
            T = pose.as12() if hasattr(pose, "as12") else pose
            T = torch.as_tensor(np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, dtype=np.float32)).reshape(12)
            staged = torch.zeros(16, dtype=torch.float32).pin_memory()
            staged[:12] = T
            poses.append(staged)
    recs = list(records if records is not None else torch.zeros(K, RECORD, dtype=torch.float32).pin_memory())
    if len(recs) != K or any(r.dtype != torch.float32 or r.numel() < RECORD or not r.is_pinned() for r in recs):
        raise ValueError(f"records: {K} pinned float32 tensors of {RECORD} floats")
    logs = [torch.zeros(conf.num_iters, LOG_STRIDE, dtype=torch.float32, device=dev) if want_log else None
            for _ in range(K)]
    codes = [torch.zeros(conf.num_iters + 1, int(x.shape[0]), dtype=torch.uint8, device=dev) if want_codes else None
             for x in pts]
    if workspace is None:
        workspace = torch.zeros(int(_lib.lib().pxt_depth_refine_workspace_bytes(K)), dtype=torch.uint8, device=dev)
    ops.depth_refine(pts, masks, sensors, scales, cams, ndist, poses, bool(from_lm), priors, int(conf.num_iters),
                     int(conf.pad), int(conf.loss), float(conf.loss_alpha), float(conf.loss_scale),
                     [float(x) for x in conf.lambda_], float(conf.max_residual), float(conf.max_edge),
                     float(conf.grad_stop), float(conf.dt_stop), float(conf.dR_stop), int(conf.min_valid), recs, logs,
                     codes, workspace)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    return PendingDepth(recs, (pts, masks, sensors, poses, keep, workspace), done, logs, codes)


def depth_refine(points, mask, sensor_u16, sensor_scale: float, camera, pose_or_lm_record, conf: DepthRefineConf,
                 prior=None, want_log: bool = False, want_codes: bool = False) -> Dict:
    """One refinement on the GPU, awaited: -> ``decode_record``'s dict plus ``record`` (float64 [32]) and, when asked
    for, ``log`` (float64 [iterations, 20]) and ``codes`` (uint8 [iterations + 1, N])."""
    h = depth_refine_batch([dict(points=points, mask=mask, sensor=sensor_u16, sensor_scale=sensor_scale, camera=camera,
                                 pose=pose_or_lm_record, prior=prior)], conf, want_log=want_log, want_codes=want_codes)
    rec = h.result()[0]
    out = decode_record(rec)
    out["record"] = rec
    n = out["iterations"]
    if want_log:
        out["log"] = h.logs[0][:n].double().cpu().numpy()
    if want_codes:
        out["codes"] = h.codes[0][:n + 1].cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------------ tracker
@dataclass
class DepthRefine:
    """The tracker option (``PixLocPoseTrackerR9(depth_refine=...)``): a conf (relative: resolved once with the SfM
    model's extent), the sensor's scale in SfM units per count, ``lookup(frame_name) -> uint16 [H, W]`` (None: the
    frame has no depth image - its pose stays the LM's) and an optional diagonal prior (w_t, w_r)."""
    lookup: Callable[[str], Optional[np.ndarray]]
    sensor_depth_scale: float
    conf: DepthRefineConf = DepthRefineConf()
    prior: Optional[Tuple[float, float]] = None


HISTORY_KEYS = ("T_lm", "depth_refined", "depth_cost_before", "depth_cost_after", "depth_n_valid", "depth_iters")


def accept(rec: Optional[Dict], lm_success: bool) -> bool:
    """The tracker's policy: the depth-refined pose replaces the LM's only if the frame succeeded, the record's status
    is 1.0, it did not fail and the final mean depth cost is not above the initial one."""
    return bool(lm_success and rec is not None and rec["status"] == 1.0 and not rec["failed"]
                and rec["cost_after"] <= rec["cost_before"])
