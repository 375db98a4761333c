"""The analytic scene of the sensor-depth refinement's tests and measurements: two ellipsoids (semi-axes
(0.05, 0.02, 0.02) at the origin, (0.015, 0.04, 0.015) at (0.02, 0.01, 0)) in front of a plane at z = 0.45, seen by a
pinhole camera of 160 x 120 (or the same intrinsics on a larger image); the depth is ray-cast per pixel and rounded to
counts of 1e-4.  numpy only."""
import numpy as np

from . import depth_refinement as DR

W, H = 160, 120
CAM10 = np.array([W, H, 210.0, 205.0, 77.3, 61.8, 0.0, 0.0, 0.0, 0.0])
SCALE = 1e-4
PLANE_Z = 0.45
ELLIPSOIDS = ((np.array([0.0, 0.0, 0.0]), np.array([0.05, 0.02, 0.02])),
              (np.array([0.02, 0.01, 0.0]), np.array([0.015, 0.04, 0.015])))
RVEC_GT = np.array([0.4, -0.7, 0.3])
T_GT = np.array([0.01, -0.005, 0.30])


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose12(R, t):
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)])


def raycast(R, t, width=W, height=H):
    """Camera-axis depth per pixel (pixel centres at integer coordinates: the LM's convention)."""
    fx, fy, cx, cy = CAM10[2:6]
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1).reshape(-1, 3)
    depth = np.full(len(d), PLANE_Z)
    for c, s in ELLIPSOIDS:
        # object frame: X = R^T (z d - t); ((X - c) / s)^2 = 1, a quadratic in z
        do = (d @ R) / s
        o = ((-t) @ R - c) / s
        A = (do * do).sum(1)
        B = 2 * (do * o).sum(1)
        C = (o * o).sum() - 1
        disc = B * B - 4 * A * C
        hit = disc > 0
        z = (-B - np.sqrt(np.where(hit, disc, 0))) / (2 * A)
        depth = np.where(hit & (z > 0) & (z < depth), z, depth)
    return depth.reshape(height, width)


def make_scene(width=W, height=H, n_per=3000, seed=7):
    """The scene at the ground-truth pose; ``points``: the samples of both surfaces that are valid there with
    |r| < 5e-4 and a footprint range below 0.004 (``all_points``: every sample)."""
    R = rodrigues(RVEC_GT)
    depth = raycast(R, T_GT, width, height)
    sensor = np.round(depth / SCALE).astype(np.uint16)
    rng = np.random.default_rng(seed)
    cam10 = np.concatenate([[width, height], CAM10[2:]])
    pts = []
    for c, s in ELLIPSOIDS:
        n = rng.normal(size=(n_per, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        pts.append(c + s * n)
    pts = np.concatenate(pts)
    sel = DR.DepthRefineConf(num_iters=0, pad=2, loss=0, max_residual=5e-4, max_edge=0.004, relative=False)
    st = DR.depth_step_reference(pts, None, sensor, SCALE, cam10, 0, pose12(R, T_GT), sel)
    return {"R": R, "t": T_GT, "T": pose12(R, T_GT), "sensor": sensor, "depth": depth, "points": pts[st["codes"] == 0],
            "all_points": pts, "cam10": cam10}
