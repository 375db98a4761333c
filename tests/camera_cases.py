"""The camera table of the projection tests: one COLMAP camera per branch of project_point (csrc/pxt_common.h).

Every case is a 320 x 240 camera as make_lm_scene(camera=...) takes it, fx != fy and an off-centre principal point
wherever the model has the parameters for it (RADIAL has one focal length).  What each case reaches:

  pinhole    PINHOLE                                         ndist 0: no distortion code at all
  radial_k2  RADIAL  k1 = -0.08, k2 = 0.03                   k2 > 0 with 9 k1^2 - 20 k2 < 0: no range limit
  k1_limit   RADIAL  k1 = 0.9,  k2 = 0                       the limit r^2 < 1 / (3 k1) = 0.370
  k2_limit   RADIAL  k1 = 1.0,  k2 = 0.2                     k2 > 0, discriminant 5 > 0: r^2 < |(sqrt 5 - 3) / 2| = 0.382
  opencv     OPENCV  k1 = -0.08, k2 = 0.03, p1 = 0.004, p2 = -0.007   ndist 4: the tangential terms; p1 and p2 differ in
                                                             size and sign, so that a swap moves a point (0.04 px)

The two limit cases are wide cameras (f = 0.6 and 0.575 x width) whose scenes overfill the image (fill = 1.5): the
limit radius (distorted, 156 px and 160 px from the principal point) lies inside the image, so in-image points beyond
the range exist (tests/test_projection_host.py asserts the shares on the float64 oracle).

A plain module, imported by the test files; it holds no test and no fixture."""
import numpy as np

WIDTH, HEIGHT = 320, 240

CAMERAS = {
    "pinhole": dict(model="PINHOLE", params=[384.0, 380.0, 163.5, 117.25]),
    "radial_k2": dict(model="RADIAL", params=[384.0, 157.0, 123.5, -0.08, 0.03]),
    "k1_limit": dict(model="RADIAL", params=[192.0, 158.0, 122.0, 0.9, 0.0]),
    "k2_limit": dict(model="RADIAL", params=[184.0, 162.5, 118.0, 1.0, 0.2]),
    "opencv": dict(model="OPENCV", params=[384.0, 379.0, 156.0, 124.5, -0.08, 0.03, 0.004, -0.007]),
}
NDIST = {"pinhole": 0, "radial_k2": 2, "k1_limit": 2, "k2_limit": 2, "opencv": 4}
LIMIT_CASES = ("k1_limit", "k2_limit")
# make_lm_scene arguments that go with a case (beside seed, size and point count)
SCENE_KW = {name: dict(camera=cam, **({"fill": 1.5} if name in LIMIT_CASES else {})) for name, cam in CAMERAS.items()}

R2_REL_MARGIN = 1e-5  # a point nearer than this (relative, in r^2) to the range limit is not decidable in float32
Z_MARGIN = 1e-6  # ... nearer than this to eps in z
PX_MARGIN = 1e-3  # ... nearer than this (px) to an image border or a padded border


def colmap(name, width=WIDTH, height=HEIGHT):
    """The case as Camera.from_colmap takes it."""
    return dict(CAMERAS[name], width=width, height=height)


def r2_limit(dist):
    """The range limit in r^2 of the distortion (k1, k2, ...) in float64, or None where the model has none: the
    rule of pixloc's undistort_points (the magnitude of a root of 1 + 3 k1 r^2 + 5 k2 r^4), written out in scalars."""
    dist = [float(x) for x in dist]
    if len(dist) < 2:
        return None
    k1, k2 = dist[0], dist[1]
    disc = 9.0 * k1 * k1 - 20.0 * k2
    if k2 > 0 and disc > 0:
        return abs((np.sqrt(disc) - 3.0 * k1) / (10.0 * k2))
    if k2 <= 0 and k1 > 0:
        return 1.0 / (3.0 * k1)
    return None


def normalised_r2(p_cam, eps=1e-3):
    """r^2 of camera-frame points [N, 3] (float64) as project_point forms it, z clamped at eps."""
    p = np.asarray(p_cam, np.float64)
    z = np.maximum(p[:, 2], eps)
    return (p[:, 0] / z) ** 2 + (p[:, 1] / z) ** 2


def r2_margin(dist, p_cam):
    """Relative distance |r^2 - limit| / limit of every point to the range limit (inf where there is none)."""
    lim = r2_limit(dist)
    if lim is None:
        return np.full(len(p_cam), np.inf)
    return np.abs(normalised_r2(p_cam) - lim) / lim
