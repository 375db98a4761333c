"""The projection arithmetic every projecting kernel shares, on the host, for every camera of tests/camera_cases.py.

Four statements of the same camera model exist on the host: oracle/lm_oracle.py (world2image, J_world2image: what the
GPU replays trust), pixtrack_amd/geometry.py (Camera), pixtrack_amd/depth_refinement.py (_project: numpy, the depth
refinement's and the occlusion gate's replays trust it) and csrc/pxt_common.h project_point compiled for the host
(pxt_unet_reference_tiles_host / pxt_unet_query_tiles_host).  Here they are held against each other in float64, the
oracle's Jacobian against a central difference of the oracle's own projection, and the camera table's scenes against
the conditions the GPU tests rely on.

Bars
  float64 against float64.  From the inputs to u the longest chain of roundings is: the division (1), r^2 (3), the
  radial polynomial (4), x + x * radial (2), the tangential terms (5), u = xd * fx + cx (2): 17 operations, each off
  by at most 2^-53 of the magnitude of what it forms.  Two correct statements in different operation order therefore
  differ by at most 2 x 17 x 2^-53 x mag, mag being the same expression with every term replaced by its magnitude
  (uv_magnitude / J_magnitude below): UV_OPS = J_OPS = 40 roundings are allowed (the Jacobian's chain, two 2 x 2 by
  2 x 3 products behind the distortion terms, is no longer than 20).
  The central difference with step h: (f(x + h) - f(x - h)) / 2h = f' + h^2 f''' / 6 + O(h^4), plus the rounding of
  the two values, 2^-53 |f| / h each.  The truncation term is measured, not guessed: the difference at h and at h / 2
  differ by 3/4 of the h^2 term, so 4/3 |D(h) - D(h/2)| is the truncation error of D(h) (to O(h^4)); the bar is twice
  that plus 4 x 2^-53 |u| / h for the roundings of both differences.  With h = 1e-4 the truncation is about 1e-5 on
  entries of about 400; a wrong cross term (2 p2 yn for 2 p1 xn) is off by 1."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import camera_cases as CC
from oracle import lm_oracle as O
from pixtrack_amd import _lib
from pixtrack_amd.depth_refinement import _project
from pixtrack_amd.geometry import Camera
from pixtrack_amd.synthetic import make_lm_scene

EPS64 = 2.0 ** -53
UV_OPS = 40
J_OPS = 40
FD_STEP = 1e-4
NAMES = list(CC.CAMERAS)


def camera64(name):
    """The case's ten-float record as the kernels get it (float32), widened: the same numbers for every statement."""
    cam = Camera.from_colmap(CC.colmap(name))
    assert cam._data.shape[-1] == 6 + CC.NDIST[name]
    return cam._data.double()


def camera_points(name, n=3000):
    """Camera-frame points: a frustum 1.4 x as wide as the image, points on and behind the camera plane, on either side
    of eps, and far outside the image."""
    cam = camera64(name).numpy()
    rng = np.random.default_rng(sum(map(ord, name)))
    z = rng.uniform(0.2, 4.0, n)
    xn = (rng.uniform(-0.2, 1.2, n) * cam[0] - cam[4]) / cam[2]
    yn = (rng.uniform(-0.2, 1.2, n) * cam[1] - cam[5]) / cam[3]
    p = np.stack([xn * z, yn * z, z], 1)
    behind = np.stack([rng.uniform(-1, 1, 60), rng.uniform(-1, 1, 60),
                       np.r_[np.zeros(10), np.full(10, 1e-3), np.full(10, 5e-4), np.full(10, 1.5e-3), -rng.uniform(0, 3, 20)]], 1)
    far = np.stack([rng.uniform(-60, 60, 100), rng.uniform(-60, 60, 100), rng.uniform(0.5, 2.0, 100)], 1)
    return np.concatenate([p, behind, far])


def uv_magnitude(cam, p):
    """[N, 2]: the projection with every term replaced by its magnitude."""
    z = p[:, 2:].clamp(min=O.CAM_EPS)
    pn = (p[:, :2] / z).abs()
    pd, _ = O._undistort(pn, cam[6:].abs())
    return pd * cam[2:4] + cam[4:6].abs()


def J_magnitude(cam, p):
    z = p[:, 2].clamp(min=O.CAM_EPS)
    zero = torch.zeros_like(z)
    Jp = torch.stack([1 / z, zero, p[:, 0].abs() / z ** 2, zero, 1 / z, p[:, 1].abs() / z ** 2], -1).reshape(-1, 2, 3)
    pn = (p[:, :2] / z[:, None]).abs()
    return torch.diag_embed(cam[2:4]).unsqueeze(0) @ O._J_undistort(pn, cam[6:].abs()) @ Jp


def oracle_parts(cam, p):
    """-> p2d, J, projectable (in front and inside the model's range), in_img, all from the float64 oracle."""
    p2d, valid = O.world2image(cam, p)
    z = p[:, 2]
    pn = p[:, :2] / z.clamp(min=O.CAM_EPS).unsqueeze(-1)
    _, in_range = O._undistort(pn, cam[6:])
    in_img = torch.all((p2d >= 0) & (p2d <= cam[:2] - 1), -1)
    projectable = (z > O.CAM_EPS) & in_range
    assert torch.equal(valid, projectable & in_img)
    return p2d, O.J_world2image(cam, p), projectable, in_img


@pytest.mark.parametrize("name", NAMES)
def test_geometry_camera_matches_the_oracle(name):
    cam = camera64(name)
    p = torch.from_numpy(camera_points(name))
    want_uv, want_J, projectable, in_img = oracle_parts(cam, p)
    got_uv, got_valid = Camera(cam).world2image(p)
    got_J, got_visible = Camera(cam).J_world2image(p)
    assert bool((got_uv - want_uv).abs().le(UV_OPS * EPS64 * uv_magnitude(cam, p)).all())
    assert bool((got_J - want_J).abs().le(J_OPS * EPS64 * J_magnitude(cam, p)).all())
    assert torch.equal(got_valid, projectable & in_img)
    assert torch.equal(got_visible, p[:, 2] > O.CAM_EPS)
    # the point set reaches every verdict
    assert 0 < int((projectable & in_img).sum()) < len(p) and int((~in_img).sum()) > 100 and int((p[:, 2] <= O.CAM_EPS).sum()) >= 40
    if name in CC.LIMIT_CASES:
        assert int(((p[:, 2] > O.CAM_EPS) & ~projectable & in_img).sum()) > 20


@pytest.mark.parametrize("name", NAMES)
def test_depth_refinement_project_matches_the_oracle(name):
    cam = camera64(name)
    pts = camera_points(name)
    p = torch.from_numpy(pts)
    want_uv, want_J, projectable, in_img = oracle_parts(cam, p)
    cam10 = np.zeros(10)
    cam10[:len(cam)] = cam.numpy()
    u, v, Jw, got_projectable, got_in_img = _project(cam10, CC.NDIST[name], pts[:, 0], pts[:, 1], pts[:, 2], np.float64)
    got_uv = torch.from_numpy(np.stack([u, v], 1))
    assert bool((got_uv - want_uv).abs().le(UV_OPS * EPS64 * uv_magnitude(cam, p)).all())
    assert bool((torch.from_numpy(Jw).reshape(-1, 2, 3) - want_J).abs().le(J_OPS * EPS64 * J_magnitude(cam, p)).all())
    assert np.array_equal(got_projectable, projectable.numpy())
    assert np.array_equal(got_in_img, in_img.numpy())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_jacobian_matches_a_central_difference(name):
    cam = camera64(name)
    # the frustum points: z >= 0.2 (the clamp of z is a kink; the difference is taken where the projection is smooth)
    # and |xn|, |yn| of an image 1.4 x as wide (at xn = 100 the polynomial's value is 1e10 and its rounding is the bar)
    pts = camera_points(name)[:3000]
    assert pts[:, 2].min() >= 0.2
    p = torch.from_numpy(pts)
    J = O.J_world2image(cam, p)

    def diff(h):
        cols = []
        for k in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[k] = h
            cols.append((O.world2image(cam, p + e)[0] - O.world2image(cam, p - e)[0]) / (2 * h))
        return torch.stack(cols, -1)

    D1, D2 = diff(FD_STEP), diff(FD_STEP / 2)
    truncation = (4.0 / 3.0) * (D1 - D2).abs()
    rounding = 4 * EPS64 * uv_magnitude(cam, p).unsqueeze(-1) / FD_STEP
    err = (D1 - J).abs()
    assert bool(err.le(2 * truncation + rounding).all()), float((err - 2 * truncation - rounding).max())
    # the bar is a bar: nowhere more than 1e-3 of the row's largest entry
    assert float(((2 * truncation + rounding) / J.abs().amax(-1, keepdim=True)).max()) < 1e-3


# ---- the camera table's scenes ----------------------------------------------------------------------------------
def scene_points_cam(sc, T12):
    T = np.asarray(T12, np.float32).astype(np.float64)
    return sc.p3d.astype(np.float32).astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:]


@pytest.mark.parametrize("name", NAMES)
def test_table_scene_carries_the_camera(name):
    sc = make_lm_scene(seed=1501, n_points=256, **CC.SCENE_KW[name])
    assert torch.equal(sc.camera._data, Camera.from_colmap(CC.colmap(name))._data)
    # the eye distance follows the case's focal length as it follows f in a default scene
    f = CC.CAMERAS[name]["params"][0]
    fill = CC.SCENE_KW[name].get("fill", 0.5)
    eye_dist = float(np.linalg.norm(sc.R_gt.T @ -sc.t_gt - sc.center))
    default = make_lm_scene(seed=1501, n_points=256)
    default_dist = float(np.linalg.norm(default.R_gt.T @ -default.t_gt - default.center))
    assert math.isclose(eye_dist / default_dist, (f / fill) / (1.2 * 320 / 0.5), rel_tol=1e-12)
    override = make_lm_scene(seed=1501, n_points=256, camera=dict(CC.CAMERAS[name], focal=2 * f), fill=fill)
    assert math.isclose(float(np.linalg.norm(override.R_gt.T @ -override.t_gt - override.center)), 2 * eye_dist, rel_tol=1e-12)
    assert torch.equal(override.camera._data, sc.camera._data)


def scene_arrays(sc):
    out = [sc.p3d, sc.camera._data.numpy(), sc.R_gt, sc.t_gt, sc.R_init, sc.t_init, sc.center, np.asarray(sc.scales)]
    return out + [t.numpy() for t in sc.feats_query] + [t.numpy() for t in sc.feats_ref]


@pytest.mark.parametrize("seed", [1001, 1305])
def test_default_scene_keeps_its_bits(seed):
    """camera=None, and the default camera handed in as camera=, give the arrays of a plain call bit for bit: the
    argument draws nothing from the generator."""
    kw = dict(seed=seed, n_points=300, k1=-0.05 if seed == 1305 else 0.0)
    plain = scene_arrays(make_lm_scene(**kw))
    none = scene_arrays(make_lm_scene(camera=None, **kw))
    same = dict(model="SIMPLE_RADIAL", params=[1.2 * 320, 160.0, 120.0, kw["k1"]])
    handed = scene_arrays(make_lm_scene(camera=same, **{**kw, "k1": 0.0}))
    for a, b, c in zip(plain, none, handed):
        assert a.dtype == b.dtype == c.dtype and a.tobytes() == b.tobytes() == c.tobytes()


@pytest.mark.parametrize("name", CC.LIMIT_CASES)
def test_limit_scenes_hold_points_on_both_sides_of_the_range(name):
    sc = make_lm_scene(seed=1501, **CC.SCENE_KW[name])
    for T in (sc.T_gt, sc.T_init):
        for s in sc.scales:
            cam = sc.camera.scale(s)._data.double()
            pc = scene_points_cam(sc, T.as12().numpy())
            _, _, projectable, in_img = oracle_parts(cam, torch.from_numpy(pc))
            n_img = int(in_img.sum())
            out_of_range = int((in_img & ~projectable).sum())
            print(f"{name} {int(cam[0])}x{int(cam[1])}: {n_img} in the image, {out_of_range} of them out of range "
                  f"({out_of_range / n_img:.1%}), nearest to the limit {CC.r2_margin(cam[6:], pc).min():.2e}")
            if cam[0] >= 80:  # the scene's own camera and the 80 x 60 level; at 20 x 15 the image is 5 % smaller, and printed only
                assert out_of_range >= 0.02 * n_img
            assert int((in_img & projectable).sum()) >= 0.5 * n_img
            assert CC.r2_margin(cam[6:], pc).min() > CC.R2_REL_MARGIN


def test_r2_limit_restates_the_oracle():
    for name in NAMES:
        dist = camera64(name)[6:]
        lim = CC.r2_limit(dist)
        r = torch.linspace(0.0, 1.5, 3001, dtype=torch.float64)
        _, ok = O._undistort(torch.stack([r, torch.zeros_like(r)], -1), dist)
        if lim is None:
            assert bool(ok.all()) and name not in CC.LIMIT_CASES
        else:
            assert name in CC.LIMIT_CASES and torch.equal(ok, r ** 2 < lim)


# ---- project_point itself, compiled for the host: the UNet's tile marking -----------------------------------------
TILE = 16
PAD, MARGIN = 1, 4


def tile_inputs(name):
    sc = make_lm_scene(seed=1501, n_points=1500, **CC.SCENE_KW[name])
    T12 = sc.T_init.as12().numpy().astype(np.float32)
    xyz = np.ascontiguousarray(sc.p3d.astype(np.float32))
    rng = np.random.default_rng(5)
    xyz[:40] += rng.normal(size=(40, 3)).astype(np.float32) * 3  # some far outside, some behind the camera
    cam10 = sc.camera.as10().numpy()
    pc = xyz.astype(np.float64) @ T12[:9].astype(np.float64).reshape(3, 3).T + T12[9:].astype(np.float64)
    return xyz, T12, cam10, pc


def record(xyz, T12, cam10, ndist, pad):
    pts = _lib.UnetSamplePoints()
    pts.p3d, pts.n_points = xyz.ctypes.data, len(xyz)
    pts.T[:] = T12.tolist()
    pts.cam[:] = cam10.tolist()
    pts.ndist, pts.pad = ndist, pad
    pts.x0, pts.y0, pts.full_w, pts.full_h = 0, 0, 0, 0
    return pts


def near_integer(x, tol=CC.PX_MARGIN):
    return np.abs(x - np.round(x)) < tol


@pytest.mark.parametrize("name", NAMES)
def test_reference_tiles_name_the_texels_of_the_float64_projection(name):
    xyz, T12, cam10, pc = tile_inputs(name)
    ndist = CC.NDIST[name]
    w, h = int(cam10[0]), int(cam10[1])
    cam = torch.from_numpy(cam10[:6 + ndist].astype(np.float64))
    p2d, _, projectable, _ = oracle_parts(cam, torch.from_numpy(pc))
    u, v = p2d[:, 0].numpy(), p2d[:, 1].numpy()
    inside = projectable.numpy() & (u >= PAD) & (v >= PAD) & (u <= w - 1 - PAD) & (v <= h - 1 - PAD)
    # decidable: away from a texel boundary (every border is one), from eps in z and from the range limit
    decidable = ~near_integer(u) & ~near_integer(v) & (np.abs(pc[:, 2] - 1e-3) > CC.Z_MARGIN) \
        & (CC.r2_margin(cam10[6:6 + ndist], pc) > CC.R2_REL_MARGIN)
    must = np.zeros((h // TILE, w // TILE), np.uint8)
    may = np.zeros_like(must)
    for i in np.nonzero(inside | ~decidable)[0]:
        if not (np.isfinite(u[i]) and np.isfinite(v[i]) and abs(u[i]) < 1e6 and abs(v[i]) < 1e6):
            continue
        for du in (-CC.PX_MARGIN, CC.PX_MARGIN) if not decidable[i] else (0.0,):
            for dv in (-CC.PX_MARGIN, CC.PX_MARGIN) if not decidable[i] else (0.0,):
                iu, iv = int(math.floor(u[i] + du)), int(math.floor(v[i] + dv))
                for tx in (iu, min(iu + 1, w - 1)):
                    for ty in (iv, min(iv + 1, h - 1)):
                        if 0 <= tx < w and 0 <= ty < h:
                            (must if decidable[i] else may)[ty // TILE, tx // TILE] = 1
    got = np.full(must.shape, 9, np.uint8)
    low = np.full((-(-(h // 2) // TILE), -(-(w // 2) // TILE)), 9, np.uint8)
    _lib.check(_lib.lib().pxt_unet_reference_tiles_host(C.byref(record(xyz, T12, cam10, ndist, PAD)), h, w, TILE, TILE,
                                                        got.ctypes.data, low.ctypes.data), "pxt_unet_reference_tiles_host")
    print(f"{name}: {int((~decidable).sum())} of {len(xyz)} points undecidable, {int(must.sum())} of {must.size} tiles needed")
    assert int((~decidable).sum()) <= 0.02 * len(xyz)
    assert 0 < must.sum() < must.size
    assert np.array_equal(got | may, must | may), (got, must)
    assert set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize("name", NAMES)
def test_query_tiles_name_the_box_of_the_float64_projection(name):
    xyz, T12, cam10, pc = tile_inputs(name)
    ndist = CC.NDIST[name]
    w, h = int(cam10[0]), int(cam10[1])
    cam = torch.from_numpy(cam10[:6 + ndist].astype(np.float64))
    p2d, _ = O.world2image(cam, torch.from_numpy(pc))
    ru, rv = p2d[:, 0].numpy(), p2d[:, 1].numpy()
    u, v = np.clip(ru, -8.0, w + 8.0), np.clip(rv, -8.0, h + 8.0)  # (the kernel's own clamp; beyond it nothing is to decide)
    decidable = ~(near_integer(ru) & (u == ru)) & ~(near_integer(rv) & (v == rv)) & (np.abs(pc[:, 2] - 1e-3) > CC.Z_MARGIN)
    must = np.zeros((h // TILE, w // TILE), np.uint8)
    may = np.zeros_like(must)

    def box(iu, iv, flags):
        xa, xb = (min(max(iu + d, 0), w - 1) for d in (-1, 2))
        ya, yb = (min(max(iv + d, 0), h - 1) for d in (-1, 2))
        xa, xb, ya, yb = max(xa - MARGIN, 0), min(xb + MARGIN, w - 1), max(ya - MARGIN, 0), min(yb + MARGIN, h - 1)
        flags[ya // TILE:yb // TILE + 1, xa // TILE:xb // TILE + 1] = 1

    for i in range(len(xyz)):
        if decidable[i]:
            if pc[i, 2] > 1e-3:
                box(int(math.floor(u[i])), int(math.floor(v[i])), must)
        else:
            for du in (-CC.PX_MARGIN, CC.PX_MARGIN):
                for dv in (-CC.PX_MARGIN, CC.PX_MARGIN):
                    box(int(math.floor(u[i] + du)), int(math.floor(v[i] + dv)), may)
    qry = _lib.UnetQueryPoints()
    qry.points = record(xyz, T12, cam10, ndist, PAD)
    qry.margin = MARGIN
    got = np.full(must.shape, 9, np.uint8)
    low = np.full((-(-(h // 2) // TILE), -(-(w // 2) // TILE)), 9, np.uint8)
    _lib.check(_lib.lib().pxt_unet_query_tiles_host(C.byref(qry), h, w, TILE, TILE, got.ctypes.data, low.ctypes.data),
               "pxt_unet_query_tiles_host")
    print(f"{name}: {int((~decidable).sum())} of {len(xyz)} points undecidable, {int(must.sum())} of {must.size} tiles marked")
    assert int((~decidable).sum()) <= 0.02 * len(xyz)
    assert 0 < must.sum()
    assert np.array_equal(got | may, must | may), (got, must)
