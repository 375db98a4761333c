"""The mesh rasteriser's rule on the host: mesh_render.rasterize_reference (the numpy restatement the kernel is held to bit
for bit in test_mesh_raster_gpu.py, which runs every case of CASES below), the readers and the view records."""
import struct

import numpy as np
import pytest
import torch

from pixtrack_amd import mesh as M
from pixtrack_amd import mesh_render as R

EYE = np.eye(3)


def view(fx=1.0, fy=1.0, cx=0.0, cy=0.0, Rm=EYE, t=(0.0, 0.0, 0.0), near=1e-6, depth_q=1.0):
    return R.pack_view(Rm, t, fx, fy, cx, cy, near, depth_q)


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def on_plane(xy, z=1.0):
    """Vertices (x, y, z) that the unit camera (f = 1, c = 0 at depth 1) puts on the image points xy."""
    xy = np.asarray(xy, np.float64)
    return np.concatenate([xy * z, np.full((len(xy), 1), z)], 1)


# ---------------------------------------------------------------------------------------------------------------- cases
SPHERE_VIEW = dict(fx=77.3, fy=75.9, cx=31.37, cy=23.61, t=(0.013, -0.007, 0.6))


def case_top_left(winding):
    F = [(0, 1, 2)] if winding == "ccw" else [(0, 2, 1)]
    return on_plane([(1, 1), (6, 1), (1, 6)]), np.asarray(F), view()[None], 8, 8


def case_shared_edge():
    return on_plane([(1, 1), (6, 1), (6, 6), (1, 6)]), np.asarray([(0, 1, 2), (0, 2, 3)]), view()[None], 8, 8


def case_icosphere(sub):
    V, F = R.icosphere(sub)
    return V * 0.1, F, view(Rm=rotation(0), **SPHERE_VIEW)[None], 64, 48


def case_torus():
    V, F = R.torus()
    a = np.deg2rad(70.0)  # seen from near its plane: the far side of the ring shows through the hole
    tilt = np.asarray([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]) @ rotation(1)
    return V * 0.1, F, view(Rm=tilt, **SPHERE_VIEW)[None], 64, 48


QUAD_DEPTH = 0.73


def case_fronto_quad():
    V = on_plane([(-0.31, -0.22), (0.29, -0.2), (0.33, 0.27), (-0.3, 0.21)], QUAD_DEPTH)
    return V, np.asarray([(0, 1, 2), (0, 2, 3)]), view(fx=61.3, fy=58.9, cx=19.7, cy=15.2)[None], 40, 32


def case_sphere_depth():
    V, F = R.icosphere(3)
    return V * 0.1, F, view(**SPHERE_VIEW)[None], 64, 48


def case_coincident():
    V = on_plane([(1, 1), (6, 1), (1, 6)])
    return V, np.asarray([(0, 1, 2), (0, 2, 1), (1, 2, 0)]), view()[None], 8, 8


SLOPE = 0.3


def case_interpenetrating():
    # two planes z = 1 +- SLOPE x through one large triangle each; they cross on the line x = 0
    xy = np.asarray([(-2.0, -2.0), (2.0, -2.0), (0.0, 3.0)])
    A = np.concatenate([xy, 1.0 + SLOPE * xy[:, :1]], 1)
    B = np.concatenate([xy, 1.0 - SLOPE * xy[:, :1]], 1)
    return np.concatenate([A, B]), np.asarray([(0, 1, 2), (3, 4, 5)]), view(fx=20.0, fy=20.0, cx=15.4, cy=11.5)[None], 32, 24


def case_culls():
    V = [(0.0, 0.0, 1.0), (3.0, 0.0, 1.0), (0.0, 3.0, 1.0),        # 0-2 a fine triangle
         (1.0, 1.0, 0.05),                                           # 3 behind near
         (np.nan, 0.0, 1.0),                                         # 4
         (40000.0, 0.0, 1.0),                                        # 5 beyond the guard: 40000 px * 256 >= 2^23
         (-5.0, 1.0, 1.0), (-3.0, 1.0, 1.0), (-4.0, 3.0, 1.0),       # 6-8 left of the image
         (12.0, 1.0, 1.0), (14.0, 1.0, 1.0), (13.0, 3.0, 1.0),       # 9-11 right
         (1.0, -5.0, 1.0), (3.0, -5.0, 1.0), (2.0, -3.0, 1.0),       # 12-14 above
         (1.0, 12.0, 1.0), (3.0, 12.0, 1.0), (2.0, 14.0, 1.0)]       # 15-17 below
    F = [(0, 1, 2), (0, 1, 3), (0, 4, 2), (5, 1, 2), (0, 1, -1), (0, len(V), 2), (0, 1, 1), (6, 7, 8), (9, 10, 11),
         (12, 13, 14), (15, 16, 17)]
    return np.asarray(V), np.asarray(F), view(near=0.1)[None], 8, 8


def case_bad_view():
    V, F = R.icosphere(1)
    good = view(**SPHERE_VIEW)
    bad = good.copy()
    bad[13] = np.inf
    nan = good.copy()
    nan[4] = np.nan
    return V * 0.1, F, np.stack([bad, good, nan]), 64, 48


CASES = {
    "top_left_ccw": lambda: case_top_left("ccw"), "top_left_cw": lambda: case_top_left("cw"),
    "shared_edge": case_shared_edge, "icosphere_80": lambda: case_icosphere(1), "icosphere_1280": lambda: case_icosphere(3),
    "torus": case_torus, "fronto_quad": case_fronto_quad, "sphere_depth": case_sphere_depth,
    "coincident": case_coincident, "interpenetrating": case_interpenetrating, "culls": case_culls,
    "bad_view": case_bad_view,
}


def draw(name, coverage=False):
    V, F, views, W, H = CASES[name]()
    return R.rasterize_reference(V, F, views, W, H, coverage=coverage)


# --------------------------------------------------------------------------------------------------------------- the rule
def test_top_left_rule_in_both_windings():
    a, b = draw("top_left_ccw"), draw("top_left_cw")
    j, i = np.mgrid[0:8, 0:8]
    want = (i >= 1) & (j >= 1) & (i + j < 7)  # the top and the left edge belong to the triangle, the hypotenuse does not
    for depth, ids, rec in (a, b):
        assert np.array_equal(depth[0, ..., 3] == 1.0, want) and rec[0, R.W_COVERED] == 15 and rec[0, R.W_DRAWN] == 1
        assert np.array_equal(ids[0] == 0, want) and np.array_equal(ids[0] == -1, ~want)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_shared_edge_is_claimed_exactly_once():
    depth, ids, rec, cov = draw("shared_edge", coverage=True)
    j, i = np.mgrid[0:8, 0:8]
    inside = (i >= 1) & (i < 6) & (j >= 1) & (j < 6)
    assert np.array_equal(cov[0], inside.astype(np.int32))
    # the diagonal is the left edge of the upper-right half
    assert np.array_equal(ids[0], np.where(inside, np.where(i >= j, 0, 1), -1))


@pytest.mark.parametrize("name,n", [("icosphere_80", 80), ("icosphere_1280", 1280)])
def test_icospheres_are_watertight(name, n):
    depth, ids, rec, cov = draw(name, coverage=True)
    assert rec[0, R.W_DRAWN] == n and set(np.unique(cov)) == {0, 2}
    assert np.array_equal(cov[0] == 2, depth[0, ..., 3] == 1.0) and rec[0, R.W_COVERED] == (cov == 2).sum() > 400


def test_torus_is_covered_an_even_number_of_times():
    depth, ids, rec, cov = draw("torus", coverage=True)
    assert (cov % 2 == 0).all() and cov.max() >= 4 and (cov == 2).any()
    assert np.array_equal(cov[0] > 0, depth[0, ..., 3] == 1.0)


def ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32))


def test_fronto_parallel_quad_returns_its_depth():
    depth, ids, rec = draw("fronto_quad")
    hit = depth[0, ..., 3] == 1.0
    assert hit.sum() > 500 and ulps(depth[0, ..., 0][hit], np.float32(QUAD_DEPTH)).max() <= 4
    assert np.array_equal(depth[0, ..., 0], depth[0, ..., 1]) and np.array_equal(depth[0, ..., 0], depth[0, ..., 2])
    z = np.asarray([rec[0, R.W_ZMIN], rec[0, R.W_ZMAX]], np.uint32).view(np.float32)
    assert z[0] == depth[0, ..., 0][hit].min() and z[1] == depth[0, ..., 0][hit].max()


def test_icosphere_depth_against_the_exact_sphere():
    V, F, views, W, H = CASES["sphere_depth"]()
    depth, ids, rec = R.rasterize_reference(V, F, views, W, H)
    r, c = 0.1, np.asarray(SPHERE_VIEW["t"], np.float64)
    j, i = np.mgrid[0:H, 0:W]
    d = np.stack([(i - SPHERE_VIEW["cx"]) / SPHERE_VIEW["fx"], (j - SPHERE_VIEW["cy"]) / SPHERE_VIEW["fy"], np.ones((H, W))], -1)
    a, b, cc = (d * d).sum(-1), (d * c).sum(-1), c @ c - r * r
    disc = b * b - a * cc
    s = (b - np.sqrt(np.maximum(disc, 0))) / a  # the point s * d; s is its camera-axis depth since d.z = 1
    normal = (s[..., None] * d - c) / r
    cos_inc = -(normal * d).sum(-1) / np.sqrt(a)
    sel = (disc > 0) & (cos_inc >= 0.5)  # hit normal within 60 degrees of the ray
    # The bound, from the tessellation: a flat triangle whose longest edge is e lies at most r - sqrt(r^2 - e^2 / 3) below
    # the sphere (its farthest point from the vertices is within e / sqrt(3) of one), seen along a ray at up to 60
    # degrees to the normal: twice that.  Vertices snap to 1/256 pixel: at most half a step per axis in the image, that
    # is sqrt(2) / 512 pixels * z / f along the surface, times tan(60 degrees) in depth.
    edge = max(np.linalg.norm(V[F[:, k]] - V[F[:, (k + 1) % 3]], axis=1).max() for k in range(3))
    bound = 2.0 * (r - np.sqrt(r * r - edge * edge / 3.0))
    bound += np.sqrt(2.0) / 512.0 * s[sel].max() / min(SPHERE_VIEW["fx"], SPHERE_VIEW["fy"]) * np.sqrt(3.0)
    err = np.abs(depth[0, ..., 0].astype(np.float64) - s)[sel]
    print("sphere depth: pixels", int(sel.sum()), "max error", float(err.max()), "bound", float(bound))
    assert sel.sum() > 300 and (depth[0, ..., 3][sel] == 1.0).all() and err.max() <= bound


def test_coincident_triangles_go_to_the_lowest_index():
    depth, ids, rec, cov = draw("coincident", coverage=True)
    assert set(np.unique(cov)) == {0, 3} and set(np.unique(ids)) == {-1, 0} and rec[0, R.W_DRAWN] == 3


def test_interpenetrating_triangles_split_along_their_intersection():
    V, F, views, W, H = CASES["interpenetrating"]()
    depth, ids, rec, cov = R.rasterize_reference(V, F, views, W, H, coverage=True)
    j, i = np.mgrid[0:H, 0:W]
    xn = (i - 15.4) / 20.0
    both = cov[0] == 2
    assert both.sum() > 300 and np.array_equal(ids[0][both], np.where(xn < 0, 0, 1)[both])
    want = 1.0 / (1.0 + SLOPE * np.abs(xn))  # the nearer of z = 1 / (1 -+ SLOPE xn)
    assert np.abs(depth[0, ..., 0][both] - want[both]).max() < 2e-3  # the snap of the vertices, nothing else


def test_every_cull_is_counted_under_its_cause():
    depth, ids, rec = draw("culls")
    want = {R.W_DRAWN: 1, R.W_NEAR: 1, R.W_GUARD: 2, R.W_ZERO: 1, R.W_INDEX: 2, R.W_OFF: 4, R.W_STATUS: 0}
    assert {k: int(rec[0, k]) for k in want} == want
    assert rec[0, 1:7].sum() == 11 and set(np.unique(ids)) == {-1, 0} and rec[0, R.W_COVERED] == (ids == 0).sum() == 6
    assert (rec[0, 10:] == 0).all()


def test_a_non_finite_view_draws_nothing():
    depth, ids, rec = draw("bad_view")
    for p in (0, 2):
        assert rec[p, R.W_STATUS] == 0xFFFFFFFF and (depth[p] == 0).all() and (ids[p] == -1).all()
        assert (rec[p, :7] == 0).all() and rec[p, R.W_ZMIN] == 0xFFFFFFFF and rec[p, R.W_ZMAX] == 0
    assert rec[1, R.W_STATUS] == 0 and rec[1, R.W_COVERED] > 400
    solo = R.rasterize_reference(*CASES["bad_view"]()[:2], CASES["bad_view"]()[2][1:2], 64, 48)
    assert np.array_equal(solo[0][0].view(np.uint32), depth[1].view(np.uint32)) and np.array_equal(solo[2][0], rec[1])


def test_depth_q_scales_the_image_and_not_the_record():
    V, F, views, W, H = CASES["icosphere_80"]()
    scaled = views.copy()
    scaled[0, 17] = 3.5
    a, b = R.rasterize_reference(V, F, views, W, H), R.rasterize_reference(V, F, scaled, W, H)
    assert np.array_equal(b[0][..., 0], a[0][..., 0] * np.float32(3.5)) and np.array_equal(a[0][..., 3], b[0][..., 3])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------------ the readers
def test_read_mesh_round_trips_and_fans(tmp_path):
    V, F = R.icosphere(1)
    V = V.astype(np.float32).astype(np.float64)
    M.write_obj(tmp_path / "a.obj", V, F)
    M.write_ply(tmp_path / "a.ply", V, F, N=V, C=np.abs(V))
    with open(tmp_path / "b.ply", "wb") as f:  # binary_little_endian with a property before x and uint8 list counts
        f.write(b"ply\nformat binary_little_endian 1.0\ncomment made by the test\nelement vertex %d\nproperty uchar tag\n"
                b"property float x\nproperty float y\nproperty double z\nelement face %d\n"
                b"property list uchar int vertex_index\nend_header\n" % (len(V), len(F)))
        for v in V:
            f.write(struct.pack("<Bffd", 7, *v))
        for t in F:
            f.write(struct.pack("<Biii", 3, *t))
    for name in ("a.obj", "a.ply", "b.ply"):
        V2, F2 = R.read_mesh(tmp_path / name)
        assert np.array_equal(F2, F) and np.array_equal(V2.astype(np.float32), V.astype(np.float32)), name
    # polygons are fanned from their first corner
    (tmp_path / "q.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 2 0\nf 1 2 3 4 5\n")
    (tmp_path / "q.ply").write_text("ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
                                    "property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                    "0 0 0\n1 0 0\n1 1 0\n0 1 0\n0.5 2 0\n5 0 1 2 3 4\n")
    for name in ("q.obj", "q.ply"):
        V2, F2 = R.read_mesh(tmp_path / name)
        assert len(V2) == 5 and F2.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4]], name


def test_read_mesh_refusals(tmp_path):
    head = "ply\nformat %s 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float %s\nelement face 1\n" \
           "property list uchar int %s\nend_header\n0 0 0\n3 0 0 0\n"
    (tmp_path / "big.ply").write_text(head % ("binary_big_endian", "z", "vertex_indices"))
    (tmp_path / "noz.ply").write_text(head % ("ascii", "w", "vertex_indices"))
    (tmp_path / "face.ply").write_text(head % ("ascii", "z", "corners"))
    (tmp_path / "index.ply").write_text((head % ("ascii", "z", "vertex_indices")).replace("3 0 0 0", "3 0 0 1"))
    (tmp_path / "mesh.stl").write_text("solid\n")
    (tmp_path / "junk.ply").write_text("plain text\n")
    for name, word in (("big.ply", "binary_big_endian"), ("noz.ply", "vertex"), ("face.ply", "face"),
                       ("index.ply", "indices"), ("mesh.stl", ".stl"), ("junk.ply", "PLY")):
        with pytest.raises(ValueError, match=word):
            R.read_mesh(tmp_path / name)


# ------------------------------------------------------------------------------------------------------- the view records
def test_view_record_projects_like_the_camera():
    from pixtrack_amd.geometry import Camera, Pose

    rng = np.random.default_rng(3)
    cam = Camera(torch.tensor([64.0, 48.0, 77.3, 75.9, 31.37, 23.61]))
    Rm, t = rotation(5), np.asarray([0.02, -0.01, 0.8])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    pose = Pose.from_Rt(torch.from_numpy(Rm), torch.from_numpy(t))
    rec = R.view_record(cam, T, near=0.01, depth_q=2.0)
    assert rec.dtype == np.float32 and rec.shape == (20,) and np.array_equal(rec, R.view_record(cam, pose, 0.01, 2.0))
    assert rec[16] == np.float32(0.01) and rec[17] == 2.0 and (rec[18:] == 0).all()
    pts = rng.uniform(-0.1, 0.1, size=(200, 3))
    want, valid = cam.world2image(pose.float() * torch.from_numpy(pts).float())
    p = pts.astype(np.float32) @ rec[:9].reshape(3, 3).T + rec[9:12]
    got = p[:, :2] / p[:, 2:] * rec[12:14] + rec[14:16]
    # both are a handful of float32 operations on coordinates below 64: a few ulp of 64
    assert valid.all() and np.abs(got - want.numpy()).max() < 64 * 8 * 2.0 ** -24
    with pytest.raises(ValueError, match="lens"):
        R.view_record(Camera(torch.tensor([64.0, 48.0, 77.3, 75.9, 31.37, 23.61, 0.1, 0.0])), T)
    zero_lens = Camera(torch.tensor([64.0, 48.0, 77.3, 75.9, 31.37, 23.61, 0.0, 0.0]))
    assert np.array_equal(R.view_record(zero_lens, T, 0.01, 2.0), rec)


def test_ngp_view_record_is_the_renderers_pixel_rule():
    C = np.concatenate([rotation(7), [[0.4], [0.5], [0.6]]], 1)
    rec = R.ngp_view_record(C, 120.0, 64, 48, depth_q=0.25)
    assert rec[12] == rec[13] == 120.0 and rec[14] == 31.5 and rec[15] == 23.5 and rec[17] == 0.25
    # the renderer's ray through pixel (i, j): origin C[:, 3], direction C[:, :3] @ ((i + .5 - W/2) / f, (j + .5 - H/2) / f, 1)
    i, j, s = 10, 40, 0.7
    point = C[:, 3] + s * (C[:, :3] @ np.asarray([(i + 0.5 - 32) / 120.0, (j + 0.5 - 24) / 120.0, 1.0]))
    p = rec[:9].reshape(3, 3).astype(np.float64) @ point + rec[9:12]
    assert abs(p[2] - s) < 1e-6 and abs(p[0] / p[2] * 120.0 + rec[14] - i) < 1e-4 and abs(p[1] / p[2] * 120.0 + rec[15] - j) < 1e-4


def test_the_op_and_the_entry_points_are_declared():
    from pixtrack_amd import _lib, ops

    assert "mesh_raster" in ops.op_names()
    assert {"pxt_mesh_raster", "pxt_mesh_raster_workspace_bytes"} <= set(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.pxt_mesh_raster_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 1, 1, 1), (4097, 1, 1, 1), (1, 0, 1, 1), (1, (1 << 24) + 1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0),
                (1, 1, 1 << 13, (1 << 13) + 1)):
        assert L.pxt_mesh_raster_workspace_bytes(*bad) < 0, bad
    assert L.pxt_mesh_raster_workspace_bytes(4096, 1 << 24, 1 << 13, 1 << 13) > 0
    # a failed check launches nothing: these return before any HIP call, on a machine without a GPU too
    assert L.pxt_mesh_raster(16, 1, 16, 1, 16, 1, 4, 4, 16, None, 16, 20, None) == -1   # workspace not 16-byte aligned
    assert L.pxt_mesh_raster(16, 1, 16, 1, 16, 1, 4, 4, 24, None, 16, 32, None) == -1   # out_depth not 16-byte aligned
    assert L.pxt_mesh_raster(16, 0, 16, 1, 16, 1, 4, 4, 16, None, 16, 32, None) == -1   # V = 0
    assert L.pxt_mesh_raster(None, 1, 16, 1, 16, 1, 4, 4, 16, None, 16, 32, None) == -1
