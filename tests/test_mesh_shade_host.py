"""The colour rule of pxt_mesh_render on the host: mesh_render.shade_reference (the numpy restatement the kernel is held
to bit for bit in test_mesh_shade_gpu.py), the colour readers, the look-at views and the reference builder."""
import struct

import numpy as np
import pytest

from pixtrack_amd import mesh as M
from pixtrack_amd import mesh_dataset as D
from pixtrack_amd import mesh_render as R
from test_mesh_raster_host import CASES, ulps, view


def colours(n, seed=7):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- the rule
TILT = np.deg2rad(60.0)
QUAD_R = np.asarray([[np.cos(TILT), 0, np.sin(TILT)], [0, 1, 0], [-np.sin(TILT), 0, np.cos(TILT)]])
QUAD_T = np.asarray([0.0, 0.0, 1.2])
QUAD_F, QUAD_C = 80.0, (31.5, 23.5)
AFFINE = np.asarray([[0.5, 0.3, 0.2], [0.5, -0.25, 0.3], [0.55, 0.1, -0.4]])  # per channel: a0 + ax x + ay y


def affine(xy):
    return AFFINE[:, 0] + xy @ AFFINE[:, 1:].T


def test_colour_is_perspective_correct():
    V = np.asarray([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)])
    F = np.asarray([(0, 1, 2), (0, 2, 3)])
    C = affine(V[:, :2])
    assert C.min() > 0.2 and C.max() < 0.85
    W, H = 64, 48
    rgba, u8, depth, nz, ids, rec = R.shade_reference(V, F, C, view(QUAD_F, QUAD_F, *QUAD_C, Rm=QUAD_R, t=QUAD_T)[None], W, H)
    hit = ids[0] >= 0
    j, i = np.mgrid[0:H, 0:W]
    # where the pixel's ray s * d meets the plane: object coordinates q = R^T (s d - t) with q.z = 0
    d = np.stack([(i - QUAD_C[0]) / QUAD_F, (j - QUAD_C[1]) / QUAD_F, np.ones((H, W))], -1)
    s = (QUAD_R.T @ QUAD_T)[2] / (d @ QUAD_R)[..., 2]
    q = (s[..., None] * d - QUAD_T) @ QUAD_R
    want = affine(q[..., :2])
    g_max = max(np.abs(want[:, 1:] - want[:, :-1])[hit[:, 1:] & hit[:, :-1]].max(),
                np.abs(want[1:] - want[:-1])[hit[1:] & hit[:-1]].max())
    bound = g_max / 128.0 + 1e-5
    err = np.abs(rgba[0, ..., :3] - want)[hit].max()
    # the same vertices interpolated in screen space
    p = V @ QUAD_R.T + QUAD_T
    xy = p[:, :2] / p[:, 2:] * QUAD_F + np.asarray(QUAD_C)
    screen = np.zeros((H, W, 3))
    for t, (a, b, c) in enumerate(F):
        Tm = np.asarray([[xy[a, 0], xy[b, 0], xy[c, 0]], [xy[a, 1], xy[b, 1], xy[c, 1]], [1.0, 1.0, 1.0]])
        lam = np.linalg.solve(Tm, np.stack([i.ravel(), j.ravel(), np.ones(H * W)]).astype(np.float64)).T.reshape(H, W, 3)
        screen[ids[0] == t] = (lam @ C[[a, b, c]])[ids[0] == t]
    err_screen = np.abs(screen - want)[hit].max()
    print("perspective: covered", int(hit.sum()), "max error", float(err), "bound", float(bound), "screen-space error",
          float(err_screen))
    assert hit.sum() > 1500 and err <= bound
    assert err_screen > bound
    assert (rgba[0, ..., 3][hit] == 1.0).all()


def test_constant_colour_and_background():
    for name in ("icosphere_80", "fronto_quad", "torus"):
        V, F, views, W, H = CASES[name]()
        rgba, u8, depth, nz, ids, rec = R.shade_reference(V, F, np.ones((len(V), 3), np.float32), views, W, H)
        hit = ids >= 0
        assert hit.any() and (~hit).any()
        assert (rgba[hit] == 1.0).all() and (u8[hit] == 255).all()
        assert (rgba[~hit] == 0.0).all() and (u8[~hit] == 0).all() and (nz[~hit] == 0).all()
        assert rgba.dtype == np.float32 and u8.dtype == np.uint8 and nz.dtype == np.uint8 and u8.shape == hit.shape + (3,)


def test_colours_follow_the_vertex_exchange():
    C = np.asarray([(0.9, 0.1, 0.3), (0.2, 0.8, 0.5), (0.4, 0.6, 0.95)], np.float32)
    a = R.shade_reference(*CASES["top_left_ccw"]()[:2], C, *CASES["top_left_ccw"]()[2:])
    b = R.shade_reference(*CASES["top_left_cw"]()[:2], C, *CASES["top_left_cw"]()[2:])
    hit = a[4] >= 0
    assert hit.sum() == 15 and np.array_equal(hit, b[4] >= 0)
    assert ulps(a[0][hit], b[0][hit]).max() <= 4
    # and the image is not a constant: the corner pixel is the first vertex's colour, the others differ
    assert ulps(a[0][0, 1, 1, :3], C[0]).max() <= 4 and np.abs(a[0][0, 1, 5, :3] - C[0]).max() > 0.3


@pytest.mark.parametrize("name", sorted(CASES))
def test_depth_ids_and_records_are_the_rasterisers(name):
    V, F, views, W, H = CASES[name]()
    got = R.shade_reference(V, F, colours(len(V)), views, W, H)
    want = R.rasterize_reference(V, F, views, W, H)
    assert np.array_equal(got[2].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[4], want[1]) and np.array_equal(got[5], want[2])
    assert np.array_equal(got[3], (((got[2][..., 0] * np.float32(255.0)).astype(np.int64) & 255) != 0).astype(np.uint8))
    assert np.array_equal(got[0][..., 3], want[0][..., 3]) and got[0].min() >= 0.0 and got[0].max() <= 1.0


def test_the_restatement_is_vectorised():
    import time

    V, F, views, W, H = CASES["icosphere_1280"]()
    C = colours(len(V))
    ids = R.rasterize_reference(V, F, views, W, H)[1]
    t0 = time.perf_counter()
    R._shade_view(V.astype(np.float32), F, C, views[0], ids[0].reshape(-1), W)
    assert time.perf_counter() - t0 < 0.5  # one pass over the covered pixels, no loop over triangles or pixels


# ------------------------------------------------------------------------------------------------------------ the readers
def test_read_mesh_colors_round_trips(tmp_path):
    V, F = R.icosphere(1)
    V = V.astype(np.float32).astype(np.float64)
    C = colours(len(V)).astype(np.float64)
    M.write_ply(tmp_path / "a.ply", V, F, N=V, C=C)
    M.write_obj(tmp_path / "a.obj", V, F, C=C)
    M.write_obj(tmp_path / "plain.obj", V, F)
    M.write_ply(tmp_path / "plain.ply", V, F)
    with open(tmp_path / "b.ply", "wb") as f:  # binary_little_endian, uchar colours and an alpha
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
                b"element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(V), len(F)))
        c8 = np.rint(C * 255).astype(np.uint8)
        for v, c in zip(V, c8):
            f.write(struct.pack("<fffBBBB", *v, *c, 200))
        for t in F:
            f.write(struct.pack("<Biii", 3, *t))
    (tmp_path / "f.ply").write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                                    "property float z\nproperty float red\nproperty float green\nproperty float blue\n"
                                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                    "0 0 0 0.25 0.5 1\n1 0 0 0 0.125 0.75\n0 1 0 1 1 0\n3 0 1 2\n")
    for name, tol in (("a.ply", 1 / 255), ("a.obj", 5e-5), ("b.ply", 1 / 255)):
        V2, F2, C2 = R.read_mesh_colors(tmp_path / name)
        assert np.array_equal(F2, F) and np.array_equal(V2.astype(np.float32), V.astype(np.float32)), name
        assert C2.shape == C.shape and np.abs(C2 - C).max() <= tol and C2.min() >= 0 and C2.max() <= 1, name
        assert np.array_equal(R.read_mesh(tmp_path / name)[0], V2)
    assert np.array_equal(R.read_mesh_colors(tmp_path / "b.ply")[2], c8 / 255.0)
    assert R.read_mesh_colors(tmp_path / "f.ply")[2].tolist() == [[0.25, 0.5, 1.0], [0.0, 0.125, 0.75], [1.0, 1.0, 0.0]]
    for name in ("plain.obj", "plain.ply"):
        V2, F2, C2 = R.read_mesh_colors(tmp_path / name)
        assert C2 is None and np.array_equal(F2, F)


# ---------------------------------------------------------------------------------------------------------- look-at views
def box(sx, sy, sz, centre=(0.0, 0.0, 0.0)):
    return np.asarray([(x * sx, y * sy, z * sz) for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)]) + centre


@pytest.mark.parametrize("V", [box(0.2, 0.2, 0.2), box(0.3, 0.1, 0.1, centre=(0.4, -0.2, 0.1))])
@pytest.mark.parametrize("sub,n", [(0, 12), (1, 42), (2, 162)])
def test_look_at_views(V, sub, n):
    W, H, fx, fy, cx, cy = 64, 48, 70.0, 65.0, 31.5, 23.5
    views, poses = R.look_at_views(V, fx, fy, cx, cy, W, H, subdivisions=sub)
    assert views.shape == (n, 20) and views.dtype == np.float32 and poses.shape == (n, 4, 4) and poses.dtype == np.float64
    assert np.isfinite(views).all() and np.isfinite(poses).all()  # the poles (0, +-1, 0) of subdivisions >= 1 included
    centre = 0.5 * (V.min(0) + V.max(0))
    r = 0.5 * np.linalg.norm(V.max(0) - V.min(0))
    dist = max(r / np.sin(np.arctan(W / (2 * fx))), r / np.sin(np.arctan(H / (2 * fy))))
    dirs = R.icosphere(sub)[0]
    for T, rec, d in zip(poses, views, dirs):
        Rm, t = T[:3, :3], T[:3, 3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
        assert np.array_equal(T[3], [0, 0, 0, 1])
        assert np.abs(Rm @ centre + t - [0, 0, dist]).max() < 1e-12  # the centre projects to (cx, cy) at depth dist
        assert np.abs(-Rm.T @ t - (centre + dist * d)).max() < 1e-12  # the eye, in the icosphere's order
        assert np.array_equal(rec, R.pack_view(Rm, t, fx, fy, cx, cy, 1e-6, 1.0))
        p = V @ Rm.T + t
        x, y = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
        assert (p[:, 2] > 0).all() and x.min() >= -0.5 and x.max() <= W - 0.5 and y.min() >= -0.5 and y.max() <= H - 0.5
    assert any(abs(d[1]) > 0.999 for d in dirs) == (sub >= 1)


# ------------------------------------------------------------------------------------------------------------ the builder
def builder_inputs():
    V, F = R.icosphere(2)
    return V * 0.1, F, colours(len(V), seed=11)


BUILD = dict(width=64, height=48, focal=60.0, cx=32.0, cy=24.0, subdivisions=0)


def read_tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_the_builder_writes_a_loadable_reference(tmp_path):
    from PIL import Image

    from pixtrack_amd.geometry import Camera
    from pixtrack_amd.model3d import Model3D, extract_covisibility

    V, F, C = builder_inputs()
    out = tmp_path / "a"
    summary = D.build_reference_from_mesh(V, F, C, out, renderer=D.reference_renderer(V, F, C), **BUILD)
    model = Model3D(str(out / "ref"))
    names = [("%d.png" % k).zfill(8) for k in range(1, 13)]
    assert names[0] == "0001.png" and sorted(p.name for p in (out / "dataset/mapping").iterdir()) == names
    assert len(model.dbs) == 12 and [model.dbs[k].name for k in range(1, 13)] == ["mapping/" + n for n in names]
    cam = model.cameras[1]
    assert list(model.cameras) == [1] and cam.model == "SIMPLE_RADIAL" and (cam.width, cam.height) == (64, 48)
    assert cam.params.tolist() == [60.0, 32.0, 24.0, 0.0]
    assert summary["views"] == 12 and summary["points"] == len(model.points3D) > 100 and summary["track_min"] >= 3
    assert summary["vertices"] == len(V) and summary["triangles"] == len(F) and summary["points_per_image_min"] > 0

    c = Camera.from_colmap(cam)._data.double().numpy()
    views, poses = R.look_at_views(V, c[2], c[3], c[4], c[5], 64, 48, subdivisions=0)
    render = R.shade_reference(V, F, C, views, 64, 48)
    covis = extract_covisibility(model)
    for k in range(1, 13):
        im = model.dbs[k]
        assert np.abs(im.qvec2rotmat() - poses[k - 1][:3, :3]).max() < 1e-12 and np.array_equal(im.tvec, poses[k - 1][:3, 3])
        assert len(covis[k]) > 0 and len(im.xys) == len(im.point3D_ids) > 0
        assert len(set(im.point3D_ids.tolist())) == len(im.point3D_ids)
        ij = np.rint(im.xys - 0.5).astype(int)
        assert (render[4][k - 1][ij[:, 1], ij[:, 0]] >= 0).all()  # every observation lies on a covered pixel
        for idx, pid in enumerate(im.point3D_ids):  # image -> track
            pt = model.points3D[int(pid)]
            where = np.nonzero(pt.image_ids == k)[0]
            assert len(where) == 1 and pt.point2D_idxs[where[0]] == idx
            p = im.qvec2rotmat() @ pt.xyz + im.tvec
            assert np.abs(p[:2] / p[2] * 60.0 + [32.0, 24.0] - im.xys[idx]).max() < 1e-9
        png = np.asarray(Image.open(out / "dataset/mapping" / names[k - 1]))
        assert png.shape == (48, 64, 3) and np.array_equal(png, render[1][k - 1])
    for pid, pt in model.points3D.items():  # track -> image
        assert len(pt.image_ids) >= 3 and pt.error == 0.0 and np.array_equal(pt.xyz, V[pid - 1])
        assert np.array_equal(pt.rgb, np.rint(C[pid - 1].astype(np.float64) * 255))
        for iid, idx in zip(pt.image_ids, pt.point2D_idxs):
            assert model.dbs[int(iid)].point3D_ids[int(idx)] == pid
    # a second run writes identical bytes
    D.build_reference_from_mesh(V, F, C, tmp_path / "b", renderer=D.reference_renderer(V, F, C), **BUILD)
    assert read_tree(out) == read_tree(tmp_path / "b") and len(read_tree(out)) == 15


def test_the_builder_strides_and_filters(tmp_path):
    V, F, C = builder_inputs()
    s = D.build_reference_from_mesh(V, F, C, tmp_path / "s", renderer=D.reference_renderer(V, F, C), max_points=40,
                                    min_track=4, **BUILD)
    from pixtrack_amd.utils.colmap import read_model

    _, images, points = read_model(tmp_path / "s" / "ref")
    assert 0 < s["points"] == len(points) <= 40 and all(len(p.image_ids) >= 4 for p in points.values())
    assert all(set(im.point3D_ids.tolist()) <= set(points) for im in images.values())
    with pytest.raises(ValueError):
        D.build_reference_from_mesh(V, F, C[:-1], tmp_path / "t", renderer=D.reference_renderer(V, F, C), **BUILD)


def test_the_command_line_refuses_a_mesh_without_colours(tmp_path):
    from pixtrack_amd import _lib

    V, F = R.icosphere(0)
    M.write_obj(tmp_path / "plain.obj", V, F)
    with pytest.raises(_lib.PxtError, match="colours"):
        D.main(["--mesh", str(tmp_path / "plain.obj"), "--out_dir", str(tmp_path / "o")])


# ----------------------------------------------------------------------------------------------------------- declarations
def test_the_op_and_the_entry_point_are_declared():
    from pixtrack_amd import _lib, ops

    assert "mesh_render" in ops.op_names() and "pxt_mesh_render" in _lib.PROTOTYPES
    L = _lib.lib()
    assert "pxt_mesh_render" not in L._pxt_missing

    def call(vertices=16, nv=1, colors=16, rgba=None, u8=None, depth=None, nz=None, tri=None, rec=16, ws=32, w=4, h=4):
        return L.pxt_mesh_render(vertices, nv, 16, 1, colors, 16, 1, w, h, rgba, u8, depth, nz, tri, rec, ws, None)

    # a failed check launches nothing: these return before any HIP call, on a machine without a GPU too
    assert call() == -1                      # every output NULL
    assert call(rgba=24) == -1 and call(depth=8) == -1 and call(depth=16, ws=24) == -1  # 16-byte alignment
    assert call(u8=18) == -1 and call(nz=17) == -1 and call(tri=6) == -1 and call(depth=16, colors=18) == -1
    assert call(depth=16, colors=None) == -1 and call(depth=16, vertices=None) == -1 and call(depth=16, rec=None) == -1
    assert call(depth=16, ws=None) == -1 and call(depth=16, nv=0) == -1 and call(u8=16, w=0) == -1
    assert call(nz=16, w=1 << 13, h=(1 << 13) + 1) == -1


def test_the_renderer_refuses_bad_colours():
    from pixtrack_amd import _lib

    V, F = R.icosphere(0)
    for bad in (np.full((12, 3), 1.5), np.full((12, 3), -0.1), np.full((12, 3), np.nan), np.zeros((11, 3))):
        with pytest.raises(_lib.PxtError, match="colors"):
            R.MeshRenderer(V, F, "cuda:0", colors=bad)
