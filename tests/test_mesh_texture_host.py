"""The texture rule of pxt_mesh_render_textured on the host: mesh_render.shade_textured_reference (the numpy restatement
the kernel is held to bit for bit in test_mesh_texture_gpu.py), the textured readers and the reference builder."""
import struct

import numpy as np
import pytest

from pixtrack_amd import mesh as M
from pixtrack_amd import mesh_dataset as D
from pixtrack_amd import mesh_render as R
from test_mesh_raster_host import CASES, on_plane, ulps, view
from test_mesh_shade_host import BUILD, QUAD_C, QUAD_F, QUAD_R, QUAD_T, read_tree


def corner_uvs(n_triangles, seed=7):
    """Seeded per-corner UVs in [-0.25, 1.25] (the clamp is exercised) -> (UV [3 T, 2] float32, FUV [T, 3])."""
    UV = np.random.default_rng(seed).uniform(-0.25, 1.25, size=(3 * n_triangles, 2)).astype(np.float32)
    return UV, np.arange(3 * n_triangles, dtype=np.int64).reshape(n_triangles, 3)


def random_texture(width=5, height=3, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(height, width, 3), dtype=np.uint8)


def sample(tex, u, v):
    """The rule in float64: row 0 is v = 1, corners aligned, bilinear, the border clamped."""
    Ht, Wt = tex.shape[:2]
    x, y = np.clip(u * (Wt - 1), 0, Wt - 1), np.clip((1.0 - v) * (Ht - 1), 0, Ht - 1)
    i0, j0 = np.floor(x).astype(int), np.floor(y).astype(int)
    i1, j1 = np.minimum(i0 + 1, Wt - 1), np.minimum(j0 + 1, Ht - 1)
    ax, ay = (x - i0)[..., None], (y - j0)[..., None]
    t = tex.astype(np.float64) / 255.0
    top = t[j0, i0] + ax * (t[j0, i1] - t[j0, i0])
    bot = t[j1, i0] + ax * (t[j1, i1] - t[j1, i0])
    return top + ay * (bot - top)


# --------------------------------------------------------------------------------------------------------------- the rule
def test_uvs_are_perspective_correct():
    V = np.asarray([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)])
    F = np.asarray([(0, 1, 2), (0, 2, 3)])
    UV = V[:, :2] + 0.5
    tex = np.zeros((256, 256, 3), np.uint8)
    tex[..., 0] = np.arange(256)[None, :]         # r = column: r is u
    tex[..., 1] = 255 - np.arange(256)[:, None]   # g = 255 - row: g is v
    W, H = 64, 48
    rgba, u8, depth, nz, ids, rec = R.shade_textured_reference(
        V, F, UV, F, tex, view(QUAD_F, QUAD_F, *QUAD_C, Rm=QUAD_R, t=QUAD_T)[None], W, H)
    hit = ids[0] >= 0
    j, i = np.mgrid[0:H, 0:W]
    d = np.stack([(i - QUAD_C[0]) / QUAD_F, (j - QUAD_C[1]) / QUAD_F, np.ones((H, W))], -1)
    s = (QUAD_R.T @ QUAD_T)[2] / (d @ QUAD_R)[..., 2]
    q = (s[..., None] * d - QUAD_T) @ QUAD_R
    want = q[..., :2] + 0.5
    g_max = max(np.abs(want[:, 1:] - want[:, :-1])[hit[:, 1:] & hit[:, :-1]].max(),
                np.abs(want[1:] - want[:-1])[hit[1:] & hit[:-1]].max())
    bound = g_max / 128.0 + 1e-5
    err = np.abs(rgba[0, ..., :2] - want)[hit].max()
    p = V @ QUAD_R.T + QUAD_T
    xy = p[:, :2] / p[:, 2:] * QUAD_F + np.asarray(QUAD_C)
    screen = np.zeros((H, W, 2))
    for t, (a, b, c) in enumerate(F):
        Tm = np.asarray([[xy[a, 0], xy[b, 0], xy[c, 0]], [xy[a, 1], xy[b, 1], xy[c, 1]], [1.0, 1.0, 1.0]])
        lam = np.linalg.solve(Tm, np.stack([i.ravel(), j.ravel(), np.ones(H * W)]).astype(np.float64)).T.reshape(H, W, 3)
        screen[ids[0] == t] = (lam @ UV[[a, b, c]])[ids[0] == t]
    err_screen = np.abs(screen - want)[hit].max()
    print("perspective uv: covered", int(hit.sum()), "max error", float(err), "bound", float(bound), "screen-space error",
          float(err_screen))
    assert hit.sum() > 1500 and err <= bound
    assert err_screen > bound
    assert (rgba[0, ..., 3][hit] == 1.0).all() and (rgba[0, ..., 2] == 0.0).all()


QUAD = on_plane([(1, 1), (6, 1), (6, 6), (1, 6)])
QUAD_FACES = np.asarray([(0, 1, 2), (0, 2, 3)])


def draw_quad(tex, u_at, v_at):
    """The 8 x 8 fronto-parallel quad whose covered pixels are i, j = 1..5; pixel i has u = u_at(i), pixel j v = v_at(j)
    (both affine) -> (rgba [8, 8, 4], rgb_u8, u [8, 8], v [8, 8], covered)."""
    UV = np.asarray([(u_at(1), v_at(1)), (u_at(6), v_at(1)), (u_at(6), v_at(6)), (u_at(1), v_at(6))])
    rgba, u8, _, _, ids, _ = R.shade_textured_reference(QUAD, QUAD_FACES, UV, QUAD_FACES, tex, view()[None], 8, 8)
    j, i = np.mgrid[0:8, 0:8]
    hit = ids[0] >= 0
    assert np.array_equal(hit, (i >= 1) & (i < 6) & (j >= 1) & (j < 6))
    return rgba[0], u8[0], u_at(i.astype(np.float64)), v_at(j.astype(np.float64)), hit


@pytest.mark.parametrize("Wt,Ht", [(2, 2), (3, 2)])
def test_texel_addressing(Wt, Ht):
    tex = (np.arange(Ht * Wt * 3, dtype=np.int64).reshape(Ht, Wt, 3) * 23 + 11).astype(np.uint8)
    assert len(np.unique(tex)) == tex.size
    tau = tex.astype(np.float32) / np.float32(255.0)
    # u = 0 at pixel 1 and u = 1 at pixel 5; v = 1 at pixel 1 and v = 0 at pixel 5
    rgba, u8, u, v, hit = draw_quad(tex, lambda i: (i - 1) / 4.0, lambda j: 1.0 - (j - 1) / 4.0)
    assert np.abs(rgba[..., :3] - sample(tex, u, v))[hit].max() < 1e-5
    assert np.abs(rgba[1, 1, :3] - tau[0, 0]).max() < 1e-6          # u = 0, v = 1: column 0 of row 0
    assert np.abs(rgba[1, 5, :3] - tau[0, Wt - 1]).max() < 1e-6     # u = 1: column Wt - 1
    assert np.abs(rgba[5, 1, :3] - tau[Ht - 1, 0]).max() < 1e-6     # v = 0: the last row
    assert np.abs(rgba[5, 5, :3] - tau[Ht - 1, Wt - 1]).max() < 1e-6
    if Wt == 3:
        assert np.abs(rgba[1, 3, :3] - tau[0, 1]).max() < 1e-6      # u = 0.5 is the middle column
    # UVs from -0.5 to 1.5: outside [0, 1] the border texels, exactly
    rgba, u8, u, v, hit = draw_quad(tex, lambda i: -0.5 + (i - 1) / 2.0, lambda j: 1.5 - (j - 1) / 2.0)
    assert u[0, 1] == -0.5 and u[0, 5] == 1.5 and v[1, 0] == 1.5 and v[5, 0] == -0.5
    assert np.abs(rgba[..., :3] - sample(tex, u, v))[hit].max() < 1e-5
    assert np.array_equal(rgba[1, 1, :3], tau[0, 0]) and np.array_equal(rgba[1, 5, :3], tau[0, Wt - 1])
    assert np.array_equal(rgba[5, 1, :3], tau[Ht - 1, 0]) and np.array_equal(rgba[5, 5, :3], tau[Ht - 1, Wt - 1])
    assert np.array_equal(u8[1, 1], R._u8(tau[0, 0])) and (np.abs(u8[1, 1].astype(int) - tex[0, 0]) <= 1).all()


def test_a_single_texel_colours_everything():
    tex = np.asarray([[[200, 17, 99]]], np.uint8)
    for u_at, v_at in ((lambda i: (i - 1) / 4.0, lambda j: 1.0 - (j - 1) / 4.0), (lambda i: 3.0 * i - 7.0, lambda j: -2.0 * j)):
        rgba, u8, u, v, hit = draw_quad(tex, u_at, v_at)
        tau = tex[0, 0].astype(np.float32) / np.float32(255.0)
        assert (rgba[hit][:, :3] == tau).all() and (rgba[hit][:, 3] == 1.0).all() and (rgba[~hit] == 0.0).all()
        assert (u8[hit] == R._u8(tau)).all() and (u8[~hit] == 0).all()


def test_uvs_follow_the_vertex_exchange():
    UV = np.asarray([(0.1, 0.9), (0.95, 0.8), (0.2, 0.05)], np.float32)
    tex = random_texture(4, 4, seed=5)
    Va, Fa, views, W, H = CASES["top_left_ccw"]()
    Vb, Fb, _, _, _ = CASES["top_left_cw"]()
    a = R.shade_textured_reference(Va, Fa, UV, Fa, tex, views, W, H)  # corner k carries its vertex's UV in both windings
    b = R.shade_textured_reference(Vb, Fb, UV, Fb, tex, views, W, H)
    hit = a[4] >= 0
    assert hit.sum() == 15 and np.array_equal(hit, b[4] >= 0)
    assert ulps(a[0][hit], b[0][hit]).max() <= 4
    # the image is not a constant: the corner pixel reads the first vertex's UV, others differ
    assert np.abs(a[0][0, 1, 1, :3] - sample(tex, np.float64(UV[0, 0]), np.float64(UV[0, 1]))).max() < 1e-5
    assert np.abs(a[0][0, 1, 5, :3] - a[0][0, 1, 1, :3]).max() > 0.1
    # exchanging the UV indices without the vertices is another image
    c = R.shade_textured_reference(Va, Fa, UV, Fb, tex, views, W, H)
    assert ulps(a[0][hit], c[0][hit]).max() > 1000


def test_a_seam_keeps_each_triangles_own_uvs():
    V, F, views, W, H = CASES["shared_edge"]()
    tex = np.zeros((1, 4, 3), np.uint8)
    tex[0, :2], tex[0, 2:] = (255, 0, 0), (0, 0, 255)  # the left half red, the right half blue
    # vertices 0 and 2 are shared; triangle 0 reads the left half through UVs 0-2, triangle 1 the right half through 3-5
    UV = np.asarray([(0.0, 0.5), (0.3, 0.5), (0.3, 0.2), (1.0, 0.5), (0.7, 0.2), (0.7, 0.5)], np.float32)
    FUV = np.asarray([(0, 1, 2), (3, 4, 5)])
    rgba, u8, _, _, ids, _ = R.shade_textured_reference(V, F, UV, FUV, tex, views, W, H)
    assert (ids[0] == 0).sum() == 15 and (ids[0] == 1).sum() == 10
    assert (u8[0][ids[0] == 0] == (255, 0, 0)).all() and (u8[0][ids[0] == 1] == (0, 0, 255)).all()
    # per-vertex UVs cannot say this: whichever of its two UVs a shared vertex keeps, one triangle crosses the halves
    for keep in ([0, 1, 2, 5], [3, 1, 4, 5]):
        flat = R.shade_textured_reference(V, F, UV[keep], F, tex, views, W, H)[1]
        assert not np.array_equal(flat, u8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_depth_ids_and_records_are_the_rasterisers(name):
    V, F, views, W, H = CASES[name]()
    UV, FUV = corner_uvs(len(F))
    got = R.shade_textured_reference(V, F, UV, FUV, random_texture(), views, W, H)
    want = R.rasterize_reference(V, F, views, W, H)
    assert np.array_equal(got[2].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[4], want[1]) and np.array_equal(got[5], want[2])
    assert np.array_equal(got[3], (((got[2][..., 0] * np.float32(255.0)).astype(np.int64) & 255) != 0).astype(np.uint8))
    assert np.array_equal(got[0][..., 3], want[0][..., 3]) and got[0].min() >= 0.0 and got[0].max() <= 1.0
    assert np.array_equal(got[1], R._u8(got[0][..., :3])) and got[0].dtype == np.float32 and got[1].dtype == np.uint8


def test_a_uv_index_outside_the_array_shades_black():
    V, F, views, W, H = CASES["shared_edge"]()
    UV, FUV = corner_uvs(2)
    tex = np.full((3, 5, 3), 255, np.uint8)
    for bad in (-1, len(UV)):
        FUV2 = FUV.copy()
        FUV2[1, 2] = bad
        rgba, u8, depth, nz, ids, rec = R.shade_textured_reference(V, F, UV, FUV2, tex, views, W, H)
        assert (rgba[0][ids[0] == 1] == (0.0, 0.0, 0.0, 1.0)).all() and (rgba[0][ids[0] == 0] == 1.0).all()
        assert (nz[0][ids[0] >= 0] == 1).all() and rec[0, R.W_INDEX] == 0


# ------------------------------------------------------------------------------------------------------------ the readers
OBJ_TEXT = """# a quad, a triangle with normals and a triangle by negative indices
mtllib skin.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.25
usemtl skin
f 1/2 2/3 3/4 4/1
v 0.5 2 0.25
vt 0.125 0.75
f 4/4/1 3/3/1 5/6/1
f -5/-6 -4/-5 -1/-2
"""
OBJ_V = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 2, 0.25)]
OBJ_UV = [(0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0.25), (0.125, 0.75)]
OBJ_F = [(0, 1, 2), (0, 2, 3), (3, 2, 4), (0, 1, 4)]
OBJ_FUV = [(1, 2, 3), (1, 3, 0), (3, 2, 5), (0, 1, 4)]


def write_textured_obj(folder, tex, text=OBJ_TEXT, mtl="newmtl skin\nKd 1 1 1\nmap_Kd tex.png\n"):
    from PIL import Image

    (folder / "textured.obj").write_text(text)
    (folder / "skin.mtl").write_text(mtl)
    Image.fromarray(tex).save(str(folder / "tex.png"))
    return folder / "textured.obj"


def test_read_mesh_textured_reads_an_obj_with_its_material(tmp_path):
    tex = random_texture(7, 4)
    path = write_textured_obj(tmp_path, tex)
    V, F, UV, FUV, image = R.read_mesh_textured(path)
    assert np.array_equal(V, OBJ_V) and np.array_equal(UV, OBJ_UV) and V.dtype == UV.dtype == np.float64
    assert np.array_equal(F, OBJ_F) and np.array_equal(FUV, OBJ_FUV) and F.dtype == FUV.dtype == np.int64
    assert image == tmp_path / "tex.png"
    got = R.read_texture(image)
    assert got.dtype == np.uint8 and np.array_equal(got, tex)
    assert np.array_equal(R.read_mesh(path)[1], F) and R.read_mesh_colors(path)[2] is None  # the older readers as before
    # an RGBA or a grey image comes back as RGB
    from PIL import Image

    Image.fromarray(np.dstack([tex, np.full(tex.shape[:2], 9, np.uint8)])).save(str(tmp_path / "rgba.png"))
    Image.fromarray(tex[..., 0]).save(str(tmp_path / "grey.png"))
    assert np.array_equal(R.read_texture(tmp_path / "rgba.png"), tex)
    assert np.array_equal(R.read_texture(tmp_path / "grey.png"), np.repeat(tex[..., :1], 3, 2))


def write_textured_plys(folder, V, F, UV):
    head = ("element vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
            "property float texture_u\nproperty float texture_v\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(V), len(F)))
    with open(folder / "a.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\ncomment TextureFile tex.png\n" + head)
        for v, uv in zip(V, UV):
            f.write("%r %r %r 0 %r %r\n" % (*map(float, v), *map(float, uv)))
        for t in F:
            f.write("3 %d %d %d\n" % tuple(t))
    with open(folder / "b.ply", "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\ncomment TextureFile tex.png\n" + head).encode())
        for v, uv in zip(V, UV):
            f.write(struct.pack("<ffffff", *v, 0.0, *uv))
        for t in F:
            f.write(struct.pack("<Biii", 3, *t))
    (folder / "st.ply").write_text(
        "ply\nformat ascii 1.0\ncomment TextureFile tex.png\nelement vertex 3\nproperty float x\nproperty float y\n"
        "property float z\nproperty float s\nproperty float t\nelement face 1\nproperty list uchar int vertex_indices\n"
        "end_header\n0 0 0 0.25 0.5\n1 0 0 0 0.125\n0 1 0 1 0.75\n3 0 1 2\n")


def test_read_mesh_textured_reads_plys_and_returns_none_without_texture(tmp_path):
    from PIL import Image

    V, F = R.icosphere(1)
    V = V.astype(np.float32).astype(np.float64)
    UV = np.random.default_rng(2).uniform(0, 1, size=(len(V), 2)).astype(np.float32).astype(np.float64)
    Image.fromarray(random_texture()).save(str(tmp_path / "tex.png"))
    write_textured_plys(tmp_path, V, F, UV)
    for name in ("a.ply", "b.ply"):
        V2, F2, UV2, FUV2, image = R.read_mesh_textured(tmp_path / name)
        assert np.array_equal(V2, V) and np.array_equal(F2, F) and np.array_equal(UV2, UV) and np.array_equal(FUV2, F), name
        assert image == tmp_path / "tex.png" and R.read_mesh_colors(tmp_path / name)[2] is None
    assert R.read_mesh_textured(tmp_path / "st.ply")[2].tolist() == [[0.25, 0.5], [0.0, 0.125], [1.0, 0.75]]
    C = np.random.default_rng(1).uniform(0, 1, size=V.shape)
    M.write_obj(tmp_path / "plain.obj", V, F)
    M.write_ply(tmp_path / "plain.ply", V, F)
    M.write_obj(tmp_path / "coloured.obj", V, F, C=C)
    M.write_ply(tmp_path / "coloured.ply", V, F, N=V, C=C)
    for name in ("plain.obj", "plain.ply", "coloured.obj", "coloured.ply"):
        assert R.read_mesh_textured(tmp_path / name) is None, name
    assert R.read_mesh_colors(tmp_path / "plain.obj")[2] is None and R.read_mesh_colors(tmp_path / "coloured.ply")[2] is not None


def test_read_mesh_textured_refuses_by_name(tmp_path):
    tex = random_texture()
    two = tmp_path / "two"
    two.mkdir()
    text = OBJ_TEXT.replace("f 4/4/1 3/3/1 5/6/1", "usemtl lid\nf 4/4/1 3/3/1 5/6/1")
    path = write_textured_obj(two, tex, text, "newmtl skin\nmap_Kd tex.png\nnewmtl lid\nmap_Kd lid.png\n")
    with pytest.raises(ValueError, match=r"several texture maps \(lid.png, tex.png\)"):
        R.read_mesh_textured(path)
    # two materials that share one map are one map
    (two / "skin.mtl").write_text("newmtl skin\nmap_Kd tex.png\nnewmtl lid\nmap_Kd tex.png\n")
    assert np.array_equal(R.read_mesh_textured(path)[3], OBJ_FUV)
    gone = tmp_path / "gone"
    gone.mkdir()
    path = write_textured_obj(gone, tex)
    (gone / "tex.png").unlink()
    with pytest.raises(ValueError, match="texture map .*tex.png is missing"):
        R.read_mesh_textured(path)
    assert R.read_mesh_textured(path, require_image=False)[4] == gone / "tex.png"  # the caller brings its own image
    (gone / "skin.mtl").unlink()
    with pytest.raises(ValueError, match="material library .*skin.mtl is missing"):
        R.read_mesh_textured(path)
    bare = tmp_path / "bare"
    bare.mkdir()
    path = write_textured_obj(bare, tex, OBJ_TEXT + "f 1 2 3\n")
    with pytest.raises(ValueError, match="line 19: a face without vt"):
        R.read_mesh_textured(path)
    (tmp_path / "u.ply").write_text(
        "ply\nformat ascii 1.0\ncomment TextureFile nowhere.png\nelement vertex 3\nproperty float x\nproperty float y\n"
        "property float z\nproperty float texture_u\nproperty float texture_v\nelement face 1\n"
        "property list uchar int vertex_indices\nend_header\n0 0 0 0 0\n1 0 0 1 0\n0 1 0 0 1\n3 0 1 2\n")
    with pytest.raises(ValueError, match="nowhere.png is missing"):
        R.read_mesh_textured(tmp_path / "u.ply")


# ------------------------------------------------------------------------------------------------------------ the builder
def textured_builder_inputs():
    V, F = R.icosphere(2)
    UV = np.random.default_rng(11).uniform(0.0, 1.0, size=(3 * len(F), 2)).astype(np.float32)
    return V * 0.1, F, UV, np.arange(3 * len(F)).reshape(-1, 3), random_texture(16, 8, seed=12)


def test_the_builder_writes_a_loadable_reference_from_a_textured_mesh(tmp_path):
    from PIL import Image

    from pixtrack_amd.geometry import Camera
    from pixtrack_amd.model3d import Model3D

    V, F, UV, FUV, tex = textured_builder_inputs()
    out = tmp_path / "a"
    kw = dict(uvs=UV, triangle_uvs=FUV, texture=tex)
    summary = D.build_reference_from_mesh(V, F, None, out, renderer=D.reference_renderer(V, F, **kw), **kw, **BUILD)
    model = Model3D(str(out / "ref"))
    names = [D.image_name(k) for k in range(1, 13)]
    assert sorted(p.name for p in (out / "dataset/mapping").iterdir()) == names and len(model.dbs) == 12
    assert summary["views"] == 12 and summary["points"] == len(model.points3D) > 100 and summary["track_min"] >= 3
    c = Camera.from_colmap(model.cameras[1])._data.double().numpy()
    views, poses = R.look_at_views(V, c[2], c[3], c[4], c[5], 64, 48, subdivisions=0)
    render = R.shade_textured_reference(V, F, UV, FUV, tex, views, 64, 48)
    for k in range(1, 13):
        png = np.asarray(Image.open(out / "dataset/mapping" / names[k - 1]))
        assert png.shape == (48, 64, 3) and np.array_equal(png, render[1][k - 1])
        ij = np.rint(model.dbs[k].xys - 0.5).astype(int)
        assert len(ij) > 0 and (render[4][k - 1][ij[:, 1], ij[:, 0]] >= 0).all()
    assert len(np.unique(render[1].reshape(-1, 3), axis=0)) > 50  # the images are textured, not flat
    # a point's colour: the nearest texel at the UV of its vertex's first corner
    for pid, pt in model.points3D.items():
        t, k = np.argwhere(F == pid - 1)[0]
        u, v = UV[FUV[t, k]].astype(np.float64)
        want = tex[int(np.rint((1.0 - v) * 7)), int(np.rint(u * 15))]
        assert np.array_equal(pt.rgb, want) and np.array_equal(pt.xyz, V[pid - 1])
    D.build_reference_from_mesh(V, F, None, tmp_path / "b", renderer=D.reference_renderer(V, F, **kw), **kw, **BUILD)
    assert read_tree(out) == read_tree(tmp_path / "b") and len(read_tree(out)) == 15
    with pytest.raises(ValueError, match="not both"):
        D.build_reference_from_mesh(V, F, np.zeros_like(V), tmp_path / "c", renderer=lambda *a: None, **kw, **BUILD)
    with pytest.raises(ValueError, match="uvs and texture"):
        D.build_reference_from_mesh(V, F, None, tmp_path / "c", renderer=lambda *a: None, **BUILD)


def test_the_command_line_still_refuses_a_mesh_with_neither(tmp_path):
    from pixtrack_amd import _lib

    V, F = R.icosphere(0)
    M.write_obj(tmp_path / "plain.obj", V, F)
    with pytest.raises(_lib.PxtError, match="colours"):
        D.main(["--mesh", str(tmp_path / "plain.obj"), "--out_dir", str(tmp_path / "o")])
    assert "--texture" in D.build_parser().format_help()


# ----------------------------------------------------------------------------------------------------------- declarations
def test_the_textured_op_and_entry_point_are_declared():
    from pixtrack_amd import _lib, ops

    assert "mesh_render_textured" in ops.op_names() and "pxt_mesh_render_textured" in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 13
    L = _lib.lib()
    assert "pxt_mesh_render_textured" not in L._pxt_missing and L.pxt_version() == 13

    def call(vertices=16, nv=1, uvs=16, nuv=1, fuv=16, tex=16, tw=4, th=4, rgba=None, u8=None, depth=None, nz=None,
             tri=None, rec=16, ws=32, w=4, h=4):
        return L.pxt_mesh_render_textured(vertices, nv, 16, 1, uvs, nuv, fuv, tex, tw, th, 16, 1, w, h, rgba, u8, depth, nz,
                                          tri, rec, ws, None)

    # a failed check launches nothing: these return before any HIP call, on a machine without a GPU too
    assert call() == -1                      # every output NULL
    assert call(rgba=24) == -1 and call(depth=8) == -1 and call(depth=16, ws=24) == -1  # 16-byte alignment
    assert call(u8=18) == -1 and call(nz=17) == -1 and call(tri=6) == -1
    assert call(depth=16, uvs=18) == -1 and call(depth=16, fuv=18) == -1 and call(depth=16, tex=17) == -1
    assert call(depth=16, tex=18) == -1 and call(depth=16, vertices=18) == -1
    assert call(depth=16, uvs=None) == -1 and call(depth=16, fuv=None) == -1 and call(depth=16, tex=None) == -1
    assert call(depth=16, vertices=None) == -1 and call(depth=16, rec=None) == -1 and call(depth=16, ws=None) == -1
    assert call(depth=16, tw=0) == -1 and call(depth=16, th=0) == -1 and call(depth=16, tw=16385) == -1
    assert call(depth=16, th=16385) == -1 and call(depth=16, tw=-1) == -1
    assert call(depth=16, nuv=0) == -1 and call(depth=16, nuv=(1 << 24) + 1) == -1 and call(depth=16, nv=0) == -1
    assert call(u8=16, w=0) == -1 and call(nz=16, w=1 << 13, h=(1 << 13) + 1) == -1


def test_the_renderer_refuses_bad_textured_inputs():
    from pixtrack_amd import _lib

    V, F = R.icosphere(0)
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    nan = UV.copy()
    nan[5, 1] = np.nan
    inf = UV.copy()
    inf[0, 0] = np.inf
    low, high = FUV.copy(), FUV.copy()
    low[3, 0], high[7, 2] = -1, len(UV)
    for kw, what in ((dict(uvs=nan, triangle_uvs=FUV, texture=tex), "uvs must be finite"),
                     (dict(uvs=inf, triangle_uvs=FUV, texture=tex), "uvs must be finite"),
                     (dict(uvs=UV, triangle_uvs=low, texture=tex), "triangle_uvs holds indices outside"),
                     (dict(uvs=UV, triangle_uvs=high, texture=tex), "triangle_uvs holds indices outside"),
                     (dict(uvs=UV, triangle_uvs=FUV[:-1], texture=tex), "triangle_uvs is"),
                     (dict(uvs=UV, texture=tex), "triangle_uvs is needed"),
                     (dict(uvs=UV, triangle_uvs=FUV), "needs uvs and texture"),
                     (dict(uvs=UV[:, :1], triangle_uvs=FUV, texture=tex), "uvs is"),
                     (dict(uvs=UV, triangle_uvs=FUV, texture=tex.astype(np.float32)), "texture is"),
                     (dict(uvs=UV, triangle_uvs=FUV, texture=tex[..., :2]), "texture is"),
                     (dict(uvs=UV, triangle_uvs=FUV, texture=tex, colors=np.zeros((12, 3))), "not both")):
        with pytest.raises(_lib.PxtError, match=what):
            R.MeshRenderer(V, F, "cuda:0", **kw)
