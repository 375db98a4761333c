"""pxt_mesh_render_textured against mesh_render.shade_textured_reference: bit for bit on all five outputs and the
records, and on depth, ids, records and depth_nz against pxt_mesh_render and pxt_mesh_raster.  No tolerance and no
excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_dataset as D
from pixtrack_amd import mesh_render as R
from test_mesh_raster_gpu import BIG_VIEW, big_quad, three_views
from test_mesh_raster_host import CASES, SPHERE_VIEW, rotation, view
from test_mesh_shade_gpu import ALL, SUBSETS, bits, same
from test_mesh_shade_host import BUILD, colours, read_tree
from test_mesh_texture_host import corner_uvs, random_texture, textured_builder_inputs

pytestmark = pytest.mark.gpu

SHAPES = {"rgba": (4, torch.float32), "rgb_u8": (3, torch.uint8), "depth": (4, torch.float32), "depth_nz": (None, torch.uint8),
          "ids": (None, torch.int32)}


def gpu_render(device, V, F, UV, FUV, tex, views, W, H, want=ALL):
    out = R.MeshRenderer(V, F, device, uvs=UV, triangle_uvs=FUV, texture=tex).render(views, W, H, want=want)
    torch.cuda.synchronize(device)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def reference(V, F, UV, FUV, tex, views, W, H):
    return dict(zip(ALL + ("records",), R.shade_textured_reference(V, F, UV, FUV, tex, views, W, H)))


def compare(device, V, F, views, W, H, tex=None, seed=7):
    UV, FUV = corner_uvs(len(F), seed)
    tex = random_texture() if tex is None else tex
    want = reference(V, F, UV, FUV, tex, views, W, H)
    got = gpu_render(device, V, F, UV, FUV, tex, views, W, H)
    same(got, want)
    return want, got


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_host_case(device, name):
    compare(device, *CASES[name]())


def test_micro_triangles(device):
    V, F = R.icosphere(5)
    want, _ = compare(device, V * 0.1, F, view(Rm=rotation(2), fx=115.0, fy=113.0, cx=47.3, cy=39.6, t=(0.01, -0.02, 0.45))[None],
                      96, 80)
    assert want["records"][0, R.W_DRAWN] == 20480 and want["records"][0, R.W_COVERED] > 1500


def test_large_triangles_clipped_on_all_four_sides(device):
    V, F = big_quad()
    want, _ = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    assert want["records"][0, R.W_COVERED] == 70 * 66 and (want["rgba"][..., 3] == 1.0).all()
    assert len(np.unique(want["rgb_u8"].reshape(-1, 3), axis=0)) > 100


def test_large_and_small_triangles_in_one_call(device):
    Vq, Fq = big_quad(0.8)
    Vs, Fs = R.icosphere(4)
    Vs = Vs * 0.25 + np.asarray([0.2, -0.1, 0.6])
    V, F = np.concatenate([Vs, Vq]), np.concatenate([Fs, Fq + len(Vs)])
    want, _ = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    assert (want["ids"] >= 5120).any() and (want["ids"] < 5120).any() and (want["ids"] >= 0).all()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (41, 1), (7, 5)])
def test_small_images_tails_and_unaligned_view_offsets(device, W, H):
    V, F = R.icosphere(2)
    v = [view(fx=60.0, fy=60.0, cx=(W - 1) / 2 + 0.2 * k, cy=(H - 1) / 2 - 0.3, t=(0, 0, 0.5 + 0.1 * k)) for k in range(3)]
    want, _ = compare(device, V * 0.1, F, np.stack(v), W, H)
    assert (want["records"][:, R.W_COVERED] >= 1).all()
    Vq, Fq = big_quad()
    want, _ = compare(device, Vq, Fq, np.stack([view(fx=20.0, fy=20.0, cx=0.3 + k, cy=0.2) for k in range(3)]), W, H)
    assert (want["records"][:, R.W_COVERED] == W * H).all()


@pytest.mark.parametrize("Wt,Ht", [(1, 1), (1, 7), (64, 1), (257, 129)])
def test_texture_shapes(device, Wt, Ht):
    want, _ = compare(device, *CASES["fronto_quad"](), tex=random_texture(Wt, Ht, seed=Wt + Ht))
    assert want["records"][0, R.W_COVERED] > 500
    if Wt * Ht > 1:
        assert len(np.unique(want["rgb_u8"].reshape(-1, 3), axis=0)) > 10


def test_a_fourth_texture_byte_is_ignored(device):
    V, F, views, W, H = CASES["icosphere_80"]()
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    a = gpu_render(device, V, F, UV, FUV, tex, views, W, H)
    b = gpu_render(device, V, F, UV, FUV, np.dstack([tex, random_texture(seed=9)[..., 0]]), views, W, H)
    same(a, b)


def test_views_of_one_call_equal_their_solo_calls_in_any_order(device):
    V, F = R.icosphere(3)
    V = V * 0.1
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    views = three_views()
    solo = [gpu_render(device, V, F, UV, FUV, tex, views[p:p + 1], 63, 47) for p in range(3)]
    for p in range(3):
        same(solo[p], reference(V, F, UV, FUV, tex, views[p:p + 1], 63, 47))
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0, 1]):
        got = gpu_render(device, V, F, UV, FUV, tex, views[order], 63, 47)
        for k, p in enumerate(order):
            same({n: a[k:k + 1] for n, a in got.items()}, solo[p])


def out_buffers(device, P, H, W):
    shapes = {k: ((P, H, W) if c is None else (P, H, W, c), d) for k, (c, d) in SHAPES.items()}
    bufs = {k: torch.empty(s, dtype=d, device=device) for k, (s, d) in shapes.items()}
    for t in bufs.values():
        t.view(torch.uint8).fill_(0xAB)
    return bufs


def test_each_output_alone_and_in_pairs_from_dirty_buffers(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(3)
    V = V * 0.1
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    views, W, H, P = three_views(), 37, 29, 3  # W * H odd
    want = reference(V, F, UV, FUV, tex, views, W, H)
    r = R.MeshRenderer(V, F, device, uvs=UV, triangle_uvs=FUV, texture=tex)
    vt = torch.from_numpy(views).to(device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, len(F), W, H)), dtype=torch.uint8, device=device)
    for subset in SUBSETS:
        bufs = out_buffers(device, P, H, W)
        ws.fill_(0x5A)
        rec = torch.full((P, 16), -1, dtype=torch.int32, device=device)
        ops.mesh_render_textured(r.vertices, r.triangles, r.uvs, r.triangle_uvs, r.texture, vt, W, H,
                                 *[bufs[k] if k in subset else None for k in ALL], rec, ws)
        torch.cuda.synchronize(device)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32), want["records"]), subset
        for k in ALL:
            if k in subset:
                assert np.array_equal(bits(bufs[k].cpu().numpy()), bits(want[k])), (subset, k)
            else:
                assert (bufs[k].view(torch.uint8) == 0xAB).all(), (subset, k)


def test_the_raster_outputs_are_the_other_two_calls(device):
    V, F = R.icosphere(3)
    V = V * 0.1
    views, W, H = three_views(), 63, 47
    _, got = compare(device, V, F, views, W, H)
    colour = R.MeshRenderer(V, F, device, colors=colours(len(V))).render(views, W, H, want=ALL)
    depth, ids, rec = R.MeshRenderer(V, F, device).render_depth(views, W, H, triangle_ids=True)
    torch.cuda.synchronize(device)
    for k in ("depth", "depth_nz", "ids"):
        assert np.array_equal(bits(colour[k].cpu().numpy()), bits(got[k])), k
    assert np.array_equal(colour["records"], got["records"]) and np.array_equal(rec, got["records"])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), got["depth"].view(np.uint32))
    assert np.array_equal(ids.cpu().numpy(), got["ids"])
    assert np.array_equal(colour["rgba"].cpu().numpy()[..., 3], got["rgba"][..., 3])


def test_a_uv_index_outside_the_array_shades_black(device):
    from pixtrack_amd.ops import ops

    V, F, views, W, H = CASES["icosphere_80"]()
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    ids = R.rasterize_reference(V, F, views, W, H)[1]
    low, high = (int(t) for t in np.argsort(np.bincount(ids[ids >= 0], minlength=len(F)))[-2:])  # the two largest on screen
    FUV = FUV.copy()
    FUV[low, 1], FUV[high, 2] = -1, len(UV)
    want = reference(V, F, UV, FUV, tex, views, W, H)
    # the uvs handed over are the leading half of an allocation twice as long: no read could leave it, guard or not
    store = torch.zeros(2 * len(UV) + 8, 2, dtype=torch.float32, device=device)
    store[:len(UV)] = torch.from_numpy(UV).to(device)
    r = R.MeshRenderer(V, F, device)
    tex4 = torch.from_numpy(np.dstack([tex, np.zeros(tex.shape[:2], np.uint8)])).to(device)
    bufs = out_buffers(device, 1, H, W)
    rec = torch.empty(1, 16, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(1, len(F), W, H)), dtype=torch.uint8, device=device)
    ops.mesh_render_textured(r.vertices, r.triangles, store[:len(UV)], torch.from_numpy(FUV.astype(np.int32)).to(device),
                             tex4, torch.from_numpy(views).to(device), W, H, *[bufs[k] for k in ALL], rec, ws)
    torch.cuda.synchronize(device)
    got = {k: bufs[k].cpu().numpy() for k in ALL}
    got["records"] = rec.cpu().numpy().view(np.uint32)
    black = (got["ids"] == low) | (got["ids"] == high)
    assert (got["ids"] == low).sum() > 3 and (got["ids"] == high).sum() > 3
    assert (got["rgba"][black] == (0.0, 0.0, 0.0, 1.0)).all() and (got["rgb_u8"][black] == 0).all()
    assert (got["rgba"][~black & (got["ids"] >= 0)][:, :3].max(1) > 0).any()
    same(got, want)


def test_every_bound_is_refused_and_nothing_is_written(device):
    L = _lib.lib()
    V, F = R.icosphere(0)
    UV, FUV = corner_uvs(len(F))
    tex = random_texture()
    W, H, P = 15, 11, 2
    need = int(L.pxt_mesh_raster_workspace_bytes(P, len(F), W, H))
    views = np.stack([view(**{**SPHERE_VIEW, "cx": 7.3, "cy": 5.1, "fx": 20.0, "fy": 20.0})] * P)
    ins = dict(v=torch.from_numpy(V.astype(np.float32)).to(device), f=torch.from_numpy(F.astype(np.int32)).to(device),
               uv=torch.from_numpy(UV).to(device), fuv=torch.from_numpy(FUV.astype(np.int32)).to(device),
               tex=torch.from_numpy(np.dstack([tex, np.zeros(tex.shape[:2], np.uint8)])).to(device),
               views=torch.from_numpy(views).to(device))
    n = P * H * W
    outs = dict(rgba=torch.empty(n * 4 + 8, dtype=torch.float32, device=device),
                u8=torch.empty(n * 3 + 8, dtype=torch.uint8, device=device),
                depth=torch.empty(n * 4 + 8, dtype=torch.float32, device=device),
                nz=torch.empty(n + 8, dtype=torch.uint8, device=device),
                tri=torch.empty(n + 2, dtype=torch.int32, device=device),
                rec=torch.empty(P * 16, dtype=torch.int32, device=device),
                ws=torch.empty(need + 32, dtype=torch.uint8, device=device))
    for t in outs.values():
        t.view(torch.uint8).fill_(0xAB)
    stream = _lib.stream_ptr(device)
    ptr = {**{k: t.data_ptr() for k, t in ins.items()}, **{k: t.data_ptr() for k, t in outs.items()}}
    assert all(ptr[k] % 16 == 0 for k in ptr)

    def call(nv=len(V), nt=len(F), nuv=len(UV), tw=tex.shape[1], th=tex.shape[0], p=P, w=W, h=H, **over):
        a = {**ptr, **over}
        return L.pxt_mesh_render_textured(a["v"], nv, a["f"], nt, a["uv"], nuv, a["fuv"], a["tex"], tw, th, a["views"], p, w, h,
                                          a["rgba"], a["u8"], a["depth"], a["nz"], a["tri"], a["rec"], a["ws"], stream)

    bad = [dict(p=0), dict(p=4097), dict(nv=0), dict(nv=(1 << 24) + 1), dict(nt=0), dict(nt=(1 << 24) + 1), dict(w=0),
           dict(h=0), dict(w=1 << 13, h=(1 << 13) + 1), dict(w=-4), dict(depth=ptr["depth"] + 4), dict(depth=ptr["depth"] + 8),
           dict(rgba=ptr["rgba"] + 8), dict(u8=ptr["u8"] + 1), dict(u8=ptr["u8"] + 2), dict(nz=ptr["nz"] + 3),
           dict(tri=ptr["tri"] + 2), dict(ws=ptr["ws"] + 8), dict(v=None), dict(ws=None), dict(rec=None),
           dict(uv=None), dict(fuv=None), dict(tex=None), dict(uv=ptr["uv"] + 2), dict(fuv=ptr["fuv"] + 2),
           dict(tex=ptr["tex"] + 1), dict(tex=ptr["tex"] + 2), dict(nuv=0), dict(nuv=-1), dict(nuv=(1 << 24) + 1),
           dict(tw=0), dict(th=0), dict(tw=16385), dict(th=16385), dict(tw=-5),
           dict(rgba=None, u8=None, depth=None, nz=None, tri=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == 0xAB).all(), name
    assert call() == 0  # and the same buffers serve a good call
    torch.cuda.synchronize(device)
    want = reference(V, F, UV, FUV, tex, views, W, H)
    assert want["records"][0, R.W_COVERED] > 20
    assert np.array_equal(outs["rec"].cpu().numpy().view(np.uint32).reshape(P, 16), want["records"])
    for name, key, per in (("rgba", "rgba", 4), ("u8", "rgb_u8", 3), ("depth", "depth", 4), ("nz", "depth_nz", 1), ("tri", "ids", 1)):
        got = outs[name][:n * per].cpu().numpy().reshape(want[key].shape)
        assert np.array_equal(bits(got), bits(want[key])), name
        assert (outs[name][n * per:].view(torch.uint8) == 0xAB).all(), name  # nothing past the planes' ends


def test_the_op_refuses_host_tensors_wrong_dtypes_and_wrong_shapes(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(0)
    UV, FUV = corner_uvs(len(F))
    r = R.MeshRenderer(V, F, device, uvs=UV, triangle_uvs=FUV, texture=random_texture())
    views = torch.from_numpy(view(**SPHERE_VIEW)[None]).to(device)
    W, H = 16, 12
    u8 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=device)
    rec = torch.empty(1, 16, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(1, len(F), W, H)), dtype=torch.uint8, device=device)
    good = dict(v=r.vertices, f=r.triangles, uv=r.uvs, fuv=r.triangle_uvs, tex=r.texture, views=views, W=W, H=H, rgba=None,
                u8=u8, depth=None, nz=None, ids=None, rec=rec, ws=ws)
    ops.mesh_render_textured(*good.values())
    bad = [dict(uv=r.uvs.double()), dict(uv=torch.zeros(60, 3, device=device)), dict(uv=r.uvs[:0]), dict(fuv=r.triangle_uvs.long()),
           dict(fuv=r.triangle_uvs[:-1].contiguous()), dict(fuv=r.triangle_uvs.t().contiguous()), dict(tex=r.texture[..., :3].contiguous()),
           dict(tex=r.texture.int()), dict(tex=r.texture[:, :0].contiguous()), dict(tex=r.texture.permute(1, 0, 2)),
           dict(u8=u8[..., :2].contiguous()), dict(ws=ws[:16]), dict(u8=None), dict(W=0)]
    for kw in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_render_textured(*{**good, **kw}.values())
    for kw in (dict(uv=r.uvs.cpu()), dict(fuv=r.triangle_uvs.cpu()), dict(tex=r.texture.cpu())):
        with pytest.raises(RuntimeError):  # PxtError, unless the dispatcher objects to the mixed devices first
            ops.mesh_render_textured(*{**good, **kw}.values())


def test_the_builder_on_the_gpu_writes_the_reference_runs_files(device, tmp_path):
    V, F, UV, FUV, tex = textured_builder_inputs()
    kw = dict(uvs=UV, triangle_uvs=FUV, texture=tex)
    D.build_reference_from_mesh(V, F, None, tmp_path / "host", renderer=D.reference_renderer(V, F, **kw), **kw, **BUILD)
    s = D.build_reference_from_mesh(V, F, None, tmp_path / "gpu", device=device, views_per_call=5, **kw, **BUILD)
    a, b = read_tree(tmp_path / "host"), read_tree(tmp_path / "gpu")
    assert s["views"] == 12 and sorted(a) == sorted(b) and len(a) == 15
    for name in a:
        assert a[name] == b[name], name


def test_the_command_line_builds_from_a_textured_obj(device, tmp_path):
    from PIL import Image

    V, F, UV, FUV, tex = textured_builder_inputs()
    with open(tmp_path / "textured.obj", "w") as f:
        f.write("mtllib textured.mtl\nusemtl material_0\n")
        f.writelines("v %r %r %r\n" % tuple(map(float, v)) for v in V)
        f.writelines("vt %r %r\n" % tuple(map(float, uv)) for uv in UV)
        f.writelines("f %d/%d %d/%d %d/%d\n" % tuple(np.stack([t + 1, k + 1], 1).ravel()) for t, k in zip(F, FUV))
    (tmp_path / "textured.mtl").write_text("newmtl material_0\nmap_Kd texture_map.png\n")
    Image.fromarray(tex).save(str(tmp_path / "texture_map.png"))
    args = ["--mesh", str(tmp_path / "textured.obj"), "--width", "64", "--height", "48", "--focal", "60", "--cx", "32", "--cy", "24",
            "--subdivisions", "0", "--device", str(device)]
    D.main(args + ["--out_dir", str(tmp_path / "cli")])
    kw = dict(uvs=UV, triangle_uvs=FUV, texture=tex)
    D.build_reference_from_mesh(V, F, None, tmp_path / "host", renderer=D.reference_renderer(V, F, **kw), **kw, **BUILD)
    assert read_tree(tmp_path / "cli") == read_tree(tmp_path / "host")
    Image.fromarray(255 - tex).save(str(tmp_path / "other.png"))
    (tmp_path / "texture_map.png").unlink()  # --texture stands in for a map that is not there
    D.main(args + ["--out_dir", str(tmp_path / "over"), "--texture", str(tmp_path / "other.png")])
    a, b = read_tree(tmp_path / "cli"), read_tree(tmp_path / "over")
    assert sorted(a) == sorted(b) and a["dataset/mapping/0001.png"] != b["dataset/mapping/0001.png"]
    assert a["ref/images.bin"] == b["ref/images.bin"]
