"""pxt_mesh_render_frame_batch: views of several meshes in one chain, against mesh_render.frame_reference per view and
against the one-mesh call - bit for bit on every output and record.  No tolerance and no excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_render as R
from test_mesh_frame_gpu import same, shading_of, sphere_view
from test_mesh_raster_gpu import BIG_VIEW, big_quad
from test_mesh_raster_host import SPHERE_VIEW, rotation, view
from test_mesh_shade_host import colours

pytestmark = pytest.mark.gpu

ALL = ("rgba", "rgb_u8", "depth", "depth_nz")


def meshes():
    """(V, F, shading): 20 triangles with vertex colours; 1280 textured triangles (two workgroups of the triangle
    launch: the small meshes' views have a workgroup beyond their T); two large triangles (a list of two entries)."""
    Va, Fa = R.icosphere(0)
    Vb, Fb = R.icosphere(3)
    Vc, Fc = big_quad()
    return [(Va * 0.1, Fa, shading_of("colors", Va, Fa, 3)), (Vb * 0.1, Fb, shading_of("texture", Vb, Fb, 5)),
            (Vc, Fc, shading_of("colors", Vc, Fc, 11))]


def tracker_requests():
    """Per mesh a tracker frame's two views - depth_nz at S = 1, rgb_u8 at S = 2 (the quad: S = 4 at 70 x 66, the list path
    on the fine lattice) - of different sizes; one view asks for all four outputs."""
    return [[(sphere_view(37, 29), 37, 29, 1, ("depth_nz",)), (sphere_view(23, 41, 1), 23, 41, 2, ("rgb_u8",))],
            [(sphere_view(63, 47, 0, Rm=rotation(1)), 63, 47, 1, ALL), (sphere_view(31, 22, 1, fx=40.0, fy=41.0), 31, 22, 2, ("rgb_u8",))],
            [(view(**BIG_VIEW), 70, 66, 1, ("depth_nz",)), (view(**BIG_VIEW), 70, 66, 4, ("rgb_u8", "rgba"))]]


@pytest.fixture(scope="module")
def scene(device):
    """The three meshes, their renderers, the tracker requests and the numpy reference of those, computed once."""
    ms = meshes()
    reqs = tracker_requests()
    want = R.frame_batch_reference([(V, F, sh, q) for (V, F, sh), q in zip(ms, reqs)])
    for w in want:
        assert all(v["records"][R.W_COVERED] > 20 for v in w)
    assert want[2][1]["records"][R.W_COVERED] == 16 * 70 * 66
    return dict(meshes=ms, renderers=[R.MeshRenderer(V, F, device, **sh) for V, F, sh in ms], requests=reqs, want=want)


def host(outs):
    return [[{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()} for o in item] for item in outs]


def gpu_batch(device, items, **kw):
    out = R.render_frame_batch(items, **kw)
    torch.cuda.synchronize(device)
    return host(out)


def same_items(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            same(a, b)


class CountingOps:
    """Stands in for a renderer's op namespace: counts the batch calls it passes on."""

    def __init__(self, ops):
        self.ops, self.calls = ops, 0

    def mesh_render_frame_batch(self, *args):
        self.calls += 1
        return self.ops.mesh_render_frame_batch(*args)


def test_three_meshes_of_different_size_and_kind_in_one_call(device, scene):
    rs, reqs = scene["renderers"], scene["requests"]
    counting = CountingOps(rs[0]._ops)
    rs[0]._ops = counting
    try:
        got = gpu_batch(device, list(zip(rs, reqs)))
    finally:
        rs[0]._ops = counting.ops
    assert counting.calls == 1
    same_items(got, scene["want"])
    # ... and the one-mesh call per mesh
    for r, q, g in zip(rs, reqs, got):
        solo = r.render_frame(q)
        torch.cuda.synchronize(device)
        same_items([g], host([solo]))


def test_orders_and_solo_calls_give_the_same_planes(device, scene):
    rs, reqs, want = scene["renderers"], scene["requests"], scene["want"]
    for order in ([0, 1, 2], [2, 0, 1]):
        got = gpu_batch(device, [(rs[m], reqs[m]) for m in order])
        same_items(got, [want[m] for m in order])
    for m in range(3):  # each mesh alone, and its views in the other order
        same_items(gpu_batch(device, [(rs[m], reqs[m])]), [want[m]])
        same_items(gpu_batch(device, [(rs[m], reqs[m][::-1])]), [want[m][::-1]])


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (41, 1), (7, 5)])
def test_small_views_beside_a_large_view_of_another_mesh(device, scene, W, H):
    # the grid is the 96 x 80 view's: every workgroup of it beyond the small views' tiles and pixels exits
    (Va, Fa, sa), (Vb, Fb, sb) = scene["meshes"][:2]
    ra, rb = scene["renderers"][:2]
    small = [(sphere_view(W, H, k), W, H, S, ("rgba", "rgb_u8")) for k, S in enumerate((4, 2, 1))]
    large = [(view(Rm=rotation(2), fx=115.0, fy=113.0, cx=47.3, cy=39.6, t=(0.01, -0.02, 0.45)), 96, 80, 1, ("rgb_u8", "depth_nz"))]
    key = "large_reference"
    if key not in scene:
        scene[key] = R.frame_reference(Vb, Fb, sb, large)
        assert scene[key][0]["records"][R.W_COVERED] > 2000
    want = [R.frame_reference(Va, Fa, sa, small), scene[key]]
    assert all(w["records"][R.W_COVERED] >= 1 for w in want[0])
    same_items(gpu_batch(device, [(ra, small), (rb, large)]), want)
    same_items(gpu_batch(device, [(rb, large), (ra, small)]), want[::-1])


def test_the_tables_at_their_bounds(device, scene):
    # P = 32 views of 7 x 5 over M = 16 descriptors, which share the arrays of two meshes
    ms, rs = scene["meshes"], scene["renderers"]
    items, want = [], []
    for m in range(16):
        k = m % 2
        q = [(sphere_view(7, 5, m % 5, Rm=rotation(m)), 7, 5, 1, ("depth_nz", "depth") if m % 3 else ("depth_nz",)),
             (sphere_view(7, 5, m % 4, Rm=rotation(m + 1)), 7, 5, (1, 2, 4)[m % 3], ("rgb_u8", "rgba"))]
        items.append((rs[k], q))
        want.append(R.frame_reference(*ms[k], q))
    assert sum(len(q) for _, q in items) == _lib.PXT_MESH_BATCH_MAX_VIEWS and len(items) == _lib.PXT_MESH_BATCH_MAX_MESHES
    assert all(v["records"][R.W_COVERED] >= 1 for w in want for v in w)
    counting = CountingOps(rs[0]._ops)
    rs[0]._ops = counting
    try:
        got = gpu_batch(device, items)
    finally:
        rs[0]._ops = counting.ops
    assert counting.calls == 1
    same_items(got, want)


def test_seventeen_items_take_two_calls(device, scene):
    ms, rs = scene["meshes"], scene["renderers"]
    items, want = [], []
    for m in range(17):
        k = (0, 2)[m % 2]
        q = [(sphere_view(9, 6, m % 5, Rm=rotation(m)) if k == 0 else view(**BIG_VIEW), 9, 6, (2, 1)[m % 2], ("rgb_u8",))]
        items.append((rs[k], q))
        want.append(R.frame_reference(*ms[k], q))
    counting = CountingOps(rs[0]._ops)
    rs[0]._ops = counting
    try:
        ws = R.FrameBatchWorkspace()
        got = gpu_batch(device, items, workspace=ws)
        again = gpu_batch(device, items, workspace=ws)  # the cached plan, the same workspace
    finally:
        rs[0]._ops = counting.ops
    assert counting.calls == 4
    same_items(got, want)
    same_items(again, want)


def test_a_non_finite_view_draws_nothing_and_the_other_meshes_views_are_intact(device, scene):
    (Va, Fa, sa), (Vb, Fb, sb) = scene["meshes"][:2]
    ra, rb = scene["renderers"][:2]
    good = sphere_view(23, 41)
    bad = good.copy()
    bad[13] = np.inf
    qa = [(bad, 19, 13, 2, ("rgba", "rgb_u8")), (bad, 9, 11, 1, ("depth", "depth_nz", "rgb_u8"))]
    qb = [(good, 23, 41, 2, ("rgba", "rgb_u8"))]
    want = [R.frame_reference(Va, Fa, sa, qa), R.frame_reference(Vb, Fb, sb, qb)]
    for w in want[0]:
        assert w["records"][R.W_STATUS] == 0xFFFFFFFF and (w["records"][:7] == 0).all()
        assert all((w[k] == 0).all() for k in w if k != "records")
    assert want[1][0]["records"][R.W_STATUS] == 0 and want[1][0]["records"][R.W_COVERED] > 1500
    same_items(gpu_batch(device, [(ra, qa), (rb, qb)]), want)


def test_bad_arguments_are_refused_and_nothing_is_written(device, scene):
    L, C = _lib.lib(), _lib.C
    (Va, Fa, sa), (Vb, Fb, sb) = scene["meshes"][:2]
    ra, rb = scene["renderers"][:2]
    (W0, H0), (W1, H1, S1) = (15, 11), (9, 7, 2)
    geometry = [W0, H0, 1, W1, H1, S1]
    views = np.stack([view(**{**SPHERE_VIEW, "cx": 7.3, "cy": 5.1, "fx": 20.0, "fy": 20.0}),
                      view(**{**SPHERE_VIEW, "cx": 4.3, "cy": 3.1, "fx": 12.0, "fy": 12.0})])
    n0, n1 = W0 * H0, W1 * H1
    off_u8_1 = (n0 * 3 + 3) // 4 * 4
    offsets = [0, 0, 0, 0, n0 * 16, off_u8_1, -1, -1]
    sizes = [(n0 + n1) * 16, off_u8_1 + n1 * 3, n0 * 16, n0]
    big = [1 << 13, (1 << 13) // 4 + 1, 4]  # a fine lattice over 2^26
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)

    def ws_bytes(counts, vm, geo):
        return int(L.pxt_mesh_render_frame_batch_workspace_bytes(len(counts), i32(counts), len(vm), i32(vm), i32(geo)))

    need = ws_bytes([len(Fa), len(Fb)], [0, 1], geometry)
    assert need > 0
    assert ws_bytes([len(Fa)], [0], big) == -1 and ws_bytes([len(Fa)], [0], [8, 8, 3]) == -1
    assert ws_bytes([len(Fa)], [1], [8, 8, 1]) == -1 and ws_bytes([len(Fa)], [-1], [8, 8, 1]) == -1
    assert ws_bytes([0], [0], [8, 8, 1]) == -1 and ws_bytes([(1 << 24) + 1], [0], [8, 8, 1]) == -1
    assert ws_bytes([4] * 17, [0], [8, 8, 1]) == -1 and ws_bytes([4], [0] * 33, [8, 8, 1] * 33) == -1
    assert L.pxt_mesh_render_frame_batch_workspace_bytes(0, i32([4]), 1, i32([0]), i32([8, 8, 1])) == -1
    assert L.pxt_mesh_render_frame_batch_workspace_bytes(1, i32([4]), 0, i32([0]), i32([8, 8, 1])) == -1
    assert ws_bytes([4], [0] * 32, [8, 8, 1] * 32) > 0 and ws_bytes([4] * 16, [15], [8, 8, 1]) > 0
    outs = dict(rgba=torch.empty(sizes[0] // 4 + 8, dtype=torch.float32, device=device),
                u8=torch.empty(sizes[1] + 8, dtype=torch.uint8, device=device),
                depth=torch.empty(sizes[2] // 4 + 8, dtype=torch.float32, device=device),
                nz=torch.empty(sizes[3] + 8, dtype=torch.uint8, device=device),
                rec=torch.empty(34 * 16, dtype=torch.int32, device=device),
                ws=torch.empty(need + 32, dtype=torch.uint8, device=device))
    for t in outs.values():
        t.view(torch.uint8).fill_(0xAB)
    stream = _lib.stream_ptr(device)
    ptr = {k: t.data_ptr() for k, t in outs.items()}
    assert all(p % 16 == 0 for p in ptr.values())
    views33 = np.ascontiguousarray(np.concatenate([views] * 17)[:33])

    def desc(r, **over):
        d = _lib.MeshDesc()
        d.vertices, d.triangles, d.colors = r.vertices.data_ptr(), r.triangles.data_ptr(), _lib.dptr(r.colors)
        d.uvs, d.triangle_uvs, d.texture = _lib.dptr(r.uvs), _lib.dptr(r.triangle_uvs), _lib.dptr(r.texture)
        d.n_vertices, d.n_triangles = r.n_vertices, r.n_triangles
        if r.texture is not None:
            d.n_uvs, d.tex_width, d.tex_height = int(r.uvs.shape[0]), int(r.texture.shape[1]), int(r.texture.shape[0])
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def call(descs=None, m=None, vm=(0, 1), p=2, geo=geometry, off=offsets, cap=None, views_ptr=views33.ctypes.data, **over):
        a = {**ptr, **over}
        descs = [desc(ra), desc(rb)] if descs is None else descs
        arr = (_lib.MeshDesc * max(1, len(descs)))(*descs)
        cap = [t.numel() * t.element_size() for t in (outs["rgba"], outs["u8"], outs["depth"], outs["nz"])] if cap is None else cap
        return L.pxt_mesh_render_frame_batch(arr, len(descs) if m is None else m, i32(list(vm)), views_ptr, p, i32(geo),
                                             (C.c_int64 * len(off))(*off), a["rgba"], a["u8"], a["depth"], a["nz"],
                                             (C.c_int64 * 4)(*cap), a["rec"], a["ws"], stream)

    def with_offsets(view_index, k, value):
        o = list(offsets)
        o[4 * view_index + k] = value
        return o

    colors = ra.colors.data_ptr()
    bad = [dict(m=0), dict(descs=[desc(ra)] * 17, vm=(0, 16)), dict(vm=(0, 2)), dict(vm=(-1, 1)), dict(vm=(2, 0)),  # M, view_mesh
           dict(p=33, vm=[0] * 33, geo=[4, 4, 1] * 33, off=[0, -1, -1, -1] * 33), dict(p=0),                        # P = 33, P = 0
           dict(off=with_offsets(1, 2, 0)), dict(off=with_offsets(1, 3, 0)),             # depth outputs with S > 1
           dict(geo=[W0, H0, 1, W1, H1, 3]), dict(geo=[W0, H0, 0, W1, H1, 2]),             # S = 3, S = 0
           dict(p=1, vm=(0,), geo=big, off=[-1, 0, -1, -1]),                               # over 2^26 fine pixels
           dict(geo=[0, H0, 1, W1, H1, 2]), dict(geo=[W0, -3, 1, W1, H1, 2]),
           dict(off=[0, 0, 0, 0, -1, -1, -1, -1]),                                         # a view without output
           dict(off=with_offsets(1, 0, n0 * 16 + 8)), dict(off=with_offsets(1, 1, off_u8_1 + 2)),  # offsets off their alignment
           dict(off=with_offsets(0, 3, 2)),
           dict(cap=[sizes[0] - 16, sizes[1], sizes[2], sizes[3]]), dict(cap=[sizes[0], sizes[1] - 1, sizes[2], sizes[3]]),
           dict(cap=[sizes[0], sizes[1], sizes[2], sizes[3] - 1]),                         # planes that do not fit
           dict(rgba=None), dict(nz=None), dict(rgba=ptr["rgba"] + 8), dict(u8=ptr["u8"] + 2), dict(nz=ptr["nz"] + 1),
           dict(depth=ptr["depth"] + 4), dict(ws=ptr["ws"] + 8), dict(ws=None), dict(rec=None), dict(views_ptr=None),
           # per mesh, the named one and one that no view names: neither or both shading groups, half a texture group, ...
           dict(descs=[desc(ra, colors=None), desc(rb)]), dict(descs=[desc(ra, uvs=colors), desc(rb)]),
           dict(descs=[desc(ra), desc(rb, texture=None)]), dict(descs=[desc(ra), desc(rb, colors=colors)]),
           dict(descs=[desc(ra), desc(rb, n_uvs=0)]), dict(descs=[desc(ra), desc(rb, tex_width=16385)]),
           dict(descs=[desc(ra), desc(rb, tex_height=0)]), dict(descs=[desc(ra, colors=colors + 2), desc(rb)]),
           dict(descs=[desc(ra, n_vertices=0), desc(rb)]), dict(descs=[desc(ra, n_triangles=0), desc(rb)]),
           dict(descs=[desc(ra), desc(rb, n_triangles=(1 << 24) + 1)]), dict(descs=[desc(ra, vertices=None), desc(rb)]),
           dict(descs=[desc(ra), desc(rb, triangles=None)]),
           dict(descs=[desc(ra), desc(rb), desc(ra, colors=None)]), dict(descs=[desc(ra), desc(rb), desc(rb, n_vertices=0)])]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == 0xAB).all(), name
    # the same buffers serve a good call, the capacities exactly the planes'; a third mesh that no view names is allowed
    assert call(descs=[desc(ra), desc(rb), desc(rb)], cap=sizes) == 0
    torch.cuda.synchronize(device)
    want = [R.frame_reference(Va, Fa, sa, [(views[0], W0, H0, 1, R.FRAME_OUTPUTS)])[0],
            R.frame_reference(Vb, Fb, sb, [(views[1], W1, H1, 2, ("rgba", "rgb_u8"))])[0]]
    assert want[0]["records"][R.W_COVERED] > 20 and want[1]["records"][R.W_COVERED] > 20
    rec = outs["rec"].cpu().numpy().view(np.uint32)
    assert np.array_equal(rec[:32].reshape(2, 16), np.stack([w["records"] for w in want])) and (rec[32:] == 0xABABABAB).all()
    raw = {k: outs[k].cpu().numpy().view(np.uint8) for k in ("rgba", "u8", "depth", "nz")}
    planes = [("rgba", 0, want[0]["rgba"]), ("u8", 0, want[0]["rgb_u8"]), ("depth", 0, want[0]["depth"]),
              ("nz", 0, want[0]["depth_nz"]), ("rgba", n0 * 16, want[1]["rgba"]), ("u8", off_u8_1, want[1]["rgb_u8"])]
    written = {k: np.zeros(len(a), bool) for k, a in raw.items()}
    for name, o, w in planes:
        wb = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        assert np.array_equal(raw[name][o:o + len(wb)], wb), (name, o)
        written[name][o:o + len(wb)] = True
    for name in raw:  # nothing between or past the planes
        assert (raw[name][~written[name]] == 0xAB).all(), name
    assert (outs["ws"][need:] == 0xAB).all()  # nothing past the workspace the size function names


def test_the_op_and_render_frame_batch_check_before_any_launch(device, scene):
    from pixtrack_amd.ops import ops

    ra, rb = scene["renderers"][:2]
    Va, Fa, sa = scene["meshes"][0]
    v = view(**{**SPHERE_VIEW, "cx": 7.3, "cy": 5.1, "fx": 20.0, "fy": 20.0})
    for items in ([(ra, [(v, 16, 12, 3, ("rgb_u8",))])], [(ra, [(v, 16, 12, 2, ("depth_nz",))])], [(ra, [])],
                  [(ra, [(v, 4, 4, 1, ("rgba",))] * 33)], [(ra, [(v, 16, 12, 1, ("ids",))])],
                  [(R.MeshRenderer(Va, Fa, device), [(v, 16, 12, 1, ("rgba",))])]):
        with pytest.raises(_lib.PxtError):
            R.render_frame_batch(items)
    assert R.render_frame_batch([]) == []
    W, H = 16, 12
    vt = torch.from_numpy(np.stack([v, v]))
    u8 = torch.full((2 * W * H * 3,), 0xAB, dtype=torch.uint8, device=device)
    rec = torch.full((2, 16), -1, dtype=torch.int32, device=device)
    need = int(_lib.lib().pxt_mesh_render_frame_batch_workspace_bytes(
        2, (_lib.C.c_int32 * 2)(ra.n_triangles, rb.n_triangles), 2, (_lib.C.c_int32 * 2)(0, 1), (_lib.C.c_int32 * 6)(W, H, 1, W, H, 1)))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    good = dict(v=[ra.vertices, rb.vertices], f=[ra.triangles, rb.triangles], c=[ra.colors, None], uv=[None, rb.uvs],
                fuv=[None, rb.triangle_uvs], tex=[None, rb.texture], vm=[0, 1], views=vt, geo=[W, H, 1, W, H, 1],
                off=[-1, 0, -1, -1, -1, W * H * 3, -1, -1], rgba=None, u8=u8, depth=None, nz=None, rec=rec, ws=ws)
    bad = [dict(c=[None, None]), dict(uv=[rb.uvs, rb.uvs]), dict(c=[ra.colors]), dict(tex=[None, None]),
           dict(c=[ra.colors.double(), None]), dict(c=[ra.colors.cpu(), None]), dict(v=[ra.vertices.cpu(), rb.vertices]),
           dict(vm=[0, 2]), dict(vm=[0, -1]), dict(vm=[0]), dict(vm=[0, 1, 1]), dict(views=vt.to(device)), dict(views=vt[:1]),
           dict(views=vt.double()), dict(geo=[W, H, 3, W, H, 1]), dict(geo=[W, H, 1]),
           dict(off=[-1, -1, -1, -1, -1, 0, -1, -1]), dict(off=[-1, 2, -1, -1, -1, W * H * 3, -1, -1]),
           dict(off=[-1, 0, -1, -1, -1, 0, -1, -1]),  # overlapping planes
           dict(u8=None), dict(u8=u8[:-1]), dict(u8=u8.int()), dict(u8=u8.cpu()), dict(ws=ws[:16]), dict(ws=ws.cpu()),
           dict(rec=rec[:, :8].contiguous()), dict(rec=rec[:1]),
           dict(v=[], f=[], c=[], uv=[], fuv=[], tex=[]),
           dict(v=[ra.vertices] * 17, f=[ra.triangles] * 17, c=[ra.colors] * 17, uv=[None] * 17, fuv=[None] * 17, tex=[None] * 17,
                vm=[0, 16])]
    for kw in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_render_frame_batch(*{**good, **kw}.values())
    torch.cuda.synchronize(device)
    assert (u8 == 0xAB).all() and (rec == -1).all()
    ops.mesh_render_frame_batch(*good.values())
    torch.cuda.synchronize(device)
    want = [R.frame_reference(Va, Fa, sa, [(v, W, H, 1, ("rgb_u8",))])[0],
            R.frame_reference(*scene["meshes"][1], [(v, W, H, 1, ("rgb_u8",))])[0]]
    got = u8.cpu().numpy().reshape(2, H, W, 3)
    assert np.array_equal(got[0], want[0]["rgb_u8"]) and np.array_equal(got[1], want[1]["rgb_u8"])
    assert want[0]["rgb_u8"].max() > 0 and want[1]["rgb_u8"].max() > 0
