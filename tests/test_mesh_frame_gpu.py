"""pxt_mesh_render_frame against mesh_render.frame_reference: bit for bit on every output and record, vertex colours and
a texture map.  No tolerance and no excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_render as R
from test_mesh_raster_gpu import BIG_VIEW, big_quad
from test_mesh_raster_host import SPHERE_VIEW, rotation, view
from test_mesh_shade_gpu import bits
from test_mesh_shade_host import colours
from test_mesh_texture_host import corner_uvs, random_texture

pytestmark = pytest.mark.gpu

SHADINGS = ("colors", "texture")


def shading_of(kind, V, F, seed=7):
    if kind == "colors":
        return {"colors": colours(len(V), seed)}
    UV, FUV = corner_uvs(len(F), seed)
    return {"uvs": UV, "triangle_uvs": FUV, "texture": random_texture()}


def renderer(device, V, F, shading):
    return R.MeshRenderer(V, F, device, **shading)


def gpu_frame(device, V, F, shading, requests, r=None):
    out = (r or renderer(device, V, F, shading)).render_frame(requests)
    torch.cuda.synchronize(device)
    return [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()} for o in out]


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def compare(device, V, F, kind, requests):
    shading = shading_of(kind, V, F)
    want = R.frame_reference(V, F, shading, requests)
    got = gpu_frame(device, V, F, shading, requests)
    assert len(got) == len(want) == len(requests)
    for g, w in zip(got, want):
        same(g, w)
    return want


def sphere_view(W, H, k=0, **kw):
    return view(**{**dict(fx=60.0, fy=58.0, cx=(W - 1) / 2 + 0.3 + 0.2 * k, cy=(H - 1) / 2 - 0.4, t=(0.01, -0.02, 0.45 + 0.1 * k)), **kw})


@pytest.mark.parametrize("kind", SHADINGS)
def test_mixed_sizes_in_one_call(device, kind):
    # different sizes, odd widths, byte-plane tails (37 * 29 and 23 * 41 are odd)
    V, F = R.icosphere(2)
    want = compare(device, V * 0.1, F, kind,
                   [(sphere_view(37, 29), 37, 29, 1, ("depth_nz", "depth", "rgb_u8")),
                    (sphere_view(23, 41, 1), 23, 41, 2, ("rgb_u8", "rgba"))])
    assert want[0]["records"][R.W_COVERED] > 300 and want[0]["depth_nz"].sum() > 300
    alpha = want[1]["rgba"][..., 3]
    assert ((alpha > 0) & (alpha < 1)).sum() > 20 and want[1]["records"][R.W_COVERED] == round(float(alpha.sum()) * 4)


@pytest.mark.parametrize("kind", SHADINGS)
@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (41, 1), (7, 5)])
def test_supersample_4_on_small_images(device, kind, W, H):
    V, F = R.icosphere(2)
    want = compare(device, V * 0.1, F, kind, [(sphere_view(W, H, k), W, H, 4, ("rgba", "rgb_u8")) for k in range(3)])
    assert all(w["records"][R.W_COVERED] >= 1 for w in want)


@pytest.mark.parametrize("kind", SHADINGS)
def test_large_triangles_clipped_on_all_four_sides(device, kind):
    V, F = big_quad()  # the list path on the fine lattice
    want = compare(device, V, F, kind, [(view(**BIG_VIEW), 70, 66, 4, ("rgba", "rgb_u8"))])
    assert want[0]["records"][R.W_COVERED] == 16 * 70 * 66 and (want[0]["rgba"][..., 3] == 1.0).all()


@pytest.mark.parametrize("kind", SHADINGS)
def test_micro_triangles(device, kind):
    V, F = R.icosphere(5)
    v = view(Rm=rotation(2), fx=115.0, fy=113.0, cx=47.3, cy=39.6, t=(0.01, -0.02, 0.45))
    want = compare(device, V * 0.1, F, kind, [(v, 96, 80, 2, ("rgba", "rgb_u8"))])
    assert want[0]["records"][R.W_DRAWN] == 20480 and want[0]["records"][R.W_COVERED] > 6000


@pytest.mark.parametrize("kind", SHADINGS)
def test_supersample_1_is_the_existing_call(device, kind):
    V, F = R.icosphere(3)
    V = V * 0.1
    shading = shading_of(kind, V, F)
    r = renderer(device, V, F, shading)
    views = np.stack([sphere_view(63, 47, k, Rm=rotation(k)) for k in range(2)])
    names = ("rgba", "rgb_u8", "depth", "depth_nz")
    old = r.render(views, 63, 47, want=names)
    got = gpu_frame(device, V, F, shading, [(views[k], 63, 47, 1, names) for k in range(2)], r=r)
    for k in range(2):
        for n in names:
            assert np.array_equal(bits(got[k][n]), bits(old[n][k].cpu().numpy())), (k, n)
        assert np.array_equal(got[k]["records"], old["records"][k]) and got[k]["records"][R.W_COVERED] > 300


@pytest.mark.parametrize("kind", SHADINGS)
def test_views_of_one_call_equal_their_solo_calls_in_two_orders(device, kind):
    V, F = R.icosphere(3)
    V = V * 0.1
    shading = shading_of(kind, V, F)
    r = renderer(device, V, F, shading)
    requests = [(sphere_view(63, 47, 0, Rm=rotation(1)), 63, 47, 1, ("rgba", "rgb_u8", "depth", "depth_nz")),
                (sphere_view(31, 22, 1, fx=40.0, fy=41.0, Rm=rotation(2)), 31, 22, 4, ("rgba", "rgb_u8")),
                (sphere_view(17, 45, 2, fx=50.0, fy=47.0), 17, 45, 2, ("rgb_u8", "rgba"))]
    solo = [gpu_frame(device, V, F, shading, [q], r=r)[0] for q in requests]
    for s, w in zip(solo, R.frame_reference(V, F, shading, requests)):
        same(s, w)
        assert s["records"][R.W_COVERED] > 100
    for order in ([0, 1, 2], [2, 0, 1]):
        got = gpu_frame(device, V, F, shading, [requests[p] for p in order], r=r)
        for k, p in enumerate(order):
            same(got[k], solo[p])


@pytest.mark.parametrize("kind", SHADINGS)
def test_a_non_finite_view_draws_nothing_and_its_neighbour_is_intact(device, kind):
    V, F = R.icosphere(2)
    good = sphere_view(23, 41)
    bad = good.copy()
    bad[13] = np.inf
    want = compare(device, V * 0.1, F, kind, [(bad, 19, 13, 2, ("rgba", "rgb_u8")), (good, 23, 41, 2, ("rgba", "rgb_u8")),
                                             (bad, 9, 11, 1, ("depth", "depth_nz", "rgb_u8"))])
    for p in (0, 2):
        assert want[p]["records"][R.W_STATUS] == 0xFFFFFFFF and (want[p]["records"][:7] == 0).all()
        assert all((want[p][k] == 0).all() for k in want[p] if k != "records")
    assert want[1]["records"][R.W_STATUS] == 0 and want[1]["records"][R.W_COVERED] > 1500


def test_bad_arguments_are_refused_and_nothing_is_written(device):
    L = _lib.lib()
    V, F = R.icosphere(0)
    C = colours(len(V))
    r = R.MeshRenderer(V, F, device, colors=C)
    P, (W0, H0), (W1, H1, S1) = 2, (15, 11), (9, 7, 2)
    geometry = [W0, H0, 1, W1, H1, S1]
    views = np.stack([view(**{**SPHERE_VIEW, "cx": 7.3, "cy": 5.1, "fx": 20.0, "fy": 20.0}),
                      view(**{**SPHERE_VIEW, "cx": 4.3, "cy": 3.1, "fx": 12.0, "fy": 12.0})])
    vt = torch.from_numpy(views).to(device)
    n0, n1 = W0 * H0, W1 * H1
    off_u8_1 = (n0 * 3 + 3) // 4 * 4
    offsets = [0, 0, 0, 0, n0 * 16, off_u8_1, -1, -1]
    sizes = [(n0 + n1) * 16, off_u8_1 + n1 * 3, n0 * 16, n0]
    big = [1 << 13, (1 << 13) // 4 + 1, 4]  # a fine lattice over 2^26
    need = int(L.pxt_mesh_render_frame_workspace_bytes(P, len(F), (_lib.C.c_int32 * 6)(*geometry)))
    assert need > 0
    assert L.pxt_mesh_render_frame_workspace_bytes(1, len(F), (_lib.C.c_int32 * 3)(*big)) == -1
    assert L.pxt_mesh_render_frame_workspace_bytes(1, len(F), (_lib.C.c_int32 * 3)(8, 8, 3)) == -1
    assert L.pxt_mesh_render_frame_workspace_bytes(9, len(F), (_lib.C.c_int32 * 27)(*([8, 8, 1] * 9))) == -1
    outs = dict(rgba=torch.empty(sizes[0] // 4 + 8, dtype=torch.float32, device=device),
                u8=torch.empty(sizes[1] + 8, dtype=torch.uint8, device=device),
                depth=torch.empty(sizes[2] // 4 + 8, dtype=torch.float32, device=device),
                nz=torch.empty(sizes[3] + 8, dtype=torch.uint8, device=device),
                rec=torch.empty(9 * 16, dtype=torch.int32, device=device),
                ws=torch.empty(need + 32, dtype=torch.uint8, device=device))
    for t in outs.values():
        t.view(torch.uint8).fill_(0xAB)
    stream = _lib.stream_ptr(device)
    ptr = {k: t.data_ptr() for k, t in outs.items()}
    assert all(p % 16 == 0 for p in ptr.values())
    views9 = torch.from_numpy(np.concatenate([views] * 5)).to(device)

    def call(p=P, geo=geometry, off=offsets, cap=None, colors=r.colors.data_ptr(), uvs=None, nv=len(V), nt=len(F), **over):
        a = {**ptr, **over}
        cap = [t.numel() * t.element_size() for t in (outs["rgba"], outs["u8"], outs["depth"], outs["nz"])] if cap is None else cap
        return L.pxt_mesh_render_frame(r.vertices.data_ptr(), nv, r.triangles.data_ptr(), nt, colors, uvs, 0, None, None, 0, 0,
                                       views9.data_ptr(), p, (_lib.C.c_int32 * len(geo))(*geo), (_lib.C.c_int64 * len(off))(*off),
                                       a["rgba"], a["u8"], a["depth"], a["nz"], (_lib.C.c_int64 * 4)(*cap), a["rec"], a["ws"], stream)

    def with_offsets(view_index, k, value):
        o = list(offsets)
        o[4 * view_index + k] = value
        return o

    bad = [dict(off=with_offsets(1, 2, 0)), dict(off=with_offsets(1, 3, 0)),             # depth outputs with S > 1
           dict(geo=[W0, H0, 1, W1, H1, 3]), dict(geo=[W0, H0, 0, W1, H1, 2]),             # S = 3, S = 0
           dict(p=9, geo=[4, 4, 1] * 9, off=[0, -1, -1, -1] * 9), dict(p=0),               # P = 9, P = 0
           dict(p=1, geo=big, off=[-1, 0, -1, -1]),                                        # over 2^26 fine pixels
           dict(geo=[0, H0, 1, W1, H1, 2]), dict(geo=[W0, -3, 1, W1, H1, 2]),
           dict(off=[0, 0, 0, 0, -1, -1, -1, -1]),                                         # a view without output
           dict(off=with_offsets(1, 0, n0 * 16 + 8)), dict(off=with_offsets(1, 1, off_u8_1 + 2)),  # offsets off their alignment
           dict(off=with_offsets(0, 3, 2)),
           dict(cap=[sizes[0] - 16, sizes[1], sizes[2], sizes[3]]), dict(cap=[sizes[0], sizes[1] - 1, sizes[2], sizes[3]]),
           dict(cap=[sizes[0], sizes[1], sizes[2], sizes[3] - 1]),                         # planes that do not fit
           dict(rgba=None), dict(nz=None), dict(rgba=ptr["rgba"] + 8), dict(u8=ptr["u8"] + 2), dict(nz=ptr["nz"] + 1),
           dict(depth=ptr["depth"] + 4), dict(ws=ptr["ws"] + 8), dict(ws=None), dict(rec=None), dict(colors=None),
           dict(uvs=r.colors.data_ptr()), dict(colors=r.colors.data_ptr() + 2), dict(nv=0), dict(nt=0), dict(nt=(1 << 24) + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == 0xAB).all(), name
    assert call(cap=sizes) == 0  # and the same buffers serve a good call, the capacities exactly the planes'
    torch.cuda.synchronize(device)
    want = R.frame_reference(V, F, {"colors": C}, [(views[0], W0, H0, 1, R.FRAME_OUTPUTS), (views[1], W1, H1, 2, ("rgba", "rgb_u8"))])
    assert want[0]["records"][R.W_COVERED] > 20 and want[1]["records"][R.W_COVERED] > 20
    rec = outs["rec"].cpu().numpy().view(np.uint32)
    assert np.array_equal(rec[:32].reshape(2, 16), np.stack([w["records"] for w in want])) and (rec[32:] == 0xABABABAB).all()
    raw = {k: outs[k].cpu().numpy().view(np.uint8) for k in ("rgba", "u8", "depth", "nz")}
    planes = [("rgba", 0, 0, want[0]["rgba"]), ("u8", 0, 0, want[0]["rgb_u8"]), ("depth", 0, 0, want[0]["depth"]),
              ("nz", 0, 0, want[0]["depth_nz"]), ("rgba", n0 * 16, 1, want[1]["rgba"]), ("u8", off_u8_1, 1, want[1]["rgb_u8"])]
    written = {k: np.zeros(len(a), bool) for k, a in raw.items()}
    for name, o, _, w in planes:
        wb = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        assert np.array_equal(raw[name][o:o + len(wb)], wb), (name, o)
        written[name][o:o + len(wb)] = True
    for name in raw:  # nothing between or past the planes
        assert (raw[name][~written[name]] == 0xAB).all(), name


def test_the_op_and_render_frame_check_before_any_launch(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(0)
    r = R.MeshRenderer(V, F, device, colors=colours(len(V)))
    v = view(**SPHERE_VIEW)
    for q in ([(v, 16, 12, 3, ("rgb_u8",))], [(v, 16, 12, 2, ("depth_nz",))], [(v, 16, 12, 2, ("depth", "rgba"))],
              [(v, 16, 12, 1, ())], [(v, 16, 12, 1, ("ids",))], [(v, 0, 12, 1, ("rgba",))], [(v, 1 << 13, (1 << 11) + 1, 4, ("rgba",))],
              [(v, 4, 4, 1, ("rgba",))] * 9, []):
        with pytest.raises(_lib.PxtError):
            r.render_frame(q)
    with pytest.raises(_lib.PxtError, match="colours"):
        R.MeshRenderer(V, F, device).render_frame([(v, 16, 12, 1, ("rgba",))])
    W, H = 16, 12
    vt = torch.from_numpy(v[None]).to(device)
    u8 = torch.full((W * H * 3,), 0xAB, dtype=torch.uint8, device=device)
    rec = torch.empty(1, 16, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_render_frame_workspace_bytes(1, len(F), (_lib.C.c_int32 * 3)(W, H, 1))),
                     dtype=torch.uint8, device=device)
    good = dict(v=r.vertices, f=r.triangles, c=r.colors, uv=None, fuv=None, tex=None, views=vt, geo=[W, H, 1], off=[-1, 0, -1, -1],
                rgba=None, u8=u8, depth=None, nz=None, rec=rec, ws=ws)
    bad = [dict(c=None), dict(uv=torch.zeros(4, 2, device=device)), dict(c=r.colors.double()), dict(geo=[W, H, 3]), dict(geo=[W, H]),
           dict(off=[-1, -1, -1, -1]), dict(off=[-1, 2, -1, -1]), dict(off=[-1, 0, -1]), dict(u8=None), dict(u8=u8[:-1]),
           dict(u8=u8.int()), dict(off=[0, 0, -1, -1]), dict(ws=ws[:16]), dict(rec=rec[:, :8].contiguous()),
           dict(views=torch.cat([vt, vt])), dict(geo=[W, H, 2], off=[-1, 0, -1, 0], nz=torch.empty(W * H, dtype=torch.uint8, device=device)),
           dict(geo=[W, H, 1, W, H, 1], off=[-1, 0, -1, -1, -1, 0, -1, -1], views=torch.cat([vt, vt]),
                u8=torch.empty(2 * W * H * 3, dtype=torch.uint8, device=device))]  # overlapping planes
    for kw in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_render_frame(*{**good, **kw}.values())
    torch.cuda.synchronize(device)
    assert (u8 == 0xAB).all()
    ops.mesh_render_frame(*good.values())
    torch.cuda.synchronize(device)
    want = R.frame_reference(V, F, {"colors": colours(len(V))}, [(v, W, H, 1, ("rgb_u8",))])[0]
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), want["rgb_u8"]) and want["rgb_u8"].max() > 0
