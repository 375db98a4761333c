"""pxt_mesh_render against mesh_render.shade_reference: bit for bit on all five outputs and the records, and on depth,
ids and records against pxt_mesh_raster.  No tolerance and no excluded pixel."""
import itertools

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_dataset as D
from pixtrack_amd import mesh_render as R
from test_mesh_raster_gpu import BIG_VIEW, big_quad, three_views
from test_mesh_raster_host import CASES, QUAD_DEPTH, SPHERE_VIEW, rotation, view
from test_mesh_shade_host import BUILD, builder_inputs, colours, read_tree

pytestmark = pytest.mark.gpu

ALL = ("rgba", "rgb_u8", "depth", "depth_nz", "ids")


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def gpu_render(device, V, F, C, views, W, H, want=ALL):
    out = R.MeshRenderer(V, F, device, colors=C).render(views, W, H, want=want)
    torch.cuda.synchronize(device)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def same(got, want, names=ALL + ("records",)):
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def reference(V, F, C, views, W, H):
    return dict(zip(ALL + ("records",), R.shade_reference(V, F, C, views, W, H)))


def compare(device, V, F, views, W, H, seed=7):
    C = colours(len(V), seed)
    want = reference(V, F, C, views, W, H)
    got = gpu_render(device, V, F, C, views, W, H)
    same(got, want)
    depth, ids, rec = R.MeshRenderer(V, F, device).render_depth(views, W, H, triangle_ids=True)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), got["depth"].view(np.uint32))
    assert np.array_equal(ids.cpu().numpy(), got["ids"]) and np.array_equal(rec, got["records"])
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_host_case(device, name):
    compare(device, *CASES[name]())


def test_micro_triangles(device):
    V, F = R.icosphere(5)
    want = compare(device, V * 0.1, F, view(Rm=rotation(2), fx=115.0, fy=113.0, cx=47.3, cy=39.6, t=(0.01, -0.02, 0.45))[None],
                   96, 80)
    assert want["records"][0, R.W_DRAWN] == 20480 and want["records"][0, R.W_COVERED] > 1500


def test_large_triangles_clipped_on_all_four_sides(device):
    V, F = big_quad()
    want = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    assert want["records"][0, R.W_COVERED] == 70 * 66 and (want["rgba"][..., 3] == 1.0).all()


def test_large_and_small_triangles_in_one_call(device):
    Vq, Fq = big_quad(0.8)
    Vs, Fs = R.icosphere(4)
    Vs = Vs * 0.25 + np.asarray([0.2, -0.1, 0.6])
    V, F = np.concatenate([Vs, Vq]), np.concatenate([Fs, Fq + len(Vs)])
    want = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    assert (want["ids"] >= 5120).any() and (want["ids"] < 5120).any() and (want["ids"] >= 0).all()


def test_more_large_triangles_than_the_list_holds(device):
    n = 1100
    z = 1.0 + 0.001 * ((np.arange(n) * 37) % n)
    V = np.stack([np.asarray([(-6.0, -3.0, 1.0), (7.0, -3.0, 1.0), (0.5, 9.0, 1.0)]) * zi for zi in z]).reshape(-1, 3)
    F = np.arange(3 * n).reshape(n, 3)
    want = compare(device, V, F, view(fx=12.0, fy=12.0, cx=19.6, cy=14.2)[None], 40, 30)
    assert (want["ids"][0] == int(np.argmin(z))).all()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (41, 1), (7, 5)])
def test_small_images_tails_and_unaligned_view_offsets(device, W, H):
    # P = 3: with W * H odd the byte planes of views 1 and 2 begin 1, 2 or 3 bytes past a dword
    V, F = R.icosphere(2)
    v = [view(fx=60.0, fy=60.0, cx=(W - 1) / 2 + 0.2 * k, cy=(H - 1) / 2 - 0.3, t=(0, 0, 0.5 + 0.1 * k)) for k in range(3)]
    want = compare(device, V * 0.1, F, np.stack(v), W, H)
    assert (want["records"][:, R.W_COVERED] >= 1).all()
    Vq, Fq = big_quad()
    want = compare(device, Vq, Fq, np.stack([view(fx=20.0, fy=20.0, cx=0.3 + k, cy=0.2) for k in range(3)]), W, H)
    assert (want["records"][:, R.W_COVERED] == W * H).all()


def test_views_of_one_call_equal_their_solo_calls_in_any_order(device):
    V, F = R.icosphere(3)
    V, C = V * 0.1, colours(642)
    views = three_views()
    solo = [gpu_render(device, V, F, C, views[p:p + 1], 63, 47) for p in range(3)]
    for p in range(3):
        same(solo[p], reference(V, F, C, views[p:p + 1], 63, 47))
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0, 1]):
        got = gpu_render(device, V, F, C, views[order], 63, 47)
        for k, p in enumerate(order):
            same({n: a[k:k + 1] for n, a in got.items()}, solo[p])


SUBSETS = [(n,) for n in ALL] + list(itertools.combinations(ALL, 2))


def test_each_output_alone_and_in_pairs_from_dirty_buffers(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(3)
    V, C = V * 0.1, colours(642)
    views, W, H, P = three_views(), 37, 29, 3  # W * H odd
    want = reference(V, F, C, views, W, H)
    r = R.MeshRenderer(V, F, device, colors=C)
    vt = torch.from_numpy(views).to(device)
    shapes = {"rgba": ((P, H, W, 4), torch.float32), "rgb_u8": ((P, H, W, 3), torch.uint8),
              "depth": ((P, H, W, 4), torch.float32), "depth_nz": ((P, H, W), torch.uint8), "ids": ((P, H, W), torch.int32)}
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, len(F), W, H)), dtype=torch.uint8, device=device)
    for subset in SUBSETS:
        # every buffer is allocated and filled with garbage; only the subset is handed to the op
        bufs = {k: torch.empty(s, dtype=d, device=device) for k, (s, d) in shapes.items()}
        for t in bufs.values():
            t.view(torch.uint8).fill_(0xAB)
        ws.fill_(0x5A)
        rec = torch.full((P, 16), -1, dtype=torch.int32, device=device)
        ops.mesh_render(r.vertices, r.triangles, r.colors, vt, W, H, *[bufs[k] if k in subset else None for k in ALL], rec, ws)
        torch.cuda.synchronize(device)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32), want["records"]), subset
        for k in ALL:
            got = bufs[k].cpu().numpy()
            if k in subset:
                assert np.array_equal(bits(got), bits(want[k])), (subset, k)
            else:
                assert (bufs[k].view(torch.uint8) == 0xAB).all(), (subset, k)


def quad_view(depth_q):
    V, F, views, W, H = CASES["fronto_quad"]()
    views = views.copy()
    views[0, 17] = depth_q
    return V, F, views, W, H


def test_the_8_bit_planes(device):
    from pixtrack_amd.ops import ops

    V, F, views, W, H = CASES["torus"]()
    got = gpu_render(device, V, F, colours(len(V)), np.concatenate([views, views]), W, H)
    for p in range(2):
        u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
        ops.rgba_to_u8(torch.from_numpy(got["rgba"][p]).to(device), 0.0, u8)
        assert np.array_equal(u8.cpu().numpy(), got["rgb_u8"][p]) and got["rgb_u8"][p].max() > 100
    # the wrap: QUAD_DEPTH * depth_q * 255 lands in [256, 257) -> the byte is 0, as uint8(depth * 255) in the reference
    V, F, views, W, H = quad_view(256.5 / 255.0 / QUAD_DEPTH)
    C = colours(len(V))
    wrap = gpu_render(device, V, F, C, views, W, H)
    hit = wrap["ids"] >= 0
    d = wrap["depth"][..., 0][hit]
    assert hit.sum() > 500 and (d * np.float32(255.0) >= 256).all() and (d * np.float32(255.0) < 257).all()
    assert (wrap["depth_nz"][hit] == 0).all() and (wrap["depth_nz"] == 0).all()
    same(wrap, reference(V, F, C, views, W, H))
    V, F, views, W, H = quad_view(1.0 / QUAD_DEPTH)
    one = gpu_render(device, V, F, C, views, W, H)
    assert np.array_equal(one["depth_nz"], (one["ids"] >= 0).astype(np.uint8))
    same(one, reference(V, F, C, views, W, H))


def test_every_bound_is_refused_and_nothing_is_written(device):
    L = _lib.lib()
    V, F = R.icosphere(0)
    C = colours(len(V))
    W, H, P = 15, 11, 2
    need = int(L.pxt_mesh_raster_workspace_bytes(P, len(F), W, H))
    views = np.stack([view(**{**SPHERE_VIEW, "cx": 7.3, "cy": 5.1, "fx": 20.0, "fy": 20.0})] * P)
    bufs = dict(v=torch.from_numpy(V.astype(np.float32)).to(device), f=torch.from_numpy(F.astype(np.int32)).to(device),
                c=torch.from_numpy(C).to(device), views=torch.from_numpy(views).to(device))
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
    ptr = {k: t.data_ptr() for k, t in outs.items()}
    assert all(ptr[k] % 16 == 0 for k in ptr)

    def call(nv=len(V), nt=len(F), p=P, w=W, h=H, vertices=bufs["v"].data_ptr(), colors=bufs["c"].data_ptr(), **over):
        a = {**ptr, **over}
        return L.pxt_mesh_render(vertices, nv, bufs["f"].data_ptr(), nt, colors, bufs["views"].data_ptr(), p, w, h,
                                 a["rgba"], a["u8"], a["depth"], a["nz"], a["tri"], a["rec"], a["ws"], stream)

    bad = [dict(p=0), dict(p=4097), dict(nv=0), dict(nv=(1 << 24) + 1), dict(nt=0), dict(nt=(1 << 24) + 1), dict(w=0),
           dict(h=0), dict(w=1 << 13, h=(1 << 13) + 1), dict(w=-4), dict(depth=ptr["depth"] + 4), dict(depth=ptr["depth"] + 8),
           dict(rgba=ptr["rgba"] + 8), dict(u8=ptr["u8"] + 1), dict(u8=ptr["u8"] + 2), dict(nz=ptr["nz"] + 3),
           dict(tri=ptr["tri"] + 2), dict(ws=ptr["ws"] + 8), dict(vertices=None), dict(colors=None),
           dict(colors=bufs["c"].data_ptr() + 2), dict(ws=None), dict(rec=None),
           dict(rgba=None, u8=None, depth=None, nz=None, tri=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == 0xAB).all(), name
    assert call() == 0  # and the same buffers serve a good call
    torch.cuda.synchronize(device)
    want = reference(V, F, C, views, W, H)
    assert want["records"][0, R.W_COVERED] > 20
    assert np.array_equal(outs["rec"].cpu().numpy().view(np.uint32).reshape(P, 16), want["records"])
    for name, key, per in (("rgba", "rgba", 4), ("u8", "rgb_u8", 3), ("depth", "depth", 4), ("nz", "depth_nz", 1), ("tri", "ids", 1)):
        got = outs[name][:n * per].cpu().numpy().reshape(want[key].shape)
        assert np.array_equal(bits(got), bits(want[key])), name
        assert (outs[name][n * per:].view(torch.uint8) == 0xAB).all(), name  # nothing past the planes' ends


def test_the_op_refuses_host_tensors_wrong_dtypes_and_wrong_shapes(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(0)
    v, f = torch.from_numpy(V.astype(np.float32)).to(device), torch.from_numpy(F.astype(np.int32)).to(device)
    c = torch.from_numpy(colours(len(V))).to(device)
    views = torch.from_numpy(view(**SPHERE_VIEW)[None]).to(device)
    W, H = 16, 12
    u8 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=device)
    nz = torch.empty(1, H, W, dtype=torch.uint8, device=device)
    depth = torch.empty(1, H, W, 4, device=device)
    rec = torch.empty(1, 16, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(1, len(F), W, H)), dtype=torch.uint8, device=device)
    ops.mesh_render(v, f, c, views, W, H, None, u8, depth, nz, None, rec, ws)
    bad = [dict(f=f.long()), dict(c=c.double()), dict(c=c[:-1].contiguous()), dict(c=c[:, :2].contiguous()),
           dict(views=views[:, :12].contiguous()), dict(u8=u8.int()), dict(u8=u8[..., :2].contiguous()),
           dict(u8=torch.empty(1, H, W + 1, 3, dtype=torch.uint8, device=device)), dict(nz=nz.float()),
           dict(nz=nz[:, :-1].contiguous()), dict(depth=depth[..., :3].contiguous()), dict(depth=depth.half()),
           dict(rgba=depth.double()), dict(ids=nz), dict(ws=ws[:16]), dict(rec=rec[:, :8].contiguous()),
           dict(u8=None, nz=None, depth=None), dict(W=0)]
    for kw in bad:
        a = dict(v=v, f=f, c=c, views=views, W=W, H=H, rgba=None, u8=u8, depth=depth, nz=nz, ids=None, rec=rec, ws=ws)
        a.update(kw)
        with pytest.raises(_lib.PxtError):
            ops.mesh_render(*a.values())
    for kw in (dict(rec=rec.cpu()), dict(u8=u8.cpu()), dict(c=c.cpu())):
        a = dict(v=v, f=f, c=c, views=views, W=W, H=H, rgba=None, u8=u8, depth=depth, nz=nz, ids=None, rec=rec, ws=ws)
        a.update(kw)
        with pytest.raises(RuntimeError):  # PxtError, unless the dispatcher objects to the mixed devices first
            ops.mesh_render(*a.values())
    with pytest.raises(_lib.PxtError, match="colours"):
        R.MeshRenderer(V, F, device).render(views, W, H)
    with pytest.raises(_lib.PxtError, match="want"):
        R.MeshRenderer(V, F, device, colors=c).render(views, W, H, want=("rgb", ))


def test_the_builder_on_the_gpu_writes_the_reference_runs_files(device, tmp_path):
    V, F, C = builder_inputs()
    D.build_reference_from_mesh(V, F, C, tmp_path / "host", renderer=D.reference_renderer(V, F, C), **BUILD)
    s = D.build_reference_from_mesh(V, F, C, tmp_path / "gpu", device=device, views_per_call=5, **BUILD)
    a, b = read_tree(tmp_path / "host"), read_tree(tmp_path / "gpu")
    assert s["views"] == 12 and sorted(a) == sorted(b) and len(a) == 15
    for name in a:
        assert a[name] == b[name], name
