"""pxt_mesh_raster against mesh_render.rasterize_reference: bit for bit on the depth image, the triangle ids and the
records, no tolerance and no excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_render as R
from test_mesh_raster_host import CASES, SPHERE_VIEW, rotation, view

pytestmark = pytest.mark.gpu


def gpu_draw(device, V, F, views, W, H, ids=True, out=None):
    depth, tri, rec = R.MeshRenderer(V, F, device).render_depth(views, W, H, out=out, triangle_ids=ids)
    torch.cuda.synchronize(device)
    return depth.cpu().numpy(), None if tri is None else tri.cpu().numpy(), rec


def same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def compare(device, V, F, views, W, H):
    want = R.rasterize_reference(V, F, views, W, H)
    got = gpu_draw(device, V, F, views, W, H)
    same(got, want)
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_host_case(device, name):
    compare(device, *CASES[name]())


def test_micro_triangles(device):
    V, F = R.icosphere(5)
    assert len(F) == 20480
    want = compare(device, V * 0.1, F, view(Rm=rotation(2), fx=115.0, fy=113.0, cx=47.3, cy=39.6, t=(0.01, -0.02, 0.45))[None],
                   96, 80)
    assert want[2][0, R.W_DRAWN] == 20480 and want[2][0, R.W_COVERED] > 1500


def big_quad(z=1.0):
    # larger than the 70 x 66 image on every side (the image spans [-1.6, 1.85] x [-1.45, 1.8] at f = 20), tilted in depth
    V = np.asarray([(-2.3, -2.1, z), (2.6, -1.9, z + 0.2), (2.4, 2.7, z + 0.3), (-2.2, 2.5, z + 0.1)])
    return V, np.asarray([(0, 1, 2), (0, 2, 3)])


BIG_VIEW = dict(fx=20.0, fy=20.0, cx=32.3, cy=29.1)


def test_large_triangles_clipped_on_all_four_sides(device):
    V, F = big_quad()
    want = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    assert want[2][0, R.W_COVERED] == 70 * 66 and set(np.unique(want[1])) == {0, 1}


def test_large_and_small_triangles_in_one_call(device):
    Vq, Fq = big_quad(0.8)
    Vs, Fs = R.icosphere(4)  # 5120 triangles in front of part of the quad
    Vs = Vs * 0.25 + np.asarray([0.2, -0.1, 0.6])
    V, F = np.concatenate([Vs, Vq]), np.concatenate([Fs, Fq + len(Vs)])
    want = compare(device, V, F, view(**BIG_VIEW)[None], 70, 66)
    ids = want[1][0]
    assert (ids >= 5120).any() and (ids < 5120).any() and (ids >= 0).all()


def test_more_large_triangles_than_the_list_holds(device):
    # 1100 triangles that each span the 40 x 30 image at their own depth: past the list's 1024 entries per view the
    # rest takes the wave path, and the image does not tell
    n = 1100
    z = 1.0 + 0.001 * ((np.arange(n) * 37) % n)
    V = np.concatenate([np.stack([np.asarray([(-6.0, -3.0, 1.0), (7.0, -3.0, 1.0), (0.5, 9.0, 1.0)]) * zi for zi in z])])
    V = V.reshape(-1, 3)
    F = np.arange(3 * n).reshape(n, 3)
    want = compare(device, V, F, view(fx=12.0, fy=12.0, cx=19.6, cy=14.2)[None], 40, 30)
    assert (want[1][0] == int(np.argmin(z))).all()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (41, 1)])
def test_degenerate_images(device, W, H):
    V, F = R.icosphere(2)
    want = compare(device, V * 0.1, F, view(fx=60.0, fy=60.0, cx=(W - 1) / 2 + 0.2, cy=(H - 1) / 2 - 0.3, t=(0, 0, 0.5))[None], W, H)
    assert want[2][0, R.W_COVERED] >= 1
    Vq, Fq = big_quad()
    want = compare(device, Vq, Fq, view(fx=20.0, fy=20.0, cx=0.3, cy=0.2)[None], W, H)
    assert want[2][0, R.W_COVERED] == W * H


def three_views():
    a = view(Rm=rotation(11), **SPHERE_VIEW)
    b = view(Rm=rotation(12), fx=140.0, fy=120.0, cx=20.5, cy=30.25, t=(-0.02, 0.03, 0.5), depth_q=2.0)
    c = view(Rm=rotation(13), fx=50.0, fy=55.0, cx=40.0, cy=10.0, t=(0.05, 0.02, 0.9), near=0.85)  # cuts into the sphere
    return np.stack([a, b, c])


def test_views_of_one_call_equal_their_solo_calls_in_any_order(device):
    V, F = R.icosphere(3)
    V = V * 0.1
    views = three_views()
    solo = [gpu_draw(device, V, F, views[p:p + 1], 64, 48) for p in range(3)]
    assert solo[2][2][0, R.W_NEAR] > 0 and solo[2][2][0, R.W_DRAWN] > 0
    for p in range(3):
        same(solo[p], R.rasterize_reference(V, F, views[p:p + 1], 64, 48))
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0, 1]):
        got = gpu_draw(device, V, F, views[order], 64, 48)
        for k, p in enumerate(order):
            same(tuple(x[k:k + 1] for x in got), solo[p])


def test_dirty_buffers_and_no_id_plane(device):
    V, F = R.icosphere(3)
    V = V * 0.1
    views = three_views()
    r = R.MeshRenderer(V, F, device)
    first = r.render_depth(views[:2], 64, 48, triangle_ids=True)
    a = (first[0].cpu().numpy(), first[1].cpu().numpy(), first[2])
    # the same workspace and image buffer, left as another render filled them
    r.render_depth(views[1:], 64, 48, out=first[0], triangle_ids=True)
    again = r.render_depth(views[:2], 64, 48, out=first[0], triangle_ids=True)
    same((again[0].cpu().numpy(), again[1].cpu().numpy(), again[2]), a)
    first[0].fill_(float("nan"))
    r._workspace.fill_(0x5A)
    none = r.render_depth(views[:2], 64, 48, out=first[0], triangle_ids=False)
    assert none[1] is None and np.array_equal(none[2], a[2])
    assert np.array_equal(none[0].cpu().numpy().view(np.uint32), a[0].view(np.uint32))


def test_every_bound_is_refused_and_nothing_is_written(device):
    L = _lib.lib()
    V, F = R.icosphere(0)
    W, H, P = 16, 12, 2
    need = int(L.pxt_mesh_raster_workspace_bytes(P, len(F), W, H))
    bufs = dict(v=torch.from_numpy(V.astype(np.float32)).to(device), f=torch.from_numpy(F.astype(np.int32)).to(device),
                views=torch.from_numpy(np.stack([view(**SPHERE_VIEW)] * P)).to(device))
    outs = dict(depth=torch.empty(P * H * W * 4 + 8, dtype=torch.float32, device=device),
                tri=torch.empty(P * H * W, dtype=torch.int32, device=device),
                rec=torch.empty(P * 16, dtype=torch.int32, device=device),
                ws=torch.empty(need + 32, dtype=torch.uint8, device=device))
    for t in outs.values():
        t.view(torch.uint8).fill_(0xAB)
    stream = _lib.stream_ptr(device)

    def call(nv=len(V), nt=len(F), p=P, w=W, h=H, depth=None, ws=None, vertices=bufs["v"].data_ptr(), rec=None):
        return L.pxt_mesh_raster(vertices, nv, bufs["f"].data_ptr(), nt, bufs["views"].data_ptr(), p, w, h,
                                 outs["depth"].data_ptr() if depth is None else depth, outs["tri"].data_ptr(),
                                 outs["rec"].data_ptr() if rec is None else rec,
                                 outs["ws"].data_ptr() if ws is None else ws, stream)

    assert outs["depth"].data_ptr() % 16 == 0 and outs["ws"].data_ptr() % 16 == 0
    bad = [dict(p=0), dict(p=4097), dict(nv=0), dict(nv=(1 << 24) + 1), dict(nt=0), dict(nt=(1 << 24) + 1), dict(w=0),
           dict(h=0), dict(w=1 << 13, h=(1 << 13) + 1), dict(w=-4), dict(depth=outs["depth"].data_ptr() + 4),
           dict(depth=outs["depth"].data_ptr() + 8), dict(ws=outs["ws"].data_ptr() + 8), dict(vertices=None),
           dict(depth=0), dict(ws=0), dict(rec=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == 0xAB).all(), name
    assert call() == 0  # and the same buffers serve a good call
    torch.cuda.synchronize(device)
    want = R.rasterize_reference(V, F, bufs["views"].cpu().numpy(), W, H)
    assert np.array_equal(outs["rec"].cpu().numpy().view(np.uint32).reshape(P, 16), want[2])
    assert np.array_equal(outs["tri"].cpu().numpy().reshape(P, H, W), want[1])
    assert (outs["depth"][P * H * W * 4:].view(torch.uint8) == 0xAB).all()


def test_the_op_refuses_host_tensors_and_wrong_shapes(device):
    from pixtrack_amd.ops import ops

    V, F = R.icosphere(0)
    v, f = torch.from_numpy(V.astype(np.float32)).to(device), torch.from_numpy(F.astype(np.int32)).to(device)
    views = torch.from_numpy(view(**SPHERE_VIEW)[None]).to(device)
    depth = torch.empty(1, 12, 16, 4, device=device)
    rec = torch.empty(1, 16, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(1, len(F), 16, 12)), dtype=torch.uint8, device=device)
    ops.mesh_raster(v, f, views, depth, None, rec, ws)
    with pytest.raises(_lib.PxtError):
        ops.mesh_raster(v, f.long(), views, depth, None, rec, ws)
    with pytest.raises(_lib.PxtError):
        ops.mesh_raster(v, f, views[:, :12].contiguous(), depth, None, rec, ws)
    with pytest.raises(_lib.PxtError):
        ops.mesh_raster(v, f, views, depth, None, rec, ws[:16])
    with pytest.raises(RuntimeError):  # PxtError, unless the dispatcher objects to the mixed devices first
        ops.mesh_raster(v, f, views, depth, None, rec.cpu(), ws)
    with pytest.raises(_lib.PxtError):
        R.MeshRenderer(V, F, "cpu")
