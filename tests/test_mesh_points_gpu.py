"""pxt_points_from_depth_views (torch.ops.pixtrack.points_from_depth_views) against mesh_render.points_reference bit for
bit - p3d as int32 views, slot_valid, records - on the smallest shapes where it can go wrong: several views of different
sizes in one call, partial segments, widths that are no multiple of a wave, every erosion radius, the cut tail, the
empty plane, 16 views; a view's independence of the call it rides in; the selection against the one-view kernel it
generalises; real planes of a frame call; the op's checks."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, mesh_render as R
from pixtrack_amd.ops import ops
from test_mesh_points_host import IDENTITY_VIEW, cut_tail_plane, lattice_pixels

pytestmark = pytest.mark.gpu


def blob_plane(rng, W, H, fill):
    """A depth plane as the rasteriser writes it: an ellipse (``fill`` of the half axes) of random depths in (0.2, 0.9),
    with a few holes punched into it; alpha 1 where covered, four zeros elsewhere."""
    y, x = np.mgrid[0:H, 0:W]
    covered = ((x - (W - 1) / 2) / (fill * W / 2)) ** 2 + ((y - (H - 1) / 2) / (fill * H / 2)) ** 2 <= 1.0
    covered &= rng.random((H, W)) > 0.02
    d = np.zeros((H, W, 4), np.float32)
    z = rng.uniform(0.2, 0.9, (H, W)).astype(np.float32)
    d[covered] = np.stack([z, z, z, np.ones_like(z)], -1)[covered]
    return d


def random_view(rng, W, H):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return R.pack_view(q, rng.normal(size=3) + [0, 0, 3.0], rng.uniform(40, 90), rng.uniform(40, 90), W * rng.uniform(0.3, 0.7),
                       H * rng.uniform(0.3, 0.7), 1e-6, rng.uniform(0.1, 0.4))


def run(device, planes, views, min_alpha, erode, n_max, record_device=True):
    K = len(planes)
    d = [p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in planes]
    sizes = [x for p in d for x in (int(p.shape[1]), int(p.shape[0]))]
    need = int(_lib.lib().pxt_points_from_depth_views_workspace_bytes(K, (_lib.C.c_int32 * (2 * K))(*sizes)))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    p3d = torch.full((K, n_max, 3), float("nan"), dtype=torch.float32, device=device)
    valid = torch.full((K, n_max), 7, dtype=torch.uint8, device=device)
    rec = torch.full((K, 4), -1, dtype=torch.int32, device=device) if record_device else torch.full((K, 4), -1, dtype=torch.int32).pin_memory()
    ops.points_from_depth_views(d, np.asarray(views, np.float32).reshape(-1).tolist(), float(min_alpha), int(erode), int(n_max),
                                p3d, valid, rec, ws)
    torch.cuda.synchronize(device)
    return p3d.cpu().numpy(), valid.cpu().numpy(), rec.cpu().numpy()


def same_bits(got, planes, views, min_alpha, erode, n_max):
    p3d, valid, rec = got
    for k, (plane, view) in enumerate(zip(planes, views)):
        want_p, want_v, want_r = R.points_reference(plane.cpu().numpy() if torch.is_tensor(plane) else plane, view, min_alpha,
                                                    erode, n_max)
        assert rec[k].tolist() == want_r.tolist(), (k, rec[k], want_r)
        assert np.array_equal(valid[k], want_v), k
        assert np.array_equal(p3d[k].view(np.int32), want_p.view(np.int32)), (k, np.abs(p3d[k] - want_p).max())


@pytest.fixture(scope="module")
def three():
    """37 x 29 (1073 pixels: two segments, the second partial, a width that is no multiple of 64), 32 x 32 (exactly one
    segment), 8 x 8 (less than one wave trip, nothing covered).  n_max = 300: view 0 has s = 1, view 1 s = 2."""
    rng = np.random.default_rng(41)
    planes = [blob_plane(rng, 37, 29, 0.6), blob_plane(rng, 32, 32, 2.0), np.zeros((8, 8, 4), np.float32)]
    views = np.stack([random_view(rng, 37, 29), random_view(rng, 32, 32), random_view(rng, 8, 8)])
    return planes, views


@pytest.mark.parametrize("erode", [0, 1, 2])
def test_three_views_of_different_sizes_in_one_call(device, three, erode):
    planes, views = three
    got = run(device, planes, views, 0.5, erode, 300)
    same_bits(got, planes, views, 0.5, erode, 300)
    rec = got[2]
    print(f"erode {erode}: records {rec.tolist()}")
    if erode == 1:
        assert rec[0, 1] == 1 and 0 < rec[0, 2] < 300 and rec[1, 1] >= 2 and rec[1, 2] > 0 and rec[2].tolist() == [0, 1, 0, 0]


def test_the_cut_tail_and_a_pinned_record(device):
    planes, views = [cut_tail_plane()], IDENTITY_VIEW[None]
    for record_device in (True, False):
        got = run(device, planes, views, 0.5, 0, 4, record_device=record_device)
        assert got[2][0].tolist() == [9, 2, 4, 9]
        same_bits(got, planes, views, 0.5, 0, 4)


def test_sixteen_views_and_one(device):
    rng = np.random.default_rng(43)
    planes = [blob_plane(rng, 16, 12, rng.uniform(0.5, 2.0)) for _ in range(16)]
    views = np.stack([random_view(rng, 16, 12) for _ in range(16)])
    same_bits(run(device, planes, views, 0.5, 1, 24), planes, views, 0.5, 1, 24)
    same_bits(run(device, planes[:1], views[:1], 0.5, 1, 24), planes[:1], views[:1], 0.5, 1, 24)


def test_a_view_does_not_depend_on_the_call_it_rides_in(device, three):
    planes, views = three
    p3d, valid, rec = run(device, planes, views, 0.5, 1, 300)
    again = run(device, planes, views, 0.5, 1, 300)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((p3d, valid, rec), again))  # two launches
    order = [2, 0, 1]
    permuted = run(device, [planes[k] for k in order], views[order], 0.5, 1, 300)
    for i, k in enumerate(order):
        alone = run(device, [planes[k]], views[k:k + 1], 0.5, 1, 300)
        for a, b, c in zip((p3d, valid, rec), alone, permuted):
            assert np.array_equal(a[k].view(np.uint8), b[0].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[i].view(np.uint8))


@pytest.mark.parametrize("erode,n_max", [(0, 300), (1, 40), (2, 7)])
def test_the_selection_is_the_one_view_kernels(device, three, erode, n_max):
    """Records and slot_valid of pxt_points_from_depth on the same 37 x 29 plane (the points follow another pixel rule)."""
    plane = torch.from_numpy(three[0][0]).to(device)
    _, valid, rec = run(device, [plane], three[1][:1], 0.5, erode, n_max)
    ws = torch.empty(int(_lib.lib().pxt_points_from_depth_workspace_bytes(37, 29)), dtype=torch.uint8, device=device)
    p3d1 = torch.empty(n_max, 3, dtype=torch.float32, device=device)
    valid1 = torch.full((n_max,), 7, dtype=torch.uint8, device=device)
    rec1 = torch.full((4,), -1, dtype=torch.int32, device=device)
    ops.points_from_depth(plane, [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], 50.0, 1.0, 0.5, erode, n_max, p3d1, valid1, rec1, ws)
    torch.cuda.synchronize(device)
    assert rec[0].tolist() == rec1.cpu().tolist() and np.array_equal(valid[0], valid1.cpu().numpy())
    assert rec[0, 0] > 0


def test_real_planes_of_one_frame_call(device):
    V, F = R.icosphere(2)
    V = V * np.array([1.0, 0.8, 0.6])
    rng = np.random.default_rng(47)
    renderer = R.MeshRenderer(V, F, device, colors=rng.uniform(0.2, 1.0, V.shape))
    radius = float(np.linalg.norm(V, axis=1).max())
    requests = []
    for W, H, f in ((75, 53, 70.0), (40, 64, 55.0)):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        t = np.array([0.1, -0.05, 3.0])
        view = R.pack_view(q, t, f, 0.9 * f, 0.45 * W, 0.55 * H, 1e-6, 1.0 / (np.linalg.norm(t) + radius))
        requests.append((view, W, H, 1, ("depth",)))
    out = renderer.render_frame(requests)
    planes, views = [o["depth"] for o in out], np.stack([r[0] for r in requests])
    assert planes[0].shape == (53, 75, 4) and planes[1].shape == (64, 40, 4)
    got = run(device, planes, views, 0.5, 1, 128)
    same_bits(got, planes, views, 0.5, 1, 128)
    for k, view in enumerate(views):
        pixels, s = lattice_pixels(planes[k].cpu().numpy(), 0.5, 1, 128)
        n = int(got[2][k, 2])
        assert n == len(pixels) and n > 50 and got[2][k, 1] == s
        v64 = view.astype(np.float64)
        cam = got[0][k, :n].astype(np.float64) @ v64[:9].reshape(3, 3).T + v64[9:12]
        u, v = v64[12] * cam[:, 0] / cam[:, 2] + v64[14], v64[13] * cam[:, 1] / cam[:, 2] + v64[15]
        err = np.hypot(u - [x for x, _ in pixels], v - [y for _, y in pixels]).max()
        print(f"view {k}: {n} points, stride {s}, max reprojection error {err:.3g} px")
        assert err < 1e-2


def test_op_checks(device):
    d = torch.zeros(8, 8, 4, dtype=torch.float32, device=device)
    views = IDENTITY_VIEW.tolist()
    need = int(_lib.lib().pxt_points_from_depth_views_workspace_bytes(1, (_lib.C.c_int32 * 2)(8, 8)))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    p3d = torch.empty(1, 4, 3, dtype=torch.float32, device=device)
    valid = torch.empty(1, 4, dtype=torch.uint8, device=device)
    rec = torch.empty(1, 4, dtype=torch.int32, device=device)
    ops.points_from_depth_views([d], views, 0.5, 1, 4, p3d, valid, rec, ws)  # the good call
    bad = [
        dict(depth=[d.cpu()]), dict(p3d=p3d.cpu()), dict(valid=valid.cpu()), dict(ws=ws.cpu()),        # wrong device
        dict(depth=[d.double()]), dict(p3d=p3d.half()), dict(valid=valid.int()), dict(rec=rec.long()),  # wrong dtype
        dict(depth=[d[..., :3].contiguous()]), dict(depth=[d[:, ::2]]), dict(depth=[]), dict(depth=[d] * 17),
        dict(p3d=p3d[0]), dict(valid=valid[0]), dict(rec=rec[0]), dict(views=views[:19]), dict(views=views * 2),
        dict(erode=3), dict(n_max=5),                                                                   # wrong shape
        dict(ws=ws[:need - 1]),                                                                         # a short workspace
        dict(rec=torch.zeros(1, 4, dtype=torch.int32)),                                                 # a pageable record
    ]
    for kw in bad:
        a = dict(depth=[d], views=views, erode=1, n_max=4, p3d=p3d, valid=valid, rec=rec, ws=ws)
        a.update(kw)
        with pytest.raises(_lib.PxtError):
            ops.points_from_depth_views(a["depth"], a["views"], 0.5, a["erode"], a["n_max"], a["p3d"], a["valid"], a["rec"], a["ws"])
    torch.cuda.synchronize(device)
