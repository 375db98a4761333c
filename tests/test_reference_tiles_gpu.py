"""Reference tiles: a UNet pass that is told the points its fine map will be sampled at computes only the tiles of its
last two decoder layers that a sample depends on (pxt_unet.hip reference_tiles_kernel, pxt_unet_forward_sampled).

What must hold: (1) the flag rule equals a replica written here from the sampler's and the up-sampling's definitions,
not from the kernel's expressions; (2) every sampled observation - descriptors, confidence, validity - is the same bits
with the option on and off, for points on tile seams, in the last row and column, outside the image, behind the camera
and inside a windowed pass; (3) a needed tile of the fine map is bit for bit the dense pass's and every other tile is
not written at all, with the workspace full of NaN beforehand (a rule one texel short for the layer before the last
lets a NaN through to a sample); (4) a tracked sequence's poses do not change.

Points are (x, y, 1) under the identity pose and a camera with f = 1 / stride, c = 0: the projection is exact in any
arithmetic, so the replica can name the texels without reproducing float rounding."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib

TILE = 16  # rows (and columns) of a tile of every decoder configuration the planner picks by itself
IDENTITY = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]
SENTINEL = -7777.0


# ---- the rule, restated ---------------------------------------------------------------------------------------------
def replica_flags(xyz, fine_h, fine_w, pad, window=None, fine_rows=TILE, low_rows=TILE):
    """-> (fine flags [tiles_y, tiles_x], low flags) for points (x, y, z) seen by the identity pose and the unit camera.

    Fine layer: the sampler reads texels (floor u, floor v) and its right / lower neighbours clamped to the full level,
    for every point in front of the camera and at least `pad` inside the full level; a windowed pass holds them at
    (. - x0, . - y0).  Layer before: a 3 x 3 convolution over the x2 bilinear up-sampling (align_corners = False) reads,
    for every row gy of the tile's one-pixel halo, the low rows floor(max((gy + 0.5) / 2 - 0.5, 0)) and the next one,
    clamped into the map - the same for columns."""
    x0, y0, full_w, full_h = window if window is not None else (0, 0, fine_w, fine_h)
    fine = np.zeros((-(-fine_h // fine_rows), -(-fine_w // 16)), np.uint8)
    for x, y, z in np.asarray(xyz, np.float32):
        if not z > 1e-3:
            continue
        u, v = np.float32(x) / np.float32(z), np.float32(y) / np.float32(z)
        if not (u >= pad and v >= pad and u <= full_w - 1 - pad and v <= full_h - 1 - pad):
            continue
        iu, iv = int(math.floor(u)), int(math.floor(v))
        for tx in (iu, min(iu + 1, full_w - 1)):
            for ty in (iv, min(iv + 1, full_h - 1)):
                wx, wy = min(max(tx - x0, 0), fine_w - 1), min(max(ty - y0, 0), fine_h - 1)
                fine[wy // fine_rows, wx // 16] = 1
    low_h, low_w = fine_h // 2, fine_w // 2
    low = np.zeros((-(-low_h // low_rows), -(-low_w // 16)), np.uint8)

    def sources(g0, g1, n):  # low rows / columns behind the halo [g0 - 1, g1] of a tile
        out = set()
        for g in range(g0 - 1, g1 + 1):
            s = int(math.floor(max((g + 0.5) / 2 - 0.5, 0.0)))
            out |= {min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1)}
        return out

    for r, c in zip(*np.nonzero(fine)):
        for ly in sources(r * fine_rows, (r + 1) * fine_rows, low_h):
            for lx in sources(c * 16, (c + 1) * 16, low_w):
                low[ly // low_rows, lx // 16] = 1
    return fine, low


def seam_points(fw, fh, rng, n_random=8):
    """Points of an fw x fh level: tile seams, the last row and column, outside, behind the camera, and a few in the left
    third (so that a map more than three tiles wide keeps tiles nobody reads)."""
    xs = [15.999, 16.0, 31.999, 32.0, 0.0, 0.5, fw - 1.0, fw - 1.001, fw - 2.0]
    ys = [15.999, 16.0, 31.999, 32.0, 0.0, 0.5, fh - 1.0, fh - 1.001, fh - 2.0]
    pts = [(x, y, 1.0) for x in xs for y in ys if x <= fw - 1 and y <= fh - 1]
    pts += [(-3.0, 5.0, 1.0), (fw + 2.0, 5.0, 1.0), (5.0, -0.25, 1.0), (5.0, fh - 0.5, 1.0), (fw - 0.5, 3.0, 1.0)]
    pts += [(8.0, 8.0, -1.0), (20.0, 9.0, 0.0)]  # behind the camera / on its plane
    pts += [(float(rng.uniform(-4, fw / 3)), float(rng.uniform(-4, fh + 4)), 1.0) for _ in range(n_random)]
    return np.asarray(pts, np.float32)


def record(p3d_ptr, n, pad, full, windowed):
    pts = _lib.UnetSamplePoints()
    pts.p3d, pts.n_points = p3d_ptr, n
    pts.T[:] = IDENTITY
    pts.cam[:] = [float(full[2]), float(full[3]), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0]
    pts.ndist, pts.pad = 0, pad
    pts.x0, pts.y0, pts.full_w, pts.full_h = full if windowed else (0, 0, 0, 0)
    return pts


@pytest.mark.parametrize("fine_hw,window,rows", [
    ((32, 32), None, (16, 16)), ((64, 96), None, (16, 16)), ((112, 160), None, (16, 16)), ((112, 160), None, (16, 8)),
    ((96, 144), None, (24, 16)), ((64, 96), None, (32, 16)), ((64, 96), (32, 16, 240, 160), (16, 16)),
    ((64, 96), (144, 96, 240, 160), (16, 16)), ((48, 80), (0, 0, 80, 48), (16, 16))])
@pytest.mark.parametrize("pad", [0, 4])
def test_flag_rule_on_the_host(fine_hw, window, rows, pad):
    """pxt_unet_reference_tiles_host runs the device kernel's own functions on the host: no GPU needed."""
    fh, fw = fine_hw
    full = window if window is not None else (0, 0, fw, fh)
    rng = np.random.default_rng(fh * 1000 + fw + pad)
    xyz = seam_points(full[2], full[3], rng)
    if window is not None:  # the seams of the WINDOW's tiles as well
        extra = seam_points(fw, fh, rng, 0)
        extra[:, 0] += window[0]
        extra[:, 1] += window[1]
        xyz = np.concatenate([xyz, extra])
    xyz = np.ascontiguousarray(xyz)
    want_fine, want_low = replica_flags(xyz, fh, fw, pad, window, *rows)
    got_fine, got_low = np.full(want_fine.shape, 9, np.uint8), np.full(want_low.shape, 9, np.uint8)
    pts = record(xyz.ctypes.data, len(xyz), pad, full, window is not None)
    _lib.check(_lib.lib().pxt_unet_reference_tiles_host(C.byref(pts), fh, fw, rows[0], rows[1], got_fine.ctypes.data,
                                                        got_low.ctypes.data), "pxt_unet_reference_tiles_host")
    assert 0 < want_fine.sum() and np.array_equal(got_fine, want_fine)
    assert np.array_equal(got_low, want_low)
    # no point at all, or none that is valid: nothing is needed
    pts.n_points = 0
    _lib.check(_lib.lib().pxt_unet_reference_tiles_host(C.byref(pts), fh, fw, rows[0], rows[1], got_fine.ctypes.data,
                                                        got_low.ctypes.data), "pxt_unet_reference_tiles_host")
    assert not got_fine.any() and not got_low.any()


# ---- on the GPU -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(device):
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    return UNet(make_synthetic_unet_weights(7), device)


def run_pass(net, image, sample_points, poison):
    """One single-image pass through the op, on buffers of this test's own: -> the three maps.  `poison`: the fine map is
    pre-filled with SENTINEL and the whole workspace with 0xFF bytes (fp16 / fp32 NaN)."""
    from pixtrack_amd.ops import ops
    from pixtrack_amd.optimizer import cstride_for
    from pixtrack_amd.unet import OUTPUT_DIMS

    H, W = int(image.shape[0]), int(image.shape[1])
    need = int(_lib.lib().pxt_unet_workspace_bytes_batch(net._ctx, 1, H, W))
    assert need > 0
    ws = torch.full((need,), 0xFF if poison else 0, dtype=torch.uint8, device=image.device)
    outs = [torch.full((h, w, cstride_for(c)), SENTINEL if poison else 0.0, device=image.device)
            for (h, w), c in zip(net.level_shapes(H, W), OUTPUT_DIMS)]
    extra = () if sample_points is None else (sample_points["p3d"], sample_points["pose_camera"], sample_points["ints"])
    ops.unet_forward_batch(int(net._ctx.value), [image], [None], [False], outs, ws, *extra)
    torch.cuda.synchronize()
    return outs


def sample(maps, p3d, pad, window, camera=None):
    """pxt_sample_sparse of the three levels with the unit cameras; window = (x0, y0, full_w, full_h) of the fine level.
    camera = (geometry.Camera of the fine level, ndist): that camera, scaled to each level, in place of the unit ones."""
    from pixtrack_amd.ops import ops
    from pixtrack_amd.unet import OUTPUT_DIMS

    n = int(p3d.shape[0])
    cams, windows = [], []
    for m, s in zip(maps, (1, 4, 16)):
        full_w, full_h = (window[2] // s, window[3] // s) if window else (int(m.shape[1]), int(m.shape[0]))
        if camera is not None:
            cams += [float(x) for x in camera[0].scale((full_w / float(camera[0].size[0]), full_h / float(camera[0].size[1]))).as10()]
        else:
            cams += [float(full_w), float(full_h), 1.0 / s, 1.0 / s, 0.0, 0.0, 0, 0, 0, 0]
        if window:
            windows += [window[0] // s, window[1] // s, full_w, full_h]
    outs = [torch.full((n, int(m.shape[2])), 5.0, device=p3d.device) for m in maps]
    valid = torch.full((n,), 7, dtype=torch.uint8, device=p3d.device)
    ndist = [0, 0, 0] if camera is None else [camera[1]] * 3
    ops.sample_sparse(p3d, IDENTITY, list(maps), list(OUTPUT_DIMS), cams, ndist, pad, True, outs, valid, windows or None)
    return outs, valid


CASES = [  # image (H, W), pad, window of the fine level or None
    ((32, 32), 0, None),                       # the smallest pyramid the sampler accepts: one tile wide at half resolution
    ((76, 100), 0, None),                      # an odd size: the maps are 64 x 96, the layer before 32 x 48 (a half tile)
    ((120, 160), 0, None),                     # 112 x 160 maps, 56 rows before: partial tile rows there
    ((120, 160), 4, None),                     # the refiner's usual pad
    ((64, 96), 0, (32, 16, 240, 160)),         # a windowed pass in the middle of a 240 x 160 level
    ((64, 96), 0, (144, 96, 240, 160)),        # ... and one that ends at the level's last row and column
]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,pad,window", CASES)
def test_sampled_pass_equals_the_dense_pass_where_it_is_read(net, device, hw, pad, window):
    H, W = hw
    g = torch.Generator().manual_seed(H * 7 + W)
    image = (torch.rand(H, W, 3, generator=g) * 255).to(device).contiguous()
    fh, fw = net.level_shapes(H, W)[0]
    full = window if window is not None else (0, 0, fw, fh)
    rng = np.random.default_rng(H + W + pad)
    xyz = seam_points(full[2], full[3], rng)
    if window is not None:
        extra = seam_points(fw, fh, rng, 0)
        extra[:, 0] += window[0]
        extra[:, 1] += window[1]
        xyz = np.concatenate([xyz, extra])
    p3d = torch.from_numpy(np.ascontiguousarray(xyz)).to(device)
    points = {"p3d": p3d, "pose_camera": IDENTITY + [float(full[2]), float(full[3]), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0],
              "ints": [0, pad] + (list(window) if window is not None else [0, 0, 0, 0])}
    net.set_reference_tiles(False)
    try:
        dense = run_pass(net, image, points, poison=True)  # (option off: the points are ignored, every tile is written)
    finally:
        net.set_reference_tiles(True)
    got = run_pass(net, image, points, poison=True)
    plain = run_pass(net, image, None, poison=False)
    for a, b in zip(dense, plain):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # the two coarser maps are untouched by the option
    assert torch.equal(got[1], dense[1]) and torch.equal(got[2], dense[2])
    # the fine map, tile by tile
    want_fine, _ = replica_flags(xyz, fh, fw, pad, window)
    assert 0 < want_fine.sum() < want_fine.size or want_fine.size <= 4
    for r in range(want_fine.shape[0]):
        for c in range(want_fine.shape[1]):
            a = got[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]
            if want_fine[r, c]:
                assert torch.equal(a, dense[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]), (r, c)
            else:
                assert bool((a == SENTINEL).all()), (r, c)
    # what the sampler hands on: the same bits, and no NaN from an uncomputed tile of either layer
    outs_d, valid_d = sample(dense, p3d, pad, window)
    outs_g, valid_g = sample(got, p3d, pad, window)
    assert torch.equal(valid_d, valid_g)
    for a, b in zip(outs_d, outs_g):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    fine_valid = (outs_d[0] != 0).any(1)
    assert int(fine_valid.sum()) >= 20 and not bool(fine_valid.all())


@pytest.mark.gpu
def test_sampled_pass_equals_the_dense_pass_under_the_opencv_camera(net, device):
    """The smallest pyramid (32 x 32: two by two fine tiles) under the OPENCV camera of tests/camera_cases.py scaled to
    the fine map (ndist 4: project_point's tangential terms decide the texels): the marked tiles are those the host
    statement of the rule names with the same record, the sampled observations are the dense pass's bit for bit, and no
    unmarked tile is written."""
    import camera_cases as CC
    from pixtrack_amd.geometry import Camera

    H, W, pad = 32, 32, 0
    image = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(H * 7 + W + 1)) * 255).to(device).contiguous()
    fh, fw = net.level_shapes(H, W)[0]
    cam = Camera.from_colmap(CC.colmap("opencv")).scale((fw / CC.WIDTH, fh / CC.HEIGHT))
    cam10 = [float(x) for x in cam.as10()]
    ndist = CC.NDIST["opencv"]
    # camera-frame points whose pinhole projections fill the upper left tile and straddle its right seam; the distortion
    # then moves them by a fraction of a texel; a few outside the map and behind the camera
    rng = np.random.default_rng(41)
    uv = np.concatenate([rng.uniform(0.5, 14.0, (40, 2)), np.stack([rng.uniform(14.5, 17.5, 12), rng.uniform(1.0, 12.0, 12)], 1),
                         [[-3.0, 5.0], [fw + 2.0, 5.0], [5.0, fh + 0.5]]])
    z = np.concatenate([rng.uniform(0.7, 1.6, len(uv) - 2), [-1.0, 0.0]])
    uv = np.concatenate([uv[:-2], [[8.0, 8.0], [9.0, 9.0]]])
    xyz = np.stack([(uv[:, 0] - cam10[4]) / cam10[2] * z, (uv[:, 1] - cam10[5]) / cam10[3] * z, z], 1).astype(np.float32)
    xyz = np.ascontiguousarray(xyz)
    p3d = torch.from_numpy(xyz).to(device)
    points = {"p3d": p3d, "pose_camera": IDENTITY + cam10, "ints": [ndist, pad, 0, 0, 0, 0]}
    net.set_reference_tiles(False)
    try:
        dense = run_pass(net, image, points, poison=True)
    finally:
        net.set_reference_tiles(True)
    got = run_pass(net, image, points, poison=True)
    pts = record(xyz.ctypes.data, len(xyz), pad, (0, 0, fw, fh), False)
    pts.cam[:] = cam10
    pts.ndist = ndist
    want_fine = np.full((-(-fh // TILE), -(-fw // 16)), 9, np.uint8)
    want_low = np.full((-(-(fh // 2) // TILE), -(-(fw // 2) // 16)), 9, np.uint8)
    _lib.check(_lib.lib().pxt_unet_reference_tiles_host(C.byref(pts), fh, fw, TILE, TILE, want_fine.ctypes.data,
                                                        want_low.ctypes.data), "pxt_unet_reference_tiles_host")
    assert 0 < want_fine.sum() < want_fine.size, want_fine
    assert torch.equal(got[1], dense[1]) and torch.equal(got[2], dense[2])
    for r in range(want_fine.shape[0]):
        for c in range(want_fine.shape[1]):
            a = got[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]
            if want_fine[r, c]:
                assert torch.equal(a, dense[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]), (r, c)
            else:
                assert bool((a == SENTINEL).all()), (r, c)
    outs_d, valid_d = sample(dense, p3d, pad, None, camera=(cam, ndist))
    outs_g, valid_g = sample(got, p3d, pad, None, camera=(cam, ndist))
    assert torch.equal(valid_d, valid_g)
    for a, b in zip(outs_d, outs_g):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    fine_valid = (outs_d[0] != 0).any(1)
    assert int(fine_valid.sum()) >= 40 and not bool(fine_valid.all())


@pytest.mark.gpu
def test_no_valid_point_computes_no_fine_tile(net, device):
    H, W = 76, 100
    image = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3)) * 255).to(device).contiguous()
    fh, fw = net.level_shapes(H, W)[0]
    xyz = np.asarray([(8.0, 8.0, -1.0), (-5.0, 3.0, 1.0), (fw + 1.0, 2.0, 1.0), (3.0, fh - 0.5, 1.0)], np.float32)
    p3d = torch.from_numpy(xyz).to(device)
    points = {"p3d": p3d, "pose_camera": IDENTITY + [float(fw), float(fh), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0],
              "ints": [0, 0, 0, 0, 0, 0]}
    got = run_pass(net, image, points, poison=True)
    plain = run_pass(net, image, None, poison=False)
    assert bool((got[0] == SENTINEL).all())
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    outs, valid = sample(got, p3d, 0, None)
    assert not bool(valid.any()) and not bool(outs[0].any())


@pytest.mark.gpu
def test_tracked_poses_do_not_change(device):
    """A few frames at 160 x 120 with the option on and off: the reference pass of every warm frame is handed its points
    (the cold start encodes a resized image and is not), and every pose, cost and verdict is the same bits."""
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    assets = make_tracking_assets(seed=1011, width=160, height=120, n_frames=4, n_points=3000)
    runs = []
    for on in (True, False):
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=1, device=device, assets=assets)
        tr.spp = 2
        model = tr.localizer.extractor.model
        model.set_reference_tiles(on)
        handed = []
        inner = model.arm_sample_points
        model.arm_sample_points = lambda sample_points: (handed.append(sample_points is not None), inner(sample_points))[1]
        frames = render_query_frames(assets, tr.testbed)
        for i, f in enumerate(frames):
            tr.run_single_frame((f"{i:06d}.png", f))
        rows = []
        for i in range(len(frames)):
            ret = tr.pose_history[f"{i:06d}.png"]
            rows.append((ret["success"], ret.get("cost"), ret.get("T_refined", ret["T_init"]).as12().detach().cpu()))
        runs.append((rows, sum(handed)))
    (rows_on, handed_on), (rows_off, handed_off) = runs
    assert handed_on >= 2 and handed_on == handed_off
    assert any(ok for ok, _, _ in rows_on)
    for (ok_a, cost_a, T_a), (ok_b, cost_b, T_b) in zip(rows_on, rows_off):
        assert ok_a == ok_b and cost_a == cost_b and torch.equal(T_a, T_b)
