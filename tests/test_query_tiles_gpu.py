"""Query tiles on the GPU: the pair pass that computes only the fine tiles the LM will read, the LM's tile guard, and the
tracker's fallback (pxt_unet.hip query_tiles_mark, pxt_lm.hip lm_tile_guard, refiner.refine_pose_using_features).

None of this provokes a fault: the NaN fill is ordinary data, and the guard case reads a fully computed map."""
import ctypes as C
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from test_query_tiles import IDENTITY, host_flags, record, replica_fine

ROOT = Path(__file__).resolve().parents[1]
TILE = 16
NH = 16 + _lib.PXT_MAX_LEVELS


# ---- the pair pass ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(device):
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    return UNet(make_synthetic_unet_weights(7), device)


def pair_pass(net, images, first, second):
    """One pair pass on buffers of this test's own, the workspace full of 0xFF bytes (fp16 / fp32 NaN) and every map of
    NaN beforehand -> (maps of image 0, maps of image 1, workspace)."""
    from pixtrack_amd.ops import ops
    from pixtrack_amd.optimizer import cstride_for
    from pixtrack_amd.unet import OUTPUT_DIMS

    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    dev = images[0].device
    if sizes[0] == sizes[1]:
        need = int(_lib.lib().pxt_unet_workspace_bytes_batch(net._ctx, 2, *sizes[0]))
    else:
        Hs, Ws = (C.c_int32 * 2)(sizes[0][0], sizes[1][0]), (C.c_int32 * 2)(sizes[0][1], sizes[1][1])
        need = int(_lib.lib().pxt_unet_workspace_bytes_pair(net._ctx, Hs, Ws))
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    outs = [torch.full((h, w, cstride_for(c)), float("nan"), device=dev)
            for hw in sizes for (h, w), c in zip(net.level_shapes(*hw), OUTPUT_DIMS)]
    ops.unet_forward_batch(int(net._ctx.value), list(images), [None, None], [False, True], outs, ws,
                           first["p3d"], first["pose_camera"], first["ints"], second["p3d"], second["pose_camera"],
                           second["ints"])
    torch.cuda.synchronize()
    return outs[:3], outs[3:], ws


def query_points(fw, fh, rng):
    """A cluster in the left third (so that tiles stay uncomputed), seam and border points, one outside, one behind."""
    pts = [(float(rng.uniform(4, fw / 3)), float(rng.uniform(4, fh - 4)), 1.0) for _ in range(24)]
    pts += [(15.999, 20.0, 1.0), (16.0, 31.999, 1.0), (2.0, fh - 1.0, 1.0), (0.0, 0.0, 1.0), (-3.0, 5.0, 1.0),
            (8.0, 8.0, -1.0)]
    return np.ascontiguousarray(np.asarray(pts, np.float32))


def tiles_info(net, sizes):
    """pxt_unet_query_tiles -> (offset, tile rows, tiles per row, rows of tiles, the last pass wrote the flags)."""
    info = (C.c_int64 * 5)()
    Hs, Ws = (C.c_int32 * 2)(sizes[0][0], sizes[1][0]), (C.c_int32 * 2)(sizes[0][1], sizes[1][1])
    _lib.check(_lib.lib().pxt_unet_query_tiles(net._ctx, Hs, Ws, info), "pxt_unet_query_tiles")
    return tuple(int(x) for x in info)


def table_camera(name, fw, fh):
    """-> (10 floats, ndist): the camera `name` of tests/camera_cases.py scaled to an fw x fh map."""
    import camera_cases as CC
    from pixtrack_amd.geometry import Camera

    cam = Camera.from_colmap(CC.colmap(name)).scale((fw / CC.WIDTH, fh / CC.HEIGHT))
    return [float(x) for x in cam.as10()], CC.NDIST[name]


def behind_pinhole(xyz, cam10):
    """Points given as (u, v, z) with pixel coordinates of a unit camera -> camera-frame points whose PINHOLE projection
    through cam10 is (u, v): the distortion then moves them by a fraction of a texel."""
    xyz = np.asarray(xyz, np.float64)
    z = xyz[:, 2]
    return np.ascontiguousarray(np.stack([(xyz[:, 0] - cam10[4]) / cam10[2] * z, (xyz[:, 1] - cam10[5]) / cam10[3] * z, z],
                                         1).astype(np.float32))


def pair_problem(net, device, hw, margin, ref_hw=None, camera=None):
    """Two random images (the reference of ``ref_hw``, the query of ``hw``) and their records.  ``camera``: a name of
    tests/camera_cases.py - the query's record carries that camera (scaled to the fine map) in place of the unit one."""
    H, W = hw
    g = torch.Generator().manual_seed(H * 7 + W)
    images = [(torch.rand(h, w, 3, generator=g) * 255).to(device).contiguous() for h, w in (ref_hw or hw, hw)]
    fh, fw = net.level_shapes(H, W)[0]
    rh, rw = net.level_shapes(*(ref_hw or hw))[0]
    rng = np.random.default_rng(H + W + margin)
    xyz = query_points(fw, fh, rng)
    ref_xyz = np.ascontiguousarray(np.asarray([(float(rng.uniform(2, rw - 3)), float(rng.uniform(2, rh - 3)), 1.0)
                                               for _ in range(40)], np.float32))
    first = {"p3d": torch.from_numpy(ref_xyz).to(device), "ints": [0, 0, 0, 0, 0, 0],
             "pose_camera": IDENTITY + [float(rw), float(rh), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0]}
    cam10, ndist = [float(fw), float(fh), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0], 0
    if camera is not None:
        cam10, ndist = table_camera(camera, fw, fh)
        xyz = behind_pinhole(xyz, cam10)
    second = {"p3d": torch.from_numpy(xyz).to(device), "ints": [ndist, 4, 0, 0, 0, 0, margin],
              "pose_camera": IDENTITY + cam10}
    return images, xyz, first, second


def same_bits(maps_a, maps_b):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(maps_a, maps_b))


def check_pair_pass(net, device, hw, margin, ref_hw=None, uses_record=True, camera=None):
    """The pair pass with the query's record against the dense one.  ``uses_record`` False: a pass that has to compute
    every tile (one batched pass) - it says so, and the map is the dense pass's throughout."""
    H, W = hw
    sizes = [ref_hw or hw, hw]
    images, xyz, first, second = pair_problem(net, device, hw, margin, ref_hw, camera)
    fh, fw = net.level_shapes(H, W)[0]
    net.set_query_tiles(False)
    try:
        ref_dense, qry_dense, _ = pair_pass(net, images, first, second)  # (option off: the record is ignored)
        assert tiles_info(net, sizes)[4] == 0  # ... and the pass says that it wrote no flags: no guard for the LM
    finally:
        net.set_query_tiles(True)
    ref_got, qry_got, ws = pair_pass(net, images, first, second)
    off, rows, per_row, n_rows, used = tiles_info(net, sizes)
    assert all(bool(torch.isfinite(m).all()) for m in qry_dense)
    # the reference image's maps (it computes its own tiles either way) and the query's two coarser maps: unchanged
    assert same_bits(ref_got, ref_dense)
    assert torch.equal(qry_got[1], qry_dense[1]) and torch.equal(qry_got[2], qry_dense[2])
    assert rows == TILE and per_row == -(-fw // 16) and n_rows == -(-fh // rows)
    if not uses_record:
        assert used == 0 and same_bits(qry_got, qry_dense)
        return
    # the device flags are the host replica's, which is the rule's restatement (tests/test_query_tiles.py)
    assert used == 1
    dev_flags = ws[off:off + per_row * n_rows].cpu().numpy().reshape(n_rows, per_row)
    rec = record(xyz, margin, (0, 0, fw, fh), False)
    if camera is None:
        want = replica_fine(xyz, fh, fw, margin)
    else:  # (the host statement against a float64 restatement on this camera: tests/test_projection_host.py)
        rec.points.cam[:], rec.points.ndist = table_camera(camera, fw, fh)
        want, _ = host_flags(rec, fh, fw)
    host, _ = host_flags(rec, fh, fw)
    assert np.array_equal(host, want) and np.array_equal(dev_flags, want)
    assert 0 < want.sum() < want.size
    # every flagged tile is the dense pass's, bit for bit; every other record is still NaN
    for r in range(n_rows):
        for c in range(per_row):
            a = qry_got[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]
            if want[r, c]:
                assert torch.equal(a, qry_dense[0][r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE]), (r, c)
            else:
                assert bool(torch.isnan(a).all()), (r, c)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,margin", [((76, 100), 4), ((76, 100), 0), ((48, 64), 4)])
def test_pair_pass_with_the_query_record_equals_the_dense_pass_on_its_tiles(net, device, hw, margin):
    check_pair_pass(net, device, hw, margin)


@pytest.mark.gpu
def test_pair_pass_under_the_opencv_camera(net, device):
    """The smallest image of this file, the query's record carrying the OPENCV camera (ndist 4): the device's flags are
    the host statement's, every flagged tile is the dense pass's bit for bit, no other tile is written."""
    check_pair_pass(net, device, (48, 64), 4, camera="opencv")


@pytest.mark.gpu
def test_the_guard_hand_off_follows_the_pass_with_one_stream(device):
    """PXT_UNET_STREAMS=1 (read once per process: a fresh child, this file's __main__).  A pair of two sizes - a
    reference camera at another scale - still runs as two single-image passes, and the query's leaves tiles out: the
    flags must be handed on (the LM reading an unwritten tile with no guard is the failure).  A pair of one size runs as
    ONE batched pass, which computes every tile: no flags, and the map is the dense pass's."""
    env = dict(os.environ, PXT_UNET_STREAMS="1", PYTHONPATH=os.pathsep.join([str(ROOT), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, str(Path(__file__).resolve())], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert "ONE_STREAM_OK" in out.stdout, out.stdout[-2000:]


@pytest.mark.gpu
def test_the_redone_query_pass_has_the_bits_of_the_pair_pass_without_the_record(net, device):
    """After a guard trip the query pass runs again alone.  At 640 x 480 a lone pass is planned differently from one image
    of the pair (other tile configurations and split-K partitions: other summation orders, other fp16 bits), so the redo
    is planned as the pair's second image (pxt_unet_forward_pair_second): every map of it is the option-off pair pass's."""
    H, W = 480, 640
    keys = ("cfg", "splits", "deep_ring")
    lone, pair = net.layer_views(1, H, W, 1), net.layer_views(1, H, W, 2)
    assert any(tuple(a[k] for k in keys) != tuple(b[k] for k in keys) for a, b in zip(lone[:17], pair[:17]))
    images, xyz, first, second = pair_problem(net, device, (H, W), 8)
    net.set_query_tiles(False)
    try:
        _, qry_dense, _ = pair_pass(net, images, first, second)
    finally:
        net.set_query_tiles(True)
    _, qry_got, ws = pair_pass(net, images, first, second)
    assert tiles_info(net, [(H, W), (H, W)])[4] == 1 and bool(torch.isnan(qry_got[0]).any())
    net.forward_pair_second((images[1], None, True), qry_got, [(H, W), (H, W)], workspace=ws)
    torch.cuda.synchronize()
    assert tiles_info(net, [(H, W), (H, W)])[4] == 0  # (the flags no longer describe the maps)
    assert same_bits(qry_got, qry_dense)


# ---- the LM's tile guard on synthetic maps ---------------------------------------------------------------------------------
FH, FW = 48, 64          # the fine map: C = 32, cstride 36, tiles of 16 x 16
KNOWN = (16.4, 24.3)     # the known point: starts right of the tile seam at x = 16 and ends with its footprint across it
SHIFT = (3.0, 2.0)       # the start pose moves every point by (3, 2) fine pixels: at most 4


def smooth_map(h, w, C, cs, stride, seed):
    """map[Y, X, c] = g_c(stride X, stride Y) for smooth g_c; channel C (the confidence) is 1 -> (map, g)."""
    rng = np.random.default_rng(seed)
    a, b, ph = rng.uniform(0.04, 0.22, C), rng.uniform(0.04, 0.22, C), rng.uniform(0, 6.28, C)

    def g(x, y):
        return np.sin(np.multiply.outer(x, a) + np.multiply.outer(y, b) + ph).astype(np.float32)

    Y, X = np.meshgrid(np.arange(h) * float(stride), np.arange(w) * float(stride), indexing="ij")
    m = np.zeros((h, w, cs), np.float32)
    m[..., :C] = g(X, Y)
    m[..., C] = 1.0
    return m, g


def lm_problem(n, device, cam10=None, ndist=0):
    """``cam10`` / ``ndist``: the fine level's camera in place of the unit one; the points are then camera-frame points
    whose pinhole projections are the same pixels, and the references are the maps' functions at their float64
    projections through the whole model (the identity pose is the optimum, as with the unit camera)."""
    rng = np.random.default_rng(n)
    # (their footprints stay right of x = 17, and the margin-8 tiles of case (b) leave the last column of tiles out)
    xy = np.stack([rng.uniform(21, 34, n), rng.uniform(12, 30, n)], 1)
    xy[0] = KNOWN
    p3d = np.concatenate([xy, np.ones((n, 1))], 1).astype(np.float32)
    if cam10 is not None:
        from oracle import lm_oracle as O

        p3d = behind_pinhole(p3d, cam10)
        uv, ok = O.world2image(torch.tensor(cam10[:6 + ndist], dtype=torch.float64), torch.from_numpy(p3d).double())
        assert bool(ok.all())
        xy = uv.numpy()
    fine, g_fine = smooth_map(FH, FW, 32, 36, 1, 11)
    coarse, g_coarse = smooth_map(FH // 4, FW // 4, 128, 132, 4, 12)
    fref_f = np.zeros((n, 36), np.float32)
    fref_f[:, :32], fref_f[:, 32] = g_fine(xy[:, 0], xy[:, 1]), 1.0
    fref_c = np.zeros((n, 132), np.float32)
    fref_c[:, :128], fref_c[:, 128] = g_coarse(xy[:, 0], xy[:, 1]), 1.0
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    return {"p3d": t(p3d), "xyz": p3d, "fine": t(fine), "coarse": t(coarse), "fref_f": t(fref_f), "fref_c": t(fref_c)}


def lm_launch(prob, path, fine_map=None, flags=None, cam10=None, ndist=0, T0=None):
    """The C = 128 level without flags, then the fine level; -> (record [NH], log [2, iters, 20], camera record [13]).
    ``cam10`` / ``ndist``: the fine level's camera (the coarse level's is its quarter, as with the unit camera)."""
    from pixtrack_amd.ops import ops

    dev = prob["p3d"].device
    num_iters = 12
    rec = torch.zeros(NH + 2 * num_iters * _lib.PXT_LM_LOG_STRIDE, dtype=torch.float32).pin_memory()
    cam_out = torch.zeros(16, dtype=torch.float32).pin_memory()
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=dev)
    cams = [FW / 4, FH / 4, 0.25, 0.25, 0.0, 0.0, 0, 0, 0, 0, float(FW), float(FH), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0]
    if cam10 is not None:
        cams = [FW / 4, FH / 4] + [x / 4 for x in cam10[2:6]] + list(cam10[6:]) + list(cam10)
    conv27 = [0.0, 0.0, 0.0, 1.0] + [1.0 if i % 5 == 0 else 0.0 for i in range(16)] + [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    T0 = IDENTITY[:9] + [SHIFT[0], SHIFT[1], 0.0] if T0 is None else T0
    guard = (-1, None, None) if flags is None else (1, flags, [TILE, FW // 16, 0, 0])
    ops.lm_refine(prob["p3d"], None, [prob["coarse"], prob["fine"] if fine_map is None else fine_map],
                  [prob["fref_c"], prob["fref_f"]], [128, 32], cams, [ndist, ndist], [0.01] * 12, T0, num_iters, 2, 0, 0.0, 1.0,
                  1e-9, 1e-4, 1e-4, 10, 0, rec, ws, True, 0, conv27, None, cam_out, path, *guard)
    torch.cuda.synchronize()
    r = rec.numpy().copy()
    return r[:NH], r[NH:].reshape(2, num_iters, _lib.PXT_LM_LOG_STRIDE), cam_out.numpy()[:13].copy()


def known_point_track(head, log):
    """u of the known point at the pose every fine iteration STARTS from (float64 on the logged float32 poses)."""
    it_c, it_f = int(head[16]), int(head[17])
    start = log[0, it_c - 1, 8:20] if it_c > 0 else np.asarray(IDENTITY[:9] + [SHIFT[0], SHIFT[1], 0.0], np.float32)
    poses = [start] + [log[1, i, 8:20] for i in range(it_f - 1)]
    us = []
    for T in np.asarray(poses, np.float64):
        p = T[:9].reshape(3, 3) @ np.asarray([KNOWN[0], KNOWN[1], 1.0]) + T[9:]
        us.append(p[0] / p[2])
    return us


@pytest.mark.gpu
@pytest.mark.parametrize("n,path", [(64, 0), (500, 0), (64, 2), (500, 2)])
def test_lm_tile_guard(device, n, path):
    prob = lm_problem(n, device)
    plain_head, plain_log, plain_cam = lm_launch(prob, path)
    assert plain_head[12] == 0 and plain_head[13] == 0 and plain_head[15] == 1 and plain_cam[12] == 1
    it_c, it_f = int(plain_head[16]), int(plain_head[17])
    assert it_c >= 1 and it_f >= 2, (it_c, it_f)
    ones = torch.ones(FH // TILE, FW // 16, dtype=torch.uint8, device=device)

    def same_bits(got, want):
        return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))

    # (a) all flags set: the launch without flags, bit for bit, and log word 6 is 0 throughout
    a = lm_launch(prob, path, flags=ones)
    assert same_bits(a, (plain_head, plain_log, plain_cam))
    assert not a[1][:, :, 6].any()
    # (b) flags from the rule at the start pose, margin 8, the map NaN wherever they are 0: the bits of (a)
    pts = record(prob["xyz"], 8, (0, 0, FW, FH), False, pad=2)
    pts.points.T[:] = IDENTITY[:9] + [SHIFT[0], SHIFT[1], 0.0]
    host, _ = host_flags(pts, FH, FW)
    assert 0 < host.sum() < host.size
    holes = prob["fine"].clone()
    mask = torch.from_numpy(np.repeat(np.repeat(host, TILE, 0), TILE, 1)[:FH, :FW].astype(bool)).to(device)
    holes[~mask] = float("nan")
    b = lm_launch(prob, path, fine_map=holes, flags=torch.from_numpy(host).to(device))
    assert same_bits(b, a)
    # (c) the whole map computed, the flag of tile (1, 0) cleared: only the known point's footprint ever reaches it -
    # columns floor(u) - 1 .. floor(u) + 2 meet x < 16 once u < 17 - at the first fine iteration that starts with u < 17
    us = known_point_track(plain_head, plain_log)
    assert all(abs(u - 17.0) > 1e-3 for u in us), us  # (the restatement is not decided by rounding)
    hits = [i for i, u in enumerate(us) if u < 17.0]
    assert hits, us  # (it converges towards u = 16.4)
    k = hits[0]
    cleared = ones.clone()
    cleared[1, 0] = 0
    head, log, cam = lm_launch(prob, path, flags=cleared)
    assert head[13] == float(_lib.PXT_E_GUARD) and head[12] == 1 and head[15] == 1  # (not the spin time-out's status)
    assert int(head[16]) == it_c and int(head[17]) == k + 1 and int(head[14]) == it_c + k + 1  # the launch stops there
    assert not log[0, :, 6].any() and not log[1, :k, 6].any() and log[1, k, 6] == 1.0
    assert cam[12] == -1.0  # the camera record is marked, the slots are left alone
    # what ran before the trip is what ran without flags; the pose handed back is the one iteration k started from
    assert np.array_equal(log[0].view(np.uint32), plain_log[0].view(np.uint32))
    assert np.array_equal(log[1, :k].view(np.uint32), plain_log[1, :k].view(np.uint32))
    before = plain_log[1, k - 1, 8:20] if k > 0 else plain_log[0, it_c - 1, 8:20]
    assert np.array_equal(head[:12].view(np.uint32), before.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("path", [0, 2])
def test_lm_tile_guard_reports_nothing_under_the_opencv_camera(device, path):
    """Case (b) above with the OPENCV camera (ndist 4) on the fine level: the flags of the marking rule at the start pose
    (margin 8), the map NaN wherever they are 0.  The marking and the LM project through the same project_point, so the
    guard reports no unmarked tile and the run is the all-flags run bit for bit."""
    cam10, ndist = table_camera("opencv", FW, FH)
    n = 64
    prob = lm_problem(n, device, cam10, ndist)
    T0 = IDENTITY[:9] + [SHIFT[0] / cam10[2], SHIFT[1] / cam10[3], 0.0]  # (3, 2) fine pixels at z = 1
    ones = torch.ones(FH // TILE, FW // 16, dtype=torch.uint8, device=device)
    a = lm_launch(prob, path, flags=ones, cam10=cam10, ndist=ndist, T0=T0)
    assert a[0][12] == 0 and a[0][13] == 0 and a[0][15] == 1 and not a[1][:, :, 6].any()
    assert int(a[0][16]) >= 1 and int(a[0][17]) >= 2
    pts = record(prob["xyz"], 8, (0, 0, FW, FH), False, pad=2)
    pts.points.T[:] = T0
    pts.points.cam[:], pts.points.ndist = cam10, ndist
    host, _ = host_flags(pts, FH, FW)
    assert 0 < host.sum() < host.size
    holes = prob["fine"].clone()
    mask = torch.from_numpy(np.repeat(np.repeat(host, TILE, 0), TILE, 1)[:FH, :FW].astype(bool)).to(device)
    holes[~mask] = float("nan")
    b = lm_launch(prob, path, fine_map=holes, flags=torch.from_numpy(host).to(device), cam10=cam10, ndist=ndist, T0=T0)
    assert b[0][13] == 0 and not b[1][:, :, 6].any()  # the guard reports no unmarked tile
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(b, a))


# ---- the tracker ---------------------------------------------------------------------------------------------------------
def displaced(tr, pixels):
    """The tracker's pose moved sideways by about ``pixels`` fine pixels at the object's depth."""
    from pixtrack_amd.geometry import Pose

    rot, t = tr.pose.numpy()
    t = np.asarray(t, np.float64).copy()
    t[0] += pixels * t[2] / float(tr.camera.f[0])
    return Pose.from_Rt(np.asarray(rot, np.float64), t)


def run_tracker(device, assets, on, margin=None, segment=None, push=None):
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import render_query_frames

    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=1, device=device, assets=assets)
    tr.spp = 2
    tr.query_tiles = on
    if margin is not None:
        tr.query_tile_margin = margin
    refiner = tr.localizer.refiner
    frames = render_query_frames(assets, tr.testbed, cold_start_indices=(0,) if segment is None else (0, segment))
    used, tripped = [], []
    for i, f in enumerate(frames):
        if segment is not None and i == segment:  # a segment head about 20 fine pixels off the last pose
            tr.start_segment(displaced(tr, 20.0))
        if push is not None and i == push:  # the same push on a steady frame, which starts its LM from it
            tr.pose = displaced(tr, 20.0)
        before = refiner.query_tile_frames, refiner.query_tile_fallbacks
        tr.run_single_frame((f"{i:06d}.png", f))
        used.append(refiner.query_tile_frames > before[0])
        tripped.append(refiner.query_tile_fallbacks > before[1])
    tr.tripped = tripped
    rows = []
    for i in range(len(used)):
        ret = tr.pose_history[f"{i:06d}.png"]
        rows.append((ret["success"], ret.get("cost"), ret.get("T_refined", ret["T_init"]).as12().detach().cpu()))
    return rows, used, tr


def same_rows(rows_a, rows_b):
    return len(rows_a) == len(rows_b) and all(
        ok_a == ok_b and cost_a == cost_b and torch.equal(T_a, T_b)
        for (ok_a, cost_a, T_a), (ok_b, cost_b, T_b) in zip(rows_a, rows_b))


@pytest.mark.gpu
def test_tracked_poses_do_not_change_with_query_tiles(device):
    """The frames of test_tracked_poses_do_not_change (160 x 120, four of them), option on against off."""
    from pixtrack_amd.synthetic import make_tracking_assets

    assets = make_tracking_assets(seed=1011, width=160, height=120, n_frames=4, n_points=3000)
    rows_on, used_on, tr_on = run_tracker(device, assets, True)
    rows_off, used_off, tr_off = run_tracker(device, assets, False)
    assert sum(used_on) >= 2 and not any(used_off)
    assert any(ok for ok, _, _ in rows_on)
    assert same_rows(rows_on, rows_off)
    assert tr_on.query_tile_fallbacks == 0 and tr_on.localizer.refiner.query_tile_fallbacks == 0


@pytest.mark.gpu
def test_a_guard_trip_redoes_the_frame_and_rests_the_option(device):
    """Margin 0 and a start pose about 20 fine pixels off: the guard trips, the frame is redone in full - the poses are
    those of the option-off run - and the option rests for 8 frames (twelve frames, so that its return is seen).

    The push comes twice.  Frame 1 is a segment head (start_segment) 20 pixels off: a cold start, which runs without the
    option and finds the pose again, so by itself it trips nothing (measured: 0 fallbacks in 12 frames).  Frame 2, the
    first steady frame, therefore has its pose pushed by the same 20 pixels: its LM launch carries the guard and starts
    from there."""
    from pixtrack_amd.synthetic import make_tracking_assets

    assets = make_tracking_assets(seed=1011, width=160, height=120, n_frames=12, n_points=3000)
    rows_on, used, tr = run_tracker(device, assets, True, margin=0, segment=1, push=2)
    rows_off, used_off, tr_off = run_tracker(device, assets, False, margin=0, segment=1, push=2)
    assert not any(used_off) and tr_off.query_tile_fallbacks == 0
    assert tr.query_tile_fallbacks >= 1 and tr.query_tile_fallbacks == tr.localizer.refiner.query_tile_fallbacks
    assert same_rows(rows_on, rows_off)
    # the pushed frame's launch carried the guard and tripped it; the eight frames after it run without the option, the
    # ninth - a steady frame - carries it again
    first = tr.tripped.index(True)
    assert first == 2 and used[first]
    assert tr.renders_ahead_rejected >= 1
    assert first + 9 < len(used), used
    assert not any(used[first + 1:first + 9]) and used[first + 9], used


if __name__ == "__main__":  # the child of test_the_guard_hand_off_follows_the_pass_with_one_stream
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    assert os.environ.get("PXT_UNET_STREAMS") == "1"
    dev = torch.device("cuda:0")
    child_net = UNet(make_synthetic_unet_weights(7), dev)
    check_pair_pass(child_net, dev, (76, 100), 4, ref_hw=(48, 64))
    check_pair_pass(child_net, dev, (48, 64), 4, uses_record=False)
    print("ONE_STREAM_OK")
