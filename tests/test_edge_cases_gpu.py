"""Edge cases and size-independent properties of the hot path through the C ABI: argument
errors, degenerate inputs, and full-size (BASELINE configs[1]) invariants that need no oracle run."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd.geometry import Pose
from pixtrack_amd.ngp import RenderMode, Testbed
from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for
from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, look_at_pose, make_lm_scene, make_synthetic_nerf
from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ C-ABI argument errors
def test_entry_points_reject_bad_arguments(device):
    L = _lib.lib()
    ws = torch.zeros(int(L.pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
    out = torch.zeros(24, device=device)
    p3d = torch.zeros(16, 3, device=device)
    conf = PixTrackOptimizer(dict(num_iters=5)).native_conf()
    lv = (_lib.LmLevel * 1)()
    T0 = (C.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    # null map pointers / zero points / too many levels
    assert L.pxt_lm_refine(p3d.data_ptr(), None, 16, lv, 1, T0, C.byref(conf), out.data_ptr(), None, ws.data_ptr(),
                           None) == -1
    assert L.pxt_lm_refine(p3d.data_ptr(), None, 0, lv, 1, T0, C.byref(conf), out.data_ptr(), None, ws.data_ptr(),
                           None) == -1
    assert L.pxt_lm_refine(p3d.data_ptr(), None, 16, lv, 9, T0, C.byref(conf), out.data_ptr(), None, ws.data_ptr(),
                           None) == -1
    assert L.pxt_unet_create(None, 0, C.byref(C.c_void_p())) == -1
    assert L.pxt_ngp_render(None, None, None, None, None) == -1
    assert L.pxt_depth_mask(None, 4, 4, 1, 5, None, None, None) == -1
    # round-4 entry points: a render with no output for an image its mode produces, a mask from no plane, an LM launch
    # whose camera request names neither a slot nor a record
    assert L.pxt_depth_mask_plane(None, 4, 4, 1, 5, None, None, None) == -1
    assert L.pxt_ngp_render_frame(None, None, 0, 0, None, None, None) == -1
    assert L.pxt_ngp_camera_slot(None) is None
    assert L.pxt_unet_activation_stats(None, 64, 64, None, None, None) == -1
    cam = _lib.LmCamera()
    assert L.pxt_lm_refine_cam(p3d.data_ptr(), None, 16, lv, 1, T0, C.byref(conf), out.data_ptr(), None, ws.data_ptr(),
                               C.byref(cam), None) == -1
    with pytest.raises(_lib.PxtError):
        _lib.check(-1, "probe")


def test_mask_ops_reject_outputs_the_kernels_cannot_write(device):
    """The mask kernels write a dense [H][W] byte plane, four bytes per store when W % 4 == 0 (include/pixtrack_hip.h):
    a strided view, a host tensor or - at such a W - a misaligned one is an error, and nothing is written."""
    from pixtrack_amd.ops import ops

    H, W = 8, 12
    nz = torch.ones(H, W, dtype=torch.uint8, device=device)
    depth = torch.ones(H, W, 4, device=device)
    scratch = torch.empty(2 * H * W, dtype=torch.uint8, device=device)
    wide = torch.full((H, 2 * W), 7, dtype=torch.uint8, device=device)
    flat = torch.full((H * W + 4,), 7, dtype=torch.uint8, device=device)
    tall = torch.full((W, H), 7, dtype=torch.uint8, device=device)
    bad = {"strided": wide[:, :W], "transposed": tall.t(), "host": torch.full((H, W), 7, dtype=torch.uint8),
           "misaligned": flat[1:1 + H * W].view(H, W), "wrong shape": flat[:H * W].view(W, H),
           "wrong dtype": torch.zeros(H, W, dtype=torch.int8, device=device)}
    assert bad["misaligned"].data_ptr() % 4 == 1 and bad["misaligned"].is_contiguous()
    for name, mask in bad.items():
        with pytest.raises(_lib.PxtError):
            ops.depth_mask_plane(nz, 1, 1, mask)
        with pytest.raises(_lib.PxtError):
            ops.depth_mask(depth, 1, 1, mask, scratch)
    with pytest.raises(_lib.PxtError):  # the float entry's scratch holds 2 * H * W bytes
        ops.depth_mask(depth, 1, 1, flat[:H * W].view(H, W), scratch[:H * W])
    torch.cuda.synchronize()
    assert bool((wide == 7).all()) and bool((flat == 7).all()) and bool((tall == 7).all())
    ops.depth_mask_plane(nz, 1, 1, flat[4:4 + H * W].view(H, W))  # aligned: runs, and an all-lit plane stays all lit
    assert bool((flat[4:] == 1).all()) and bool((flat[:4] == 7).all())


def test_unet_rejects_images_it_cannot_encode(device):
    net = UNet(make_synthetic_unet_weights(1), device)
    with pytest.raises(_lib.PxtError):  # 8 px: the fourth pooling would have nothing left
        net.forward_packed(torch.zeros(8, 8, 3, device=device), None, False)
    with pytest.raises(_lib.PxtError):  # a batch of more than two holds one image size (checked by the op; exactly
        # two images of two sizes are the pair entry: tests/test_unet_gpu.py)
        net.forward_packed_batch([(torch.zeros(32, 32, 3, device=device), None, False),
                                  (torch.zeros(32, 48, 3, device=device), None, False),
                                  (torch.zeros(32, 32, 3, device=device), None, False)])
    with pytest.raises(_lib.PxtError):  # ... and a pair one of whose images cannot be encoded
        net.forward_packed_batch([(torch.zeros(32, 32, 3, device=device), None, False),
                                  (torch.zeros(8, 8, 3, device=device), None, False)])
    with pytest.raises(_lib.PxtError):  # PXT_UNET_MAX_BATCH
        net.forward_packed_batch([(torch.zeros(32, 32, 3, device=device), None, False)] * 17)


# ------------------------------------------------------------------ LM degenerate inputs
def _packs(sc, device):
    lam = [10.0 ** (-6 + torch.sigmoid(torch.full((6,), -2.0)) * 11) for _ in range(3)]
    packs = []
    for level in reversed(range(3)):
        fq = sc.feats_query[level]
        Cc = fq.shape[0] - 1
        cs = cstride_for(Cc)
        fmap = torch.zeros(fq.shape[1], fq.shape[2], cs)
        fmap[..., :Cc] = (fq[:-1] / fq[:-1].norm(dim=0, keepdim=True).clamp_min(1e-12)).permute(1, 2, 0)
        fmap[..., Cc] = fq[-1]
        fr = sc.feats_ref[level]
        fref = torch.zeros(fr.shape[0], cs)
        fref[:, :Cc] = fr[:, :-1] / fr[:, :-1].norm(dim=1, keepdim=True).clamp_min(1e-12)
        fref[:, Cc] = fr[:, -1]
        packs.append(LevelPack(fmap.to(device), fref.to(device), Cc, sc.camera.scale(sc.scales[level]), lam[level]))
    return packs


def test_lm_all_points_behind_the_camera_or_outside_the_image(device):
    """No valid point at all: failed, pose returned unchanged, no NaN anywhere in the record."""
    sc = make_lm_scene(seed=1007, width=160, height=120, n_points=300, sigma_px=2.0)
    packs = _packs(sc, device)
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
    conf = PixTrackOptimizer(dict(num_iters=20, pad=1)).native_conf()
    behind = torch.from_numpy(sc.p3d).float().to(device)
    R, t = sc.T_init.R.double().numpy(), sc.T_init.t.double().numpy()
    flip = Pose.from_Rt(torch.from_numpy(np.diag([1.0, 1.0, -1.0]) @ R), torch.from_numpy(np.diag([1.0, 1.0, -1.0]) @ t))
    for T0 in (flip, Pose.from_Rt(torch.from_numpy(R), torch.from_numpy(t + np.array([50.0, 0.0, 0.0])))):
        res = PixTrackOptimizer.refine_levels(behind, packs, T0, conf, ws).result()
        assert res.failed and res.total_iters == 1
        assert torch.isfinite(res.T.as12()).all()
        assert torch.allclose(res.T.as12(), T0.as12().float(), atol=1e-6)


def test_lm_single_point_and_odd_counts(device):
    """N = 1 (and N not a multiple of the lane-group size) run without touching memory past N."""
    for n in (1, 11, 257):
        sc = make_lm_scene(seed=1008, width=160, height=120, n_points=n, sigma_px=2.0)
        packs = _packs(sc, device)
        ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
        conf = PixTrackOptimizer(dict(num_iters=30, pad=1)).native_conf()
        p3d = torch.from_numpy(sc.p3d).float().to(device)
        res = PixTrackOptimizer.refine_levels(p3d, packs, sc.T_init, conf, ws).result()
        assert torch.isfinite(res.T.as12()).all()
        assert res.failed == (n < 10)


def test_lm_is_bitwise_repeatable_at_full_size(device):
    """Fixed-order cross-workgroup reduction: the same inputs give the same bits, run after run."""
    sc = make_lm_scene(seed=1009, width=640, height=480, n_points=2287, sigma_px=2.0)
    packs = _packs(sc, device)
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
    conf = PixTrackOptimizer(dict(num_iters=150, pad=1)).native_conf()
    p3d = torch.from_numpy(sc.p3d).float().to(device)
    first = PixTrackOptimizer.refine_levels(p3d, packs, sc.T_init, conf, ws).result()
    for _ in range(4):
        again = PixTrackOptimizer.refine_levels(p3d, packs, sc.T_init, conf, ws).result()
        assert torch.equal(first.T.as12(), again.T.as12()) and first.iters == again.iters
        assert first.costs == again.costs
    assert not first.failed


# ------------------------------------------------------------------ NeRF full-size properties
@pytest.fixture(scope="module")
def testbed(device):
    tb = Testbed(device=device)
    tb.load_snapshot(make_synthetic_nerf(11))
    tb.background_color = [255, 255, 255, 0.0]
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = 1e-7
    tb.render_aabb.min, tb.render_aabb.max = PREMIER_PROTEIN_AABB
    lo, hi = np.array(PREMIER_PROTEIN_AABB)
    c = 0.5 * (lo + hi)
    eye = c + np.array([0.9, 0.5, 0.3]) / np.linalg.norm([0.9, 0.5, 0.3]) * 1.69
    R, _ = look_at_pose(eye, c, up=np.array([0, 1.0, 0]))
    tb._cam_ngp = np.concatenate([R.T, eye[:, None]], 1)
    tb.fov = math.degrees(2 * math.atan(640 / (2 * 1.2 * 640)))
    return tb


def test_full_size_render_properties(testbed):
    """640x480, spp 8 (BASELINE configs[1]) without an oracle run: bit-repeatable (the live-ray
    compaction order is not fixed, the image is), premultiplied colour bounded by alpha, alpha in
    [0, 1], background exactly zero, Depth's alpha channel equals Shade's."""
    tb = testbed
    tb.render_mode = RenderMode.Shade
    a = tb.render_device(640, 480, 8, True)
    b = tb.render_device(640, 480, 8, True)
    assert torch.equal(a, b)
    assert torch.isfinite(a).all()
    alpha = a[..., 3]
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0 + 1e-6
    assert bool((a[..., :3] <= alpha[..., None] + 1e-6).all()) and float(a[..., :3].min()) >= 0.0
    assert bool((a[alpha == 0] == 0).all())
    assert 0.05 < float((alpha > 0.5).float().mean()) < 0.5
    tb.render_mode = RenderMode.Depth
    d = tb.render_device(640, 480, 8, True)
    tb.render_mode = RenderMode.Shade
    assert torch.equal(d[..., 3], alpha)
    rgba, depth = tb.render_both_device(640, 480, 8)
    assert torch.equal(rgba, a) and torch.equal(depth, d)


def test_render_of_a_camera_that_sees_nothing(testbed):
    tb = testbed
    keep = tb._cam_ngp.copy()
    tb._cam_ngp = keep.copy()
    tb._cam_ngp[:, 3] = keep[:, 3] + keep[:, 2] * -5.0  # far away ...
    tb._cam_ngp[:, 2] = -keep[:, 2]                      # ... and looking the other way
    tb._cam_ngp[:, 0] = -keep[:, 0]
    out = tb.render_device(96, 64, 4, True)
    tb._cam_ngp = keep
    assert bool((out == 0).all())


def test_single_pixel_and_ragged_renders(testbed):
    """1x1, 3x5 (smaller than one 4x2 enumeration block) and spp 1 / 5 renders complete."""
    for (w, h, spp) in ((1, 1, 1), (3, 5, 5), (7, 2, 8)):
        out = testbed.render_device(w, h, spp, True)
        assert out.shape == (h, w, 4) and torch.isfinite(out).all()


def test_three_concurrent_trackers_share_one_gpu(device):
    """Several sequences on one GPU, one Python thread + one HIP stream each (scripts/bench_multiseq.py):
    every tracker's persistent LM grid (64 workgroups, its own counters) must stay live beside the other
    trackers' renders, UNets and LM grids - no PXT_E_TIMEOUT, every frame tracked, and each sequence's
    poses equal, bit for bit, what it gets when it runs alone."""
    import threading

    from pixtrack_amd import optimizer
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    S, n = 3, 24
    seqs = []
    for k in range(S):
        assets = make_tracking_assets(seed=1040 + k, width=320, height=240, n_frames=n, n_points=4000)
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
        tr.spp = 4
        seqs.append((assets, tr, render_query_frames(assets, tr.testbed), torch.cuda.Stream(device=device)))
    torch.cuda.synchronize()
    # reference: each sequence alone
    alone = []
    for assets, tr, frames, _ in seqs:
        solo = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
        solo.spp = 4
        for i, f in enumerate(frames):
            solo.run_single_frame((f"{i:06d}.png", f))
        alone.append([solo.pose_history[f"{i:06d}.png"]["T_refined"].numpy() for i in range(n)])
    errors = []
    old_poll = optimizer.PendingLM.poll
    optimizer.PendingLM.poll = False  # several trackers on threads: wait on the event, do not spin under the GIL

    def work(k):
        try:
            _, tr, frames, stream = seqs[k]
            with torch.cuda.stream(stream):
                for i, f in enumerate(frames):
                    tr.run_single_frame((f"{i:06d}.png", f))
                stream.synchronize()
        except Exception as e:  # PxtError (in-kernel status / HIP error) would land here
            errors.append((k, repr(e)))

    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(S)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
    finally:
        optimizer.PendingLM.poll = old_poll
    assert not errors, errors
    for k, (assets, tr, frames, _) in enumerate(seqs):
        for i in range(n):
            ret = tr.pose_history[f"{i:06d}.png"]
            assert ret["success"], (k, i)
            R, t = ret["T_refined"].numpy()
            # Bit for bit the solo run's poses.  (Round 6 found them up to ~1e-3 apart: beside another stream's kernels the
            # ray generator computed single waves' rays from a slightly different camera - removed by the way the camera is
            # loaded, csrc/pxt_ngp.hip camera_pointer; profiles/r06_experiments.md sections 4 and 8.)
            assert np.array_equal(R, alone[k][i][0]) and np.array_equal(t, alone[k][i][1]), (k, i, np.abs(R - alone[k][i][0]).max())


def test_two_processes_share_one_gpu(tmp_path):
    """INTEGRATION.md "Sharing a GPU": the supported deployment is ONE tracking process per GPU (several objects go through
    MultiObjectTracker).  Two processes on one GPU are the documented edge: each LM launch takes at most half of the
    resident workgroup slots, so two fit side by side - both processes finish with every frame tracked - or, if the
    persistent launches do starve each other, a process ends with PxtError (in-kernel status -3, the bounded spin) within
    seconds: never a hang, never a silently wrong pose."""
    import subprocess
    import sys
    import textwrap
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {str(root)!r})
        import numpy as np, torch
        from pixtrack_amd import _lib
        from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
        from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames
        seed = int(sys.argv[1])
        dev = torch.device("cuda:0")
        assets = make_tracking_assets(seed=seed, width=320, height=240, n_frames=40, n_points=4000)
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
        tr.spp = 4
        frames = render_query_frames(assets, tr.testbed)
        try:
            for i, f in enumerate(frames):
                tr.run_single_frame((f"{{i:06d}}.png", f))
            torch.cuda.synchronize()
        except _lib.PxtError as e:
            print("PXTERROR", e)
            sys.exit(3)
        ok = sum(bool(tr.pose_history[f"{{i:06d}}.png"]["success"]) for i in range(len(frames)))
        rot = []
        for i in range(1, len(frames)):
            R, t = tr.pose_history[f"{{i:06d}}.png"]["T_refined"].numpy()
            Rg, tg = assets["gt_poses"][i]
            rot.append(float(np.arccos(np.clip((np.trace(R @ Rg.T) - 1) / 2, -1, 1))))
        print("TRACKED", ok, len(frames), max(rot))
    """)
    script = tmp_path / "one_tracker.py"
    script.write_text(code)
    procs = [subprocess.Popen([sys.executable, str(script), str(1060 + k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    finished = 0
    for p, (out, err) in zip(procs, outs):
        if p.returncode == 0:
            line = next(l for l in out.splitlines() if l.startswith("TRACKED"))
            _, ok, n, worst = line.split()
            assert int(ok) == int(n) and float(worst) < 2e-2, line  # every frame tracked, near the synthetic ground truth
            finished += 1
        else:  # the documented failure mode, and only that one
            assert p.returncode == 3 and "PXTERROR" in out and "status -3" in out, (p.returncode, out[-500:], err[-1500:])
    assert finished >= 1


def test_renders_beside_another_streams_unet_passes_keep_their_bits(device):
    """Round 6's concurrency defect (profiles/r06_experiments.md section 8): with UNet passes running on another HIP stream,
    about one render in six came back with a few 4 x 2 pixel blocks changed - single waves of the ray generator had computed
    from a slightly different camera (mechanism not established).  240 renders on one stream beside 60 eight-image UNet passes on
    another: every float and 8-bit plane equals the render made alone."""
    from pixtrack_amd import parallel
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    obj = parallel.load_object_configs()[0]
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=3, aabb=obj["aabb"])
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
    frames = render_query_frames(assets, tr.testbed, first_frame_sigma=24.0)
    for i in range(3):
        tr.run_single_frame((f"{i:06d}.png", frames[i]))
    torch.cuda.synchronize()
    tb, model, mask = tr.testbed, tr.localizer.extractor.model, tr.localizer.refiner.query_mask
    ref_u8 = frames[1].clamp(0, 255).to(torch.uint8).contiguous()
    items = [(ref_u8, None, False), (frames[2].contiguous(), mask, True)] * 4
    tb.set_nerf_camera_matrix(np.asarray(tr._nerf_pose(tr.pose))[:3, :])
    w, h, tb.fov = tr._frame_views()[0]
    s_render, s_unet = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)

    def render():
        return {k: v.clone() for k, v in tb.render_frame_device(w, h, 8, mode=2, want_float=True).items() if v is not None}

    with torch.cuda.stream(s_render):
        alone = render()
    torch.cuda.synchronize()
    differing = 0
    for _ in range(60):
        with torch.cuda.stream(s_unet):
            model.set_batch_plan(True)
            model.forward_packed_batch(items)
            model.set_batch_plan(False)
        with torch.cuda.stream(s_render):
            got = [render() for _ in range(4)]
        torch.cuda.synchronize()
        differing += sum(1 for g in got if any(not torch.equal(g[k], alone[k]) for k in alone))
    assert differing == 0, f"{differing} of 240 renders differ from the render made alone"
