"""The relocaliser on the device: pxt_score_pose_hypotheses against a float64 CPU restatement and against the LM's own
first logged cost, its determinism, and relocalisation / lost-track recovery on the synthetic assets.  The restatement
runs on the SIMPLE_RADIAL bank and, with the same hypothesis recipe, on an OPENCV bank and on a bank whose camera has its
range limit inside the image (tests/camera_cases.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import camera_cases as CC
from oracle import lm_oracle as O
from pixtrack_amd import _lib
from pixtrack_amd.geometry import Pose
from pixtrack_amd.ops import ops
from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for, parse_loss_fn
from pixtrack_amd.synthetic import make_lm_scene, perturb_pose, rodrigues

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 2e-2, 0.05  # synthetic vs ground truth, as tests/test_bench_gpu.py applies them
LEVEL = 2                        # stride 16, C = 128


# ------------------------------------------------------------------------------------------------ kernel inputs
def _pack(scene, level, device):
    fq = scene.feats_query[level]
    Cc = fq.shape[0] - 1
    cs = cstride_for(Cc)
    h, w = fq.shape[1:]
    fmap = torch.zeros(h, w, cs)
    fmap[..., :Cc] = O.l2_normalize(fq[:-1], dim=0).permute(1, 2, 0)
    fmap[..., Cc] = fq[-1]
    fr = scene.feats_ref[level]
    fref = torch.zeros(fr.shape[0], cs)
    fref[:, :Cc] = O.l2_normalize(fr[:, :-1], dim=1)
    fref[:, Cc] = fr[:, -1]
    return fmap, fref, Cc, scene.camera.scale(scene.scales[level])


def _make_bank(device, **scene_kw):
    sc = make_lm_scene(seed=1201, width=320, height=240, n_points=1500, sigma_px=2.0, **scene_kw)
    fmap, fref, Cc, cam = _pack(sc, LEVEL, device)
    rng = np.random.default_rng(12)
    n = sc.p3d.shape[0]
    valid = (rng.uniform(size=n) > 0.15).astype(np.uint8)
    # ~300 hypotheses: ranges of odd lengths (not multiples of 64) at random offsets, poses from the ground truth perturbed
    # by 0..20 degrees / 0..10 cm; a few look away from the object (no valid point) and a few have empty ranges
    poses, ranges = [], []
    for h in range(300):
        count = int(rng.choice([1, 7, 63, 65, 129, 333, 700, 1499]))
        begin = int(rng.integers(0, n - count + 1))
        if h % 50 == 7:
            count = 0
        R, t = perturb_pose(sc.R_gt, sc.t_gt, rng, float(rng.uniform(0, 20)), float(rng.uniform(0, 0.1)), sc.center)
        if h % 37 == 5:
            t = t + np.array([0.0, 0.0, -50.0])  # every point behind the camera
        poses.append(np.concatenate([R.reshape(-1), t]))
        ranges.append((begin, count))
    return dict(scene=sc, fmap=fmap, fref=fref, C=Cc, cam=cam, p3d=sc.p3d, valid=valid,
                poses=np.asarray(poses, np.float64), ranges=np.asarray(ranges, np.int32))


@pytest.fixture(scope="module")
def scene_bank(device):
    return _make_bank(device, k1=-0.08)


@pytest.fixture(scope="module", params=["opencv", "k1_limit"])
def table_bank(request, device):
    """The same hypothesis recipe on a camera of tests/camera_cases.py: ndist 4, and a range limit inside the image."""
    return request.param, _make_bank(device, **CC.SCENE_KW[request.param])


def _launch(sb, device, loss=(2, 0.0, 0.1), pad=1, poses=None, ranges=None, out=None, fmap=None):
    poses = sb["poses"] if poses is None else poses
    ranges = sb["ranges"] if ranges is None else ranges
    M = poses.shape[0]
    t = sb.setdefault("_dev", {})
    if "fmap" not in t:
        t["fmap"] = sb["fmap"].to(device).contiguous()
        t["p3d"] = torch.from_numpy(sb["p3d"]).float().to(device).contiguous()
        t["fref"] = sb["fref"].to(device).contiguous()
        t["valid"] = torch.from_numpy(sb["valid"]).to(device)
    cam = sb["cam"]
    out = torch.full((M, 4), -7.0, device=device) if out is None else out
    ops.score_pose_hypotheses(t["fmap"] if fmap is None else fmap, sb["C"], [float(x) for x in cam.as10().tolist()],
                              int(cam._data.shape[-1] - 6), t["p3d"], t["fref"], t["valid"],
                              torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(device),
                              torch.from_numpy(np.ascontiguousarray(ranges, np.int32)).to(device), pad, *loss, out)
    return out


def _restatement(sb, loss_kind, alpha, scale, pad=1):
    """float64: the oracle's world2image / interpolator / make_loss over each hypothesis's valid points.  Returns the four
    sums per hypothesis and, per hypothesis, how many points lie within 1e-3 px of the padded image border or within
    relative 1e-5 (in r^2) of the distortion model's range limit (where float32 and float64 may decide validity
    differently)."""
    name = {0: "squared", 1: "huber", 2: "barron"}[loss_kind]
    loss = O.make_loss(name) if loss_kind == 0 else O.make_loss(name, alpha, scale)
    fmap = sb["fmap"].double()
    C_ = sb["C"]
    chw = fmap[..., :C_ + 1].permute(2, 0, 1).contiguous()
    h, w = chw.shape[1:]
    cam = sb["cam"]._data.double()
    if cam.shape[-1] < 10:
        cam = torch.cat([cam, torch.zeros(10 - cam.shape[-1], dtype=torch.float64)])
    fref = sb["fref"].double()
    p3d = torch.from_numpy(sb["p3d"])
    valid = torch.from_numpy(sb["valid"]).bool()
    outs, edge = [], []
    for pose, (b, n) in zip(sb["poses"], sb["ranges"]):
        if n == 0:
            outs.append([0.0, 0.0, 0.0, 0.0])
            edge.append(0)
            continue
        R = torch.from_numpy(pose[:9].reshape(3, 3))
        t = torch.from_numpy(pose[9:])
        pc = p3d[b:b + n] @ R.T + t
        p2d, vis = O.world2image(cam, pc)
        F, inimg, _ = O.interpolator(chw, p2d, pad)
        ok = vis & inimg & valid[b:b + n]
        lim = torch.tensor([w - pad - 1, h - pad - 1], dtype=torch.float64)
        margin = torch.minimum((p2d - pad).abs().min(-1).values, (lim - p2d).abs().min(-1).values)
        near_limit = torch.from_numpy(CC.r2_margin(cam[6:], pc.numpy()) <= CC.R2_REL_MARGIN)
        edge.append(int((valid[b:b + n] & ((vis & (margin < 1e-3)) | near_limit)).sum()))
        r = F[:, :C_] - fref[b:b + n, :C_]
        rho = loss(((r * r).sum(-1)))[0]
        wgt = F[:, C_] * fref[b:b + n, C_]
        rho, wgt = rho[ok], wgt[ok]
        outs.append([float(rho.sum()), float(ok.sum()), float((wgt * rho).sum()), float(wgt.sum())])
    return np.asarray(outs), np.asarray(edge)


# ------------------------------------------------------------------------------------------------ 1. CPU restatement
@pytest.mark.parametrize("loss", [(0, 2.0, 1.0), (1, 0.0, 0.1), (2, 0.0, 0.1)], ids=["squared", "huber", "barron"])
def test_kernel_matches_float64_restatement(device, scene_bank, loss):
    got = _launch(scene_bank, device, loss).cpu().double().numpy()
    want, edge = _restatement(scene_bank, *loss)
    assert (want[:, 1] == 0).sum() >= 10 and (want[:, 1] > 100).sum() >= 50  # the cases are there
    exact = edge == 0
    assert exact.mean() > 0.95, edge
    np.testing.assert_array_equal(got[exact, 1], want[exact, 1])
    assert np.all(np.abs(got[~exact, 1] - want[~exact, 1]) <= edge[~exact])
    for k in (0, 2, 3):
        # (atol: float32 cancellation in r = F_q - F_ref for near-identical descriptors; seen up to 2e-8 on sums of few points)
        np.testing.assert_allclose(got[exact, k], want[exact, k], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("loss", [(0, 2.0, 1.0), (1, 0.0, 0.1), (2, 0.0, 0.1)], ids=["squared", "huber", "barron"])
def test_kernel_matches_float64_restatement_on_the_camera_table(device, table_bank, loss):
    name, bank = table_bank
    got = _launch(bank, device, loss).cpu().double().numpy()
    want, edge = _restatement(bank, *loss)
    assert (want[:, 1] == 0).sum() >= 10 and (want[:, 1] > 100).sum() >= 50  # the cases are there
    exact = edge == 0
    print(f"{name}: {int((~exact).sum())} of {len(edge)} hypotheses hold a point the two precisions may decide differently")
    assert exact.mean() > 0.95, edge
    np.testing.assert_array_equal(got[exact, 1], want[exact, 1])
    assert np.all(np.abs(got[~exact, 1] - want[~exact, 1]) <= edge[~exact])
    for k in (0, 2, 3):
        np.testing.assert_allclose(got[exact, k], want[exact, k], rtol=1e-5, atol=1e-7)
    if name in CC.LIMIT_CASES:
        # hypotheses near the ground truth see points inside the image and beyond the range: they must not count
        sc, cam = bank["scene"], bank["cam"]._data.double()
        pc = torch.from_numpy(sc.p3d @ sc.R_gt.T + sc.t_gt)
        p2d, vis = O.world2image(cam, pc)
        in_img = torch.all((p2d >= 0) & (p2d <= cam[:2] - 1), -1)
        assert int((in_img & ~vis).sum()) >= 10


# ------------------------------------------------------------------------------------------------ 2. the LM's cost
def test_masked_mean_equals_the_lm_first_logged_cost(device, scene_bank):
    sb = scene_bank
    opt = PixTrackOptimizer(dict(num_iters=1, pad=1))
    conf = opt.native_conf()
    kind, alpha, scale = parse_loss_fn(opt.conf.loss_fn)
    sel = [h for h in range(len(sb["ranges"])) if sb["ranges"][h][1] >= 300][:8]
    assert len(sel) == 8
    out = _launch(sb, device, (kind, alpha, scale), pad=conf.pad).cpu().numpy()
    dev = sb["_dev"]
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
    lam = torch.full((6,), 1e-3)
    checked = 0
    for h in sel:
        b, n = (int(x) for x in sb["ranges"][h])
        pack = LevelPack(dev["fmap"], dev["fref"][b:b + n].contiguous(), sb["C"], sb["cam"], lam)
        res = PixTrackOptimizer.refine_levels(dev["p3d"][b:b + n].contiguous(), [pack],
                                              Pose(torch.from_numpy(sb["poses"][h]).float()), conf, ws,
                                              mask=dev["valid"][b:b + n].contiguous()).result()
        k0, k1 = float(res.log[0, 0, 0]), float(res.log[0, 0, 1])
        assert out[h, 1] == k1, (h, out[h], k0, k1)
        if k1 >= conf.min_valid:
            assert out[h, 0] / out[h, 1] == pytest.approx(k0, rel=1e-6), (h, out[h], k0)
            checked += 1
    assert checked >= 6


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_bit_identical_across_launches_orders_and_streams(device, scene_bank):
    sb = scene_bank
    a = _launch(sb, device).cpu()
    b = _launch(sb, device).cpu()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    perm = np.random.default_rng(3).permutation(len(sb["ranges"]))
    c = _launch(sb, device, poses=sb["poses"][perm], ranges=sb["ranges"][perm]).cpu()
    assert torch.equal(c.view(torch.int32), a[perm].view(torch.int32))
    one = _launch(sb, device, poses=sb["poses"][5:6], ranges=sb["ranges"][5:6]).cpu()
    assert torch.equal(one.view(torch.int32), a[5:6].view(torch.int32))
    # ... and beside another stream's UNet passes
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    net = UNet(make_synthetic_unet_weights(7), device)
    img = torch.rand(240, 320, 3, device=device) * 255
    side = torch.cuda.Stream(device=device)
    outs = [torch.empty(len(sb["ranges"]), 4, device=device) for _ in range(100)]
    main = torch.cuda.current_stream(device)
    side.wait_stream(main)
    for o in outs:
        with torch.cuda.stream(side):
            net.forward_packed(img, None, True)
        _launch(sb, device, out=o)
    torch.cuda.synchronize(device)
    bad = [i for i, o in enumerate(outs) if not torch.equal(o.cpu().view(torch.int32), a.view(torch.int32))]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_invalid_arguments_raise(device, scene_bank):
    sb = scene_bank
    _launch(sb, device)
    dev = sb["_dev"]
    with pytest.raises(_lib.PxtError):  # M = 0
        _launch(sb, device, poses=np.zeros((0, 12)), ranges=np.zeros((0, 2), np.int32), out=torch.empty(0, 4, device=device))
    with pytest.raises(_lib.PxtError):  # a host-memory point mask beside device tensors: refused before the launch
        ops.score_pose_hypotheses(dev["fmap"], sb["C"], [float(x) for x in sb["cam"].as10().tolist()],
                                  int(sb["cam"]._data.shape[-1] - 6), dev["p3d"], dev["fref"], dev["valid"].cpu(),
                                  torch.zeros(2, 12, device=device), torch.zeros(2, 2, dtype=torch.int32, device=device),
                                  1, 2, 0.0, 0.1, torch.zeros(2, 4, device=device))
    with pytest.raises(_lib.PxtError):  # fref / map cstride mismatch
        _launch(sb, device, fmap=torch.zeros(15, 20, 136, device=device))
    L = _lib.lib()
    mp = _lib.RelocMap()
    mp.fmap, mp.h, mp.w, mp.C, mp.cstride = dev["fmap"].data_ptr(), 15, 20, 128, 132
    mp.ndist = 2
    bank = _lib.RelocBank()
    bank.p3d, bank.fref, bank.valid, bank.n_points = dev["p3d"].data_ptr(), dev["fref"].data_ptr(), None, dev["p3d"].shape[0]
    conf = _lib.LmConf()
    conf.pad, conf.loss, conf.loss_scale = 1, 2, 0.1
    poses = torch.zeros(4, 12, device=device)
    ranges = torch.zeros(4, 2, dtype=torch.int32, device=device)
    out = torch.zeros(4, 4, device=device)
    s = _lib.stream_ptr(device)

    def call(m=mp, b=bank, M=4):
        return L.pxt_score_pose_hypotheses(C.byref(m), b if b is None else C.byref(b), poses.data_ptr(), ranges.data_ptr(), M,
                                           C.byref(conf), out.data_ptr(), s)

    assert call() == 0
    assert call(M=0) == -1
    assert call(M=-3) == -1
    assert call(b=None) == -1
    mp.cstride = 130
    assert call() == -1
    mp.cstride, mp.C = 132, 130
    assert call() == -1
    mp.C = 128
    bank.p3d = None
    assert call() == -1
    torch.cuda.synchronize(device)


# ------------------------------------------------------------------------------------------------ 4./5. relocalisation
@pytest.fixture(scope="module")
def reloc_tracker(device):
    """640 x 480, the assets bench.py tracks (seed 1002: its own trajectory tracks frame after frame)."""
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets

    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=20)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets, relocalizer="views")
    tr.spp = 2
    return assets, tr


def _frames(assets, tr, poses, seed=5, cold=()):
    from pixtrack_amd.synthetic import render_query_frames

    a = dict(assets)
    a["gt_poses"] = poses
    return render_query_frames(a, tr.testbed, seed=seed, cold_start_indices=cold)


def _err(pose, R, t):
    from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

    Rp, tp = pose.numpy()
    return geodesic_distance_for_rotations(Rp, R), float(np.linalg.norm(np.asarray(tp) - t))


def _rolled(R, t, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return Rz @ R, Rz @ t


def _about_axis(assets, pose, deg):
    """The pose after the object turned by ``deg`` about its long axis (the orbit's axis) through its centre."""
    R, t = pose
    c = assets["center"]
    dR = rodrigues(np.array([0.0, 0.0, 1.0]) * math.radians(deg))
    return R @ dR, R @ (c - dR @ c) + t


def _reset_cold(tr, relocalizer):
    tr.relocalizer = relocalizer
    tr.pose, tr.cold_start, tr.success, tr._lost, tr._accepted_pose = None, True, True, False, None
    tr.cost_threshold, tr.dynamic_id, tr.cache_hit = None, None, False
    tr.reference_ids = tr._initial_reference_ids({"upright_ref_img": "mapping/0001.png"})


def _far_poses(assets, dbs, seed=21):
    """Ground truths near mapping views 5, 9 and 13 (90 degrees or more from the upright view 1), rolled in-plane by 40 and
    130 degrees, then perturbed by up to 5 degrees / 1 cm."""
    rng = np.random.default_rng(seed)
    gts = []
    for v in (5, 9, 13):
        for roll in (40.0, 130.0):
            R, t = _rolled(dbs[v].qvec2rotmat(), dbs[v].tvec, roll)
            gts.append(perturb_pose(R, t, rng, float(rng.uniform(0, 5)), float(rng.uniform(0, 0.01)), assets["center"]))
    return gts


def test_localize_far_from_the_upright_view(reloc_tracker):
    assets, tr = reloc_tracker
    gts = _far_poses(assets, tr.localizer.model3d.dbs)
    frames = _frames(assets, tr, gts)
    reloc = tr.relocalizer
    for k, ((R, t), fr) in enumerate(zip(gts, frames)):
        tr.camera = tr.get_query_camera(fr)
        res = reloc.localize(fr, tr.camera)
        assert res.pose is not None and res.n_hypotheses == reloc.n_views * reloc.rolls == len(reloc.views)
        rot, tra = _err(res.pose, R, t)
        assert rot < ROT_TOL and tra < TRANS_TOL, (k, rot, tra, res.view_id, [c["cost"] for c in res.candidates])
    # the default cold start (upright pose, then refine at scales [4, 1]) on the same frames does not get there
    for k, ((R, t), fr) in enumerate(zip(gts, frames)):
        _reset_cold(tr, None)
        tr.run_single_frame((f"{k:06d}.png", fr))
        rot, _ = _err(tr.pose, R, t)
        assert rot > 0.3, (k, rot)
    _reset_cold(tr, reloc)


def _track(tr, frames, names_from=0):
    for i, fr in enumerate(frames):
        tr.run_single_frame((f"{names_from + i:06d}.png", fr))
        yield tr.pose_history[f"{names_from + i:06d}.png"], tr.pose


def test_lost_track_recovery(reloc_tracker):
    """Ten frames of the assets' orbit, then the object turns by 120 degrees (a cut), then ten more."""
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    assets, tr = reloc_tracker
    gt = assets["gt_poses"]
    gts = gt[:10] + [_about_axis(assets, p, 120.0) for p in gt[10:20]]
    frames = _frames(assets, tr, gts, seed=8, cold=(0,))  # the cold-start frame is the noisier one, as in every synthetic run
    results = {}
    for mode in ("off", "views"):  # a fresh tracker each, as a user would start one
        t2 = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=tr.device, assets=assets, relocalizer=mode)
        t2.spp = tr.spp
        rows = []
        for i, (ret, pose) in enumerate(_track(t2, frames)):
            rows.append(_row(ret, pose, gts[i]))
        results[mode] = (rows, t2.relocalization_count, t2.cost_threshold)
    off, _, thr_off = results["off"]
    on, n_reloc, thr_on = results["views"]
    assert all(r["tracked"] and r["close"] for r in off[:10]), (off, thr_off)
    assert not any(r["tracked"] and r["close"] for r in off[10:]), (off, thr_off)  # today: the track is lost for good
    # With the relocaliser, every frame from the second after the cut is on the object: its refinement converges within the
    # synthetic-vs-ground-truth bounds.  Whether the tracker ACCEPTS it is the reference's frozen gate (cost <= 1.1 x the
    # cold-start frame's cost, kept as is): a relocalised cold start fits frame 0 better than the upright start does, so
    # its gate is tighter than the cost of a masked steady frame (measured: threshold 0.0059 against steady costs
    # 0.0062-0.0070 on this sequence; the default tracker's own cold start left it enough room).  A frame the gate rejects
    # is relocalised on the next one; the gate is the only reason a frame goes untracked (on this sequence it rejects
    # every frame after the cut: the issue's "tracked" is unreachable under the frozen gate).
    for r in on[:1] + on[11:]:
        assert r["refined_close"] and (r["tracked"] or r["cost"] > thr_on), (on, thr_on)
    assert any(r["relocalised"] for r in on[11:]), (on, thr_on)
    assert n_reloc >= 2, n_reloc


def _row(ret, pose, gt):
    """What a frame did: tracked (refiner AND gate), its pose against the ground truth, and its refined pose (before the gate)."""
    rot, tra = _err(pose, *gt)
    refined = ret.get("T_refined")
    rrot, rtra = _err(refined, *gt) if refined is not None else (float("inf"), float("inf"))
    return {"tracked": bool(ret["tracked"]), "close": rot < ROT_TOL and tra < TRANS_TOL, "rot": round(rot, 4),
            "refined_close": bool(ret["success"]) and rrot < ROT_TOL and rtra < TRANS_TOL, "cost": float(ret["cost"]),
            "relocalised": bool(ret.get("relocalized", False))}


def test_start_segment_without_a_pose_relocalises(reloc_tracker):
    assets, tr = reloc_tracker
    dbs = tr.localizer.model3d.dbs
    start = _rolled(dbs[9].qvec2rotmat(), dbs[9].tvec, 70.0)
    gts = [_about_axis(assets, start, 0.5 * i) for i in range(3)]
    frames = _frames(assets, tr, gts, seed=11, cold=(0,))
    tr.start_segment(None)
    n0 = tr.relocalization_count
    rows = [_row(ret, pose, gts[i]) for i, (ret, pose) in enumerate(_track(tr, frames, names_from=300))]
    assert rows[0]["relocalised"] and rows[0]["tracked"] and rows[0]["close"], rows
    # later frames: on the object; untracked only where the frozen gate rejects them (test_lost_track_recovery)
    assert all(r["refined_close"] and (r["tracked"] or r["cost"] > tr.cost_threshold) for r in rows), (rows, tr.cost_threshold)
    assert tr.relocalization_count >= n0 + 1
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    with pytest.raises(ValueError):
        PixLocPoseTrackerR9.start_segment(type("T", (), {"relocalizer": None})(), None)


def test_cli_relocalize_on_disk_assets(reloc_tracker, tmp_path, monkeypatch):
    """The command line on an object directory in the reference's layout whose first frame is far from the upright view:
    --relocalize views tracks it, --relocalize off (the default) does not."""
    import pickle

    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as cli
    from pixtrack_amd.synthetic import write_object_dir

    assets, tr = reloc_tracker
    dbs = tr.localizer.model3d.dbs
    start = _rolled(dbs[13].qvec2rotmat(), dbs[13].tvec, 130.0)
    gts = [_about_axis(assets, start, 0.5 * i) for i in range(3)]
    frames = _frames(assets, tr, gts, seed=12, cold=(0,))
    obj, query = tmp_path / "obj", tmp_path / "query"
    write_object_dir(assets, obj, query, frames)
    monkeypatch.setenv("UPRIGHT_REF_IMG", assets["upright_ref_img"])
    monkeypatch.setenv("OBJ_AABB", str([list(map(float, assets["aabb"][0])), list(map(float, assets["aabb"][1]))]))
    monkeypatch.delenv("PIXTRACK_WEIGHTS", raising=False)
    init = cli.PixLocPoseTrackerR9.__init__

    def small_spp(self, *a, **k):
        init(self, *a, **k)
        self.spp = 2

    monkeypatch.setattr(cli.PixLocPoseTrackerR9, "__init__", small_spp)
    errs = {}
    for mode in ("views", "off"):
        out = tmp_path / mode
        cli.main(["--object_path", str(obj), "--query", str(query), "--out_dir", str(out), "--relocalize", mode])
        with open(out / "poses.pkl", "rb") as f:
            poses = pickle.load(f)
        keys = sorted(poses, key=str)
        assert len(keys) == 3
        pose_of = lambda r: r["T_refined"] if "T_refined" in r else r["T_init"]  # (a failed frame has no refined pose)
        errs[mode] = [(bool(poses[k]["tracked"]),) + _err(pose_of(poses[k]), *gts[i]) for i, k in enumerate(keys)]
    assert all(ok and rot < ROT_TOL and tra < TRANS_TOL for ok, rot, tra in errs["views"]), errs
    assert all(rot > 0.3 for _, rot, _ in errs["off"]), errs
