"""The opt-in ``reference_points="render"`` of the r9 tracker: a frame is refined on points back-projected from its own
Depth render (pxt_points_from_depth, tests/test_points_from_depth_gpu.py) instead of the SfM points of the nearest
mapping image.  Off (the default) nothing changes."""
import numpy as np
import pytest
import torch

from pixtrack_amd.geometry import Camera, Pose
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames, sfm_to_ngp_points

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 6
NAMES = [f"{i:06d}.png" for i in range(N)]
_SHARED = {}


def _assets():
    if "assets" not in _SHARED:
        _SHARED["assets"] = make_tracking_assets(width=W, height=H, n_frames=N)
    return _SHARED["assets"]


def _tracker(device, **kw):
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=_assets(), **kw)


def _frames(tr):
    if "frames" not in _SHARED:
        _SHARED["frames"] = render_query_frames(_assets(), tr.testbed)
    return _SHARED["frames"]


def _run(device, key, n=N, force=None, **kw):
    """The history of a run over the first ``n`` frames (computed once per key); ``force`` = (frame index, reference ids
    set before that frame)."""
    if key not in _SHARED:
        tr = _tracker(device, **kw)
        frames = _frames(tr)
        for i in range(n):
            if force is not None and force[0] == i:
                tr.reference_ids = list(force[1])
            tr.run_single_frame((NAMES[i], frames[i]))
        torch.cuda.synchronize()
        _SHARED[key] = tr.pose_history
    return _SHARED[key]


def _pose_bits(ret):
    T = ret["T_refined"] if ret.get("success") else ret["T_init"]
    return T.as12().double().numpy().reshape(-1).view(np.uint64)


def _errors(history):
    """(max rotation error [rad], max translation error) of the refined poses against the synthetic ground truth."""
    rot, trans = [], []
    for name, (Rg, tg) in zip(NAMES, _assets()["gt_poses"]):
        ret = history[name]
        R, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
        R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
        rot.append(float(np.arccos(np.clip((np.trace(Rg.T @ R) - 1.0) / 2.0, -1.0, 1.0))))
        trans.append(float(np.linalg.norm(t - tg)))
    return max(rot), max(trans)


def _render_at_gt(device, k=0):
    """A "render" tracker with the frame's renders made at ground-truth pose k: (tracker, pose, depth, view, ref_u8)."""
    tr = _tracker(device, reference_points="render")
    tr.camera = Camera.from_colmap(_assets()["query_camera"])
    Rg, tg = _assets()["gt_poses"][k]
    pose = Pose.from_Rt(Rg, tg)
    _, ref_u8 = tr._mask_and_reference(pose, from_slot=False)
    depth = tr._own.depth
    return tr, pose, depth, tr._depth_view(pose), ref_u8


def _select(depth, n_max, erode, min_alpha):
    """The pixels the points come from, in slot order (float64 / integer restatement of the kernel's selection)."""
    Hh, Ww, _ = depth.shape
    base = (depth[..., 3] >= np.float32(min_alpha)) & (depth[..., 0] > 0)
    acc = np.zeros_like(base)
    e = erode
    inner = np.ones((Hh - 2 * e, Ww - 2 * e), bool)
    for dy in range(-e, e + 1):
        for dx in range(-e, e + 1):
            inner &= base[e + dy:Hh - e + dy, e + dx:Ww - e + dx]
    acc[e:Hh - e, e:Ww - e] = inner
    A = int(acc.sum())
    s = 1
    while s * s * n_max < A:
        s += 1
    ys, xs = np.nonzero(acc)
    keep = (xs % s == s // 2) & (ys % s == s // 2)
    return xs[keep][:n_max], ys[keep][:n_max], [A, s, min(int(keep.sum()), n_max), int(keep.sum())]


def test_points_land_on_their_pixels(device):
    tr, pose, depth, view, _ = _render_at_gt(device)
    refiner = tr.localizer.refiner
    conf = refiner.conf
    p3d, slot_valid, rec = refiner.points_from_render(depth, view)
    torch.cuda.synchronize()
    xs, ys, want_rec = _select(depth.cpu().numpy(), int(conf.reference_points_max), int(conf.reference_points_erode),
                               float(conf.reference_points_min_alpha))
    assert rec.tolist() == want_rec and want_rec[2] >= 100
    n = want_rec[2]
    assert slot_valid.cpu().numpy().tolist() == [1] * n + [0] * (int(conf.reference_points_max) - n)
    pts = p3d.cpu().double().numpy()[:n]
    # the sampler's camera model (pxt_common.h project_point) in float64, with the query camera at the render's pose
    R, t = pose.numpy()
    pc = pts @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    c10 = [float(v) for v in tr.camera.as10().tolist()]
    fx, fy, cx, cy, k1, k2 = c10[2:8]
    xn, yn = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    r2 = xn * xn + yn * yn
    rad = k1 * r2 + k2 * r2 * r2
    u, v = fx * (xn + xn * rad) + cx, fy * (yn + yn * rad) + cy
    err = max(float(np.abs(u - xs).max()), float(np.abs(v - ys).max()))
    print("max reprojection error [px]:", err)
    assert (pc[:, 2] > 0).all() and err <= 1e-2
    # inside the render box (ngp coordinates)
    p_ngp = sfm_to_ngp_points(pts)
    lo, hi = np.asarray(tr.testbed.render_aabb.min), np.asarray(tr.testbed.render_aabb.max)
    assert (p_ngp >= lo - 1e-5).all() and (p_ngp <= hi + 1e-5).all()
    # the two-camera path (Depth and Shade as a pair of renders) hands over the same Depth image
    tr.fuse_identical_views = False
    tr._coincide_cache = None
    assert len(tr._frame_views()) == 2
    tr._mask_and_reference(pose, from_slot=False)
    assert tr._own.pose is pose and torch.equal(tr._own.depth.view(torch.int32), depth.view(torch.int32))


def test_extract_reference_features_from_render(device):
    tr, pose, depth, view, ref_u8 = _render_at_gt(device, 1)
    refiner = tr.localizer.refiner
    refiner.feature_extractor.unstage()
    dbids = tr.reference_ids
    feats = refiner.extract_reference_features(dbids, pose, ref_u8, depth=depth, depth_view=view)["1"]
    torch.cuda.synchronize()
    n_max = int(refiner.conf.reference_points_max)
    rec = feats.points_record.tolist()
    n_points = rec[2]
    assert 100 <= n_points <= n_max
    assert int(feats.slot_valid.sum()) == n_points and int(feats.slot_valid[:n_points].sum()) == n_points
    valid = feats.valid.cpu().numpy()
    assert not valid[n_points:].any() and valid[:n_points].sum() >= n_points // 2
    assert feats.p3dids_all == list(range(n_max)) and tuple(feats.p3d.shape) == (n_max, 3)
    # the packed features are those of the sampler given the same points, on the whole render (no window)
    maps, scales = refiner.dense_feature_extraction(ref_u8, "ref", 1)
    want = refiner.interp_sparse_observations(maps, scales, dbids[0], feats.p3dids_all, pose, feats.p3d)
    torch.cuda.synchronize()
    assert torch.equal(want.valid, feats.valid)
    keep = feats.valid.bool()
    for a, b in zip(want.packed, feats.packed):
        assert torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32))
    with pytest.raises(ValueError):
        refiner.extract_reference_features(dbids, pose, ref_u8)  # the option needs the Depth render
    with pytest.raises(ValueError):
        refiner.points_from_render(depth, {**view, "k1": 0.01})  # no lens undistortion in the kernel


def test_pose_does_not_depend_on_the_mapping_image(device):
    """One steady frame (index 2) with the reference id forced to two mapping images that share camera 1."""
    cams = {_assets()["model3d"].dbs[i].camera_id for i in (1, 2)}
    assert cams == {1}
    out = {}
    for mode in ("render", "sfm"):
        for ref in (1, 2):
            h = _run(device, (mode, "forced", ref), n=3, force=(2, [ref]), reference_points=mode)
            assert h[NAMES[2]]["success"]
            out[mode, ref] = _pose_bits(h[NAMES[2]])
    assert np.array_equal(out["render", 1], out["render", 2])
    assert not np.array_equal(out["sfm", 1], out["sfm", 2])


def test_six_frame_sequence(device):
    sfm = _run(device, "sfm", reference_points="sfm")
    ren = _run(device, "render", reference_points="render")
    (r_sfm, t_sfm), (r_ren, t_ren) = _errors(sfm), _errors(ren)
    print(f"max rotation error [rad]: sfm {r_sfm:.6f} render {r_ren:.6f}; max translation error: sfm {t_sfm:.6f} "
          f"render {t_ren:.6f}; points per frame {[ren[n]['n_reference_points'] for n in NAMES]}, "
          f"stride {[ren[n]['reference_point_stride'] for n in NAMES]}")
    assert all(ren[n]["tracked"] for n in NAMES)
    assert all(0 < ren[n]["n_reference_points"] <= 2048 and ren[n]["reference_point_stride"] >= 1 for n in NAMES)
    assert r_ren <= 2.0 * r_sfm and t_ren <= 2.0 * t_sfm


def test_option_off_is_the_default(device):
    default = _run(device, "default")
    sfm = _run(device, "sfm", reference_points="sfm")
    for n in NAMES:
        assert np.array_equal(_pose_bits(default[n]), _pose_bits(sfm[n]))
        assert set(default[n]) == set(sfm[n]) and "n_reference_points" not in default[n]
        assert default[n]["tracked"] == sfm[n]["tracked"] and default[n]["cost"] == sfm[n]["cost"]


def test_refused_combinations(device):
    kw = dict(debug=0, device=device, assets=_assets())
    with pytest.raises(ValueError):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="render", relocalizer="views", **kw)
    with pytest.raises(ValueError):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="render", uncertainty=True, **kw)
    with pytest.raises(ValueError):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="points", **kw)
    with pytest.raises(ValueError):
        PixLocPoseTrackerYCB("", "", "/tmp", "", reference_points="render", **kw)
    with pytest.raises(ValueError):
        MultiObjectTracker([_tracker(device, reference_points="render")])
