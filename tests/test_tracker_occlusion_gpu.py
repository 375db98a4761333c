"""The opt-in ``occlusion`` of the r9 tracker (pixtrack_amd/occlusion.py): on a frame that gets a mask, the pixels where
the frame's sensor depth image lies in front of the mask view's Depth render leave the query mask (pxt_occlusion_mask),
and the reference points that project onto them leave the LM's point mask (pxt_points_visible).  Off (the default)
nothing changes.

The set-up is tests/test_tracker_depth_refine_gpu.py's: 160 x 120, six frames, "sensor" frames made of Depth renders at
the ground-truth poses.  The occluder is a noise-textured slab painted over the object's left third in the colour
frames from frame 2 on, the sensor counts there set to half the object's depth.

Accuracy and tracked counts, option on against off on the slab sequence, are PRINTED, not asserted: nobody has measured
whether masking helps on this synthetic scene (DESIGN 3.13 holds the figures of one run)."""
import numpy as np
import pytest
import torch

from pixtrack_amd import depth_refinement as DR
from pixtrack_amd import occlusion as OC
from pixtrack_amd import render_evaluation as RE
from pixtrack_amd import sensor_evaluation as SE
from pixtrack_amd.geometry import Camera
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 6
NAMES = [f"{i:06d}.png" for i in range(N)]
MAX_COUNT = 20000
MIN_ALPHA = 0.5
SLAB_FROM = 2
_SHARED = {}


def _assets():
    if "assets" not in _SHARED:
        _SHARED["assets"] = make_tracking_assets(width=W, height=H, n_frames=N)
    return _SHARED["assets"]


def _tracker(device, **kw):
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=_assets(), **kw)


def _scene(device):
    """The clean and the slab sequence: colour frames, uint16 [N, H, W] sensor images on the query camera's pixels, SfM
    units per count."""
    if "scene" not in _SHARED:
        tr = _tracker(device)
        frames = render_query_frames(_assets(), tr.testbed)
        camera = Camera.from_colmap(_assets()["query_camera"])
        out = torch.empty(N, H, W, 4, dtype=torch.float32, device=device)
        for k, (Rg, tg) in enumerate(_assets()["gt_poses"]):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rg, tg
            RE._render_depth(tr.testbed, tr.nerf2sfm, T, camera, 8, out[k])
        torch.cuda.synchronize(device)
        g = out.cpu().numpy()
        on = (g[..., 3] >= MIN_ALPHA) & (g[..., 0] > 0)
        with np.errstate(all="ignore"):
            z = np.where(on, g[..., 0] / np.where(on, g[..., 3], 1) * RE.z_scale(tr.testbed, tr.nerf2sfm), 0.0)
        scale = float(z.max() / MAX_COUNT)
        counts = np.where(on, np.rint(z / scale), 3 * MAX_COUNT).astype(np.uint16)  # the object before a far background
        sx, sy, residual = SE.sensor_alignment(camera)
        print(f"sensor alignment: shift ({sx}, {sy}), residual {residual:.3f} px; SfM units per count {scale:.3e}")
        clean = SE.shifted_sensor(counts, (-sx, -sy))
        sil = SE.shifted_sensor(on.astype(np.uint16), (-sx, -sy)) != 0
        # the slab: the left third of the silhouette's bounding box, its full height and a little more
        rng = np.random.default_rng(77)
        slab_frames, slab_sensor = [f.clone() for f in frames], clean.copy()
        for k in range(SLAB_FROM, N):
            ys, xs = np.nonzero(sil[k])
            x0, x1 = int(xs.min()), int(xs.min() + (xs.max() - xs.min() + 1) // 3)
            y0, y1 = max(int(ys.min()) - 4, 0), min(int(ys.max()) + 5, H)
            texture = rng.integers(0, 256, size=(y1 - y0, x1 - x0, 3)).astype(np.float32)
            slab_frames[k][y0:y1, x0:x1] = torch.from_numpy(texture).to(device)
            half = np.rint(np.median(clean[k][sil[k]]) / 2)
            slab_sensor[k, y0:y1, x0:x1] = np.uint16(half)
        _SHARED["scene"] = dict(frames=frames, sensor=clean, slab_frames=slab_frames, slab_sensor=slab_sensor, scale=scale)
    return _SHARED["scene"]


def _option(device, slab=False, **kw):
    sc = _scene(device)
    images = sc["slab_sensor" if slab else "sensor"]
    table = {n: images[k] for k, n in enumerate(NAMES)}
    return OC.OcclusionMask(lookup=table.get, sensor_depth_scale=sc["scale"], **kw)


def _snapshot(tr):
    """The frame's occlusion pass, downloaded while its buffers still hold this frame."""
    occ = tr.last_occlusion
    if occ is None:
        return None
    torch.cuda.synchronize(tr.device)
    snap = {k: occ[k] for k in ("shift", "min_alpha", "sensor_q", "delta_q", "radii", "record")}
    for k in ("depth", "mask_in", "mask", "occluder"):
        snap[k] = occ[k].cpu().numpy().copy()
    snap["sensor"] = occ["sensor"].cpu().numpy().view(np.uint16).copy()
    snap["query_mask"] = tr.localizer.refiner.query_mask.cpu().numpy().copy()
    snap["gates"] = [dict(p3d=g["p3d"].cpu().numpy().copy(), valid_in=None if g["valid_in"] is None else
                          g["valid_in"].cpu().numpy().copy(), valid=g["valid"].cpu().numpy().copy(), T_init=g["T_init"],
                          camera=g["camera"]) for g in occ["gates"]]
    return snap


def _run(device, key, slab=False, **kw):
    if key not in _SHARED:
        sc = _scene(device)
        tr = _tracker(device, **kw)
        snaps = []
        for name, frame in zip(NAMES, sc["slab_frames" if slab else "frames"]):
            tr.run_single_frame((name, frame))
            snaps.append(_snapshot(tr) if kw.get("occlusion") is not None else None)
        torch.cuda.synchronize(device)
        _SHARED[key] = (tr, snaps)
    return _SHARED[key]


def _bits(T):
    return T.as12().double().numpy().reshape(-1).view(np.uint64)


def _final(ret):
    return ret["T_refined"] if ret.get("success") else ret["T_init"]


def _errors(history):
    """(rotation error in degrees, translation error) per frame against ground truth."""
    rot, tr = [], []
    for name, (Rg, tg) in zip(NAMES, _assets()["gt_poses"]):
        R, t = _final(history[name]).numpy()
        c = (np.trace(np.asarray(R, np.float64).T @ Rg) - 1.0) / 2.0
        rot.append(float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))))
        tr.append(float(np.linalg.norm(np.asarray(t, np.float64) - tg)))
    return rot, tr


def test_option_off_adds_nothing(device):
    off, _ = _run(device, "off")
    for n in NAMES:
        assert not set(OC.HISTORY_KEYS) & set(off.pose_history[n])
    assert off.occlusion is None and off.localizer.refiner.point_gate is None and off.last_occlusion is None
    assert off.sensor_uploads == 0


def test_an_occluder_free_sensor_changes_no_pose(device):
    off, _ = _run(device, "off")
    on, snaps = _run(device, "on", occlusion=_option(device))
    assert on.render_ahead and on.renders_ahead_used > 0
    assert on.localizer.refiner.point_gate is not None and on.sensor_uploads == N
    applied = 0
    for n, snap in zip(NAMES, snaps):
        ret, ref = on.pose_history[n], off.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret) and set(ret) - set(OC.HISTORY_KEYS) == set(ref)
        assert ret["n_occluder_pixels"] == 0 and ret["n_points_gated"] == 0
        assert ret["occlusion_applied"] == (snap is not None)
        if snap is not None:
            applied += 1
            assert snap["record"][4] == 0 and snap["record"][0] > 0 and snap["record"][1] > 0
            assert ret["occluded_fraction"] is not None and np.array_equal(snap["mask"], snap["mask_in"])
        else:
            assert ret["occluded_fraction"] is None
        assert ret["tracked"] == ref["tracked"] and np.array_equal(_bits(_final(ret)), _bits(_final(ref)))
    assert applied >= 1 and snaps[0] is None  # (the cold start gets no mask)
    assert on.renders_ahead_used == off.renders_ahead_used


def test_a_slab_leaves_the_mask_and_the_points(device):
    on, snaps = _run(device, "on_slab", slab=True, occlusion=_option(device, slab=True))
    seen = 0
    for k, (n, snap) in enumerate(zip(NAMES, snaps)):
        ret = on.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret)
        if snap is None:
            assert not ret["occlusion_applied"]
            continue
        ref = OC.occlusion_mask_reference(snap["depth"], snap["sensor"], snap["mask_in"], snap["shift"], snap["min_alpha"],
                                          snap["sensor_q"], snap["delta_q"], *snap["radii"])
        assert np.array_equal(snap["occluder"], ref["occluder"]) and np.array_equal(snap["mask"], ref["mask"])
        assert np.array_equal(snap["query_mask"], ref["mask"])
        assert snap["record"][:8] == ref["record"][:8].tolist()
        assert len(snap["gates"]) == 1
        g = snap["gates"][0]
        pts = OC.points_visible_reference(g["p3d"], g["valid_in"], g["T_init"], g["camera"], ref["occluder"])
        keep = ~pts["fragile"]
        assert pts["fragile"].sum() <= 0.02 * len(keep)
        assert np.array_equal(g["valid"][keep], pts["valid"][keep])
        assert snap["record"][8:11] == [len(keep), pts["counts"][1], int(g["valid"].sum())]
        assert ret["n_points_gated"] == snap["record"][9] - snap["record"][10]
        assert ret["n_occluder_pixels"] == snap["record"][4]
        assert ret["occluded_fraction"] == snap["record"][2] / snap["record"][0]
        if k >= SLAB_FROM:
            seen += 1
            assert ret["n_occluder_pixels"] > 0 and ret["n_points_gated"] > 0, (n, snap["record"])
            assert (snap["mask"] < snap["mask_in"]).any()
        else:
            assert ret["n_occluder_pixels"] == 0
    assert seen >= 1


def test_accuracy_on_the_slab_sequence_is_reported(device):
    """Printed, not asserted (module docstring): only that both runs complete and the keys are there."""
    on, _ = _run(device, "on_slab", slab=True, occlusion=_option(device, slab=True))
    off, _ = _run(device, "off_slab", slab=True)
    for label, tr in (("on ", on), ("off", off)):
        rot, tra = _errors(tr.pose_history)
        tracked = sum(bool(tr.pose_history[n]["tracked"]) for n in NAMES)
        print(f"slab sequence, option {label}: tracked {tracked}/{N}; rotation error (deg) " +
              " ".join(f"{e:.3f}" for e in rot) + f" mean {np.mean(rot):.3f}; translation error " +
              " ".join(f"{e:.5f}" for e in tra) + f" mean {np.mean(tra):.5f}; renders ahead used {tr.renders_ahead_used}")
    print("slab sequence, option on: per frame (applied, occluded_fraction, n_occluder_pixels, n_points_gated):",
          [(on.pose_history[n]["occlusion_applied"], on.pose_history[n]["occluded_fraction"],
            on.pose_history[n]["n_occluder_pixels"], on.pose_history[n]["n_points_gated"]) for n in NAMES])
    assert all(set(OC.HISTORY_KEYS) <= set(on.pose_history[n]) for n in NAMES)
    assert all(not set(OC.HISTORY_KEYS) & set(off.pose_history[n]) for n in NAMES)


def test_refused_uses(device):
    kw = dict(debug=0, device=device, assets=_assets())
    opt = _option(device)
    with pytest.raises(ValueError):
        PixLocPoseTrackerR9("", "", "", "/tmp", occlusion=opt, relocalizer="views", **kw)
    with pytest.raises(ValueError):
        PixLocPoseTrackerYCB("", "", "/tmp", "", occlusion=opt, **kw)
    with pytest.raises(ValueError):
        MultiObjectTracker([_tracker(device, occlusion=opt)])
    sc = _scene(device)
    # two options, two lookups (or two scales): one upload cannot serve both
    other = DR.DepthRefine(lookup=lambda name: None, sensor_depth_scale=sc["scale"])
    with pytest.raises(ValueError):
        _tracker(device, occlusion=opt, depth_refine=other)
    with pytest.raises(ValueError):
        _tracker(device, occlusion=opt, depth_refine=DR.DepthRefine(lookup=opt.lookup, sensor_depth_scale=2 * sc["scale"]))
    # a sensor image of another size than the query
    small = OC.OcclusionMask(lookup=lambda name: sc["sensor"][0][:-1], sensor_depth_scale=sc["scale"])
    tr = _tracker(device, occlusion=small)
    with pytest.raises(ValueError):
        tr.run_single_frame((NAMES[0], sc["frames"][0]))


def test_together_with_depth_refine_one_upload_serves_both(device):
    opt = _option(device, slab=True)
    both, snaps = _run(device, "both", slab=True, occlusion=opt,
                       depth_refine=DR.DepthRefine(lookup=opt.lookup, sensor_depth_scale=opt.sensor_depth_scale))
    assert both.sensor_uploads == N
    for n in NAMES:
        ret = both.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret) and set(DR.HISTORY_KEYS) <= set(ret)
    assert any(s is not None for s in snaps)
