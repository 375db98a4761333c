"""The opt-in ``depth_refine`` of the r9 tracker (pixtrack_amd/depth_refinement.py): one pxt_depth_refine problem queued
behind a frame's last LM launch, the pose taken from it by _frame_policy.  Off (the default) nothing changes.

The "sensor" frames are made of Depth renders at the ground-truth poses: camera-axis depth in SfM units, quantised to
uint16 counts, a far background behind the object.  The renders put the principal point at the image centre and use one
focal length; the sensor image is shifted onto the query camera's pixels as sensor_evaluation.sensor_alignment says.
The accuracy statement is made with reference_points="render" (points on the composited depth surface); the synthetic
SfM points sit on an iso-level of the density, beside that surface - with them the run only has to complete.
"""
import numpy as np
import pytest
import torch

from pixtrack_amd import depth_refinement as DR
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
_SHARED = {}


def _assets():
    if "assets" not in _SHARED:
        _SHARED["assets"] = make_tracking_assets(width=W, height=H, n_frames=N)
    return _SHARED["assets"]


def _tracker(device, **kw):
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=_assets(), **kw)


def _sensor(device):
    """(uint16 [N, H, W] sensor images on the query camera's pixels, SfM units per count)."""
    if "sensor" not in _SHARED:
        tr = _tracker(device)
        _SHARED["frames"] = render_query_frames(_assets(), tr.testbed)
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
        _SHARED["sensor"] = (SE.shifted_sensor(counts, (-sx, -sy)), scale)
    return _SHARED["sensor"]


def _option(device, zero=False, **kw):
    images, scale = _sensor(device)
    table = {n: (np.zeros_like(images[k]) if zero else images[k]) for k, n in enumerate(NAMES)}
    return DR.DepthRefine(lookup=table.get, sensor_depth_scale=scale, **kw)


def _run(device, key, **kw):
    if key not in _SHARED:
        _sensor(device)
        tr = _tracker(device, **kw)
        for name, frame in zip(NAMES, _SHARED["frames"]):
            tr.run_single_frame((name, frame))
        torch.cuda.synchronize(device)
        _SHARED[key] = tr
    return _SHARED[key]


def _bits(T):
    return T.as12().double().numpy().reshape(-1).view(np.uint64)


def _trans_errors(history):
    out = []
    for name, (Rg, tg) in zip(NAMES, _assets()["gt_poses"]):
        ret = history[name]
        _, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
        out.append(float(np.linalg.norm(np.asarray(t, np.float64) - tg)))
    return out


def test_option_off_adds_nothing(device):
    off = _run(device, "off", reference_points="render")
    for n in NAMES:
        assert not set(DR.HISTORY_KEYS) & set(off.pose_history[n])
    assert off.depth_refine is None and off.localizer.refiner.depth_hook is None


def test_option_on_refines_behind_the_lm(device):
    off = _run(device, "off", reference_points="render")
    on = _run(device, "on", reference_points="render", depth_refine=_option(device))
    assert on.renders_ahead_used == 0 and not on.render_ahead
    for n in NAMES:
        ret = on.pose_history[n]
        assert set(DR.HISTORY_KEYS) <= set(ret) and set(ret) - set(DR.HISTORY_KEYS) == set(off.pose_history[n])
        if ret["depth_refined"]:
            assert ret["tracked"] and ret["depth_cost_after"] <= ret["depth_cost_before"]
            assert ret["depth_n_valid"] >= 10 and ret["depth_iters"] >= 1
            assert not np.array_equal(_bits(ret["T_refined"]), _bits(ret["T_lm"]))
        elif ret["success"]:
            assert np.array_equal(_bits(ret["T_refined"]), _bits(ret["T_lm"]))
    # the LM of the first frame ran on what the run without the option ran on
    first = on.pose_history[NAMES[0]]
    assert np.array_equal(_bits(first["T_lm"]), _bits(off.pose_history[NAMES[0]]["T_refined"]))
    assert any(on.pose_history[n]["depth_refined"] for n in NAMES)
    e_on, e_off = _trans_errors(on.pose_history), _trans_errors(off.pose_history)
    print("translation error per frame, option on :", " ".join(f"{e:.5f}" for e in e_on), "mean %.5f" % np.mean(e_on))
    print("translation error per frame, option off:", " ".join(f"{e:.5f}" for e in e_off), "mean %.5f" % np.mean(e_off))
    print("depth cost before -> after:", [(on.pose_history[n]["depth_cost_before"], on.pose_history[n]["depth_cost_after"],
                                           on.pose_history[n]["depth_refined"]) for n in NAMES])
    assert np.mean(e_on) <= np.mean(e_off)


def test_frames_without_a_measurement_keep_the_lm_pose(device):
    zero = _run(device, "zero", reference_points="render", depth_refine=_option(device, zero=True))
    off = _run(device, "off", reference_points="render")
    for n in NAMES:
        ret = zero.pose_history[n]
        assert ret["depth_refined"] is False and ret["tracked"] == off.pose_history[n]["tracked"]
        if ret["success"]:
            assert np.array_equal(_bits(ret["T_refined"]), _bits(ret["T_lm"]))
        # (render-ahead aside, the run is the run without the option)
        assert np.array_equal(_bits(ret["T_refined"] if ret["success"] else ret["T_init"]),
                              _bits(off.pose_history[n]["T_refined"] if off.pose_history[n]["success"]
                                    else off.pose_history[n]["T_init"]))


def test_sfm_points_complete(device):
    on = _run(device, "on_sfm", depth_refine=_option(device, prior=(0.0, 50.0)))
    off = _run(device, "off_sfm")
    e_on, e_off = _trans_errors(on.pose_history), _trans_errors(off.pose_history)
    print("SfM points: mean translation error on %.5f off %.5f; refined frames %d of %d" % (
        np.mean(e_on), np.mean(e_off), sum(bool(on.pose_history[n]["depth_refined"]) for n in NAMES), N))
    assert all(set(DR.HISTORY_KEYS) <= set(on.pose_history[n]) for n in NAMES)


def test_refused_uses(device):
    kw = dict(debug=0, device=device, assets=_assets())
    opt = _option(device)
    with pytest.raises(ValueError):
        PixLocPoseTrackerR9("", "", "", "/tmp", depth_refine=opt, relocalizer="views", **kw)
    with pytest.raises(ValueError):
        PixLocPoseTrackerYCB("", "", "/tmp", "", depth_refine=opt, **kw)
    with pytest.raises(ValueError):
        MultiObjectTracker([_tracker(device, depth_refine=opt)])
    # a sensor image of another size than the query
    images, scale = _sensor(device)
    small = DR.DepthRefine(lookup=lambda name: images[0][:-1], sensor_depth_scale=scale)
    tr = _tracker(device, depth_refine=small)
    with pytest.raises(ValueError):
        tr.run_single_frame((NAMES[0], _SHARED["frames"][0]))
