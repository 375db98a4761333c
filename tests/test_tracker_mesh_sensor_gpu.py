"""The sensor options of a mesh-template tracker: with ``reference_points="template"`` the r9 tracker takes
``occlusion`` (the pass runs on the float depth plane the template's frame call draws, scaled by that frame's own
depth_q) and ``depth_refine`` (on the template's points, which lie on the sensed surface).  With "sfm" both stay refused.

The object is test_tracker_mesh_template_gpu.py's synthetic mesh at 128 x 96, six frames; the sensor frames are uint16
counts of the mesh's own depth render at the ground-truth poses; the slab is tests/test_tracker_occlusion_gpu.py's.

Accuracy with the slab, option on against off, is PRINTED, not asserted (as DESIGN 3.13 does for the NeRF template)."""
import numpy as np
import pytest
import torch

from pixtrack_amd import depth_refinement as DR
from pixtrack_amd import mesh_render as R
from pixtrack_amd import occlusion as OC
from pixtrack_amd.geometry import Camera
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames
from test_tracker_mesh_template_gpu import TRACKER_KEYS

pytestmark = pytest.mark.gpu

W, H, N = 128, 96, 6
NAMES = [f"{i:06d}.png" for i in range(N)]
MAX_COUNT = 20000
FAR = 3 * MAX_COUNT  # the background's count: far behind the object
SLAB_FROM = 2


def mesh_object(device, seed, out_dir):
    """(assets, renderer, colour frames, float64 [N, H, W] depths of the mesh at the ground-truth poses in SfM units - 0
    where the mesh does not cover the pixel)."""
    assets = make_mesh_tracking_assets(seed=seed, width=W, height=H, n_frames=N, out_dir=out_dir, device=device)
    V, F = assets["mesh"][:2]
    renderer = R.MeshRenderer(V, F, device, **assets["mesh_shading"])
    frames = render_mesh_query_frames(assets, renderer)
    camera = Camera.from_colmap(assets["query_camera"])
    z = np.zeros((N, H, W))
    for k, (Rg, tg) in enumerate(assets["gt_poses"]):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rg, tg
        plane = renderer.render_frame([(R.view_record(camera, T), W, H, 1, ("depth",))], download_records=False)[0]["depth"]
        g = plane.cpu().numpy()  # (d, d, d, 1) on covered pixels, depth_q = 1: d is the depth itself
        z[k] = np.where(g[..., 3] > 0, g[..., 0], 0.0)
    return assets, renderer, frames, z


def counts_of(z, scale):
    """uint16 counts of a depth image; the background far behind."""
    return np.where(z > 0, np.rint(z / scale), FAR).astype(np.uint16)


def mesh_tracker(device, obj, lm_grid=0, render_ahead=False, **kw):
    assets, renderer = obj[0], obj[1]
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                             template=MeshTemplate(renderer, supersample=2, render_ahead=render_ahead), **kw)
    if lm_grid:
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = lm_grid
    return tr


def bits(T):
    return T.as12().double().numpy().reshape(-1).view(np.uint64)


def final(ret):
    return ret["T_refined"] if ret.get("success") else ret["T_init"]


def snapshot(tr):
    """The frame's occlusion pass, downloaded while its buffers still hold this frame."""
    occ = tr.last_occlusion
    if occ is None:
        return None
    torch.cuda.synchronize(tr.device)
    snap = {k: occ[k] for k in ("shift", "min_alpha", "sensor_q", "delta_q", "radii", "record", "view")}
    for k in ("depth", "mask_in", "mask", "occluder"):
        snap[k] = occ[k].cpu().numpy().copy()
    snap["sensor"] = occ["sensor"].cpu().numpy().view(np.uint16).copy()
    snap["query_mask"] = tr.localizer.refiner.query_mask.cpu().numpy().copy()
    return snap


def check_snapshot(snap, conf_delta, scale):
    """The pass's planes and counts are the restatement's on what the pass read; its quanta follow the mesh rule."""
    ref = OC.occlusion_mask_reference(snap["depth"], snap["sensor"], snap["mask_in"], snap["shift"], snap["min_alpha"],
                                      snap["sensor_q"], snap["delta_q"], *snap["radii"])
    assert np.array_equal(snap["occluder"], ref["occluder"]) and np.array_equal(snap["mask"], ref["mask"])
    assert np.array_equal(snap["query_mask"], ref["mask"])
    assert snap["record"][:8] == ref["record"][:8].tolist()
    assert snap["shift"] == (0, 0)
    depth_q = float(np.float32(snap["view"][17]))
    assert (snap["sensor_q"], snap["delta_q"]) == OC.quantize(conf_delta, scale, 1.0 / depth_q)
    return ref


@pytest.fixture(scope="module")
def scene(device, tmp_path_factory):
    """The object, the clean and the slab sequence, and the runs of the module, made once per key."""
    obj = mesh_object(device, 1031, tmp_path_factory.mktemp("mesh_sensor_object"))
    assets, _, frames, z = obj
    scale = float(z.max() / MAX_COUNT)
    clean = counts_of(z, scale)
    rng = np.random.default_rng(77)
    slab_frames, slab_sensor = [f.clone() for f in frames], clean.copy()
    for k in range(SLAB_FROM, N):  # the left third of the silhouette's bounding box, its full height and a little more
        ys, xs = np.nonzero(z[k] > 0)
        x0, x1 = int(xs.min()), int(xs.min() + (xs.max() - xs.min() + 1) // 3)
        y0, y1 = max(int(ys.min()) - 4, 0), min(int(ys.max()) + 5, H)
        texture = rng.integers(0, 256, size=(y1 - y0, x1 - x0, 3)).astype(np.float32)
        slab_frames[k][y0:y1, x0:x1] = torch.from_numpy(texture).to(device)
        slab_sensor[k, y0:y1, x0:x1] = np.uint16(np.rint(np.median(clean[k][z[k] > 0]) / 2))
    return dict(obj=obj, frames=frames, sensor=clean, slab_frames=slab_frames, slab_sensor=slab_sensor, scale=scale, runs={})


def lookup_of(scene, slab=False):
    images = scene["slab_sensor" if slab else "sensor"]
    return {n: images[k] for k, n in enumerate(NAMES)}.get


def run(device, scene, key, slab=False, render_ahead=False, **kw):
    """(tracker, per-frame occlusion snapshots) of a solo run with reference_points="template"."""
    if key not in scene["runs"]:
        tr = mesh_tracker(device, scene["obj"], render_ahead=render_ahead, reference_points="template", **kw)
        snaps = []
        for name, frame in zip(NAMES, scene["slab_frames" if slab else "frames"]):
            tr.run_single_frame((name, frame))
            snaps.append(snapshot(tr) if kw.get("occlusion") is not None else None)
        torch.cuda.synchronize(device)
        scene["runs"][key] = (tr, snaps)
    return scene["runs"][key]


def trans_errors(tr, gt):
    return [float(np.linalg.norm(np.asarray(final(tr.pose_history[n]).numpy()[1], np.float64) - tg)) for n, (_Rg, tg) in zip(NAMES, gt)]


@pytest.mark.parametrize("render_ahead", (False, True), ids=("plain", "render_ahead"))
def test_an_occluder_free_sensor_changes_no_pose(device, scene, render_ahead):
    """(a): occlusion on against off on the clean sensor - bit-identical poses, no occluder pixel, one upload per frame;
    with MeshTemplate(render_ahead=True) the frames are still used ahead."""
    off, _ = run(device, scene, ("off", render_ahead), render_ahead=render_ahead)
    opt = OC.OcclusionMask(lookup=lookup_of(scene), sensor_depth_scale=scene["scale"])
    on, snaps = run(device, scene, ("occ", render_ahead), render_ahead=render_ahead, occlusion=opt)
    assert on.sensor_uploads == N and off.sensor_uploads == 0
    assert on.localizer.refiner.point_gate is not None
    applied = 0
    for n, snap in zip(NAMES, snaps):
        ret, ref = on.pose_history[n], off.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret) and set(ret) - set(OC.HISTORY_KEYS) == set(ref)
        assert ret["n_occluder_pixels"] == 0 and ret["n_points_gated"] == 0
        assert ret["occlusion_applied"] == (snap is not None)
        if snap is not None:
            applied += 1
            check_snapshot(snap, on._occ_conf.delta, scene["scale"])
            assert snap["record"][4] == 0 and snap["record"][0] > 0 and snap["record"][1] == snap["record"][0]
            assert ret["occluded_fraction"] is not None and np.array_equal(snap["mask"], snap["mask_in"])
        else:
            assert ret["occluded_fraction"] is None
        assert ret["tracked"] == ref["tracked"] and np.array_equal(bits(final(ret)), bits(final(ref)))
    assert applied >= N - 2 and snaps[0] is None  # (the cold start gets no mask)
    assert on.render_ahead == render_ahead and on.renders_ahead_used == off.renders_ahead_used
    if render_ahead:
        assert on.renders_ahead_used > 0


def test_a_slab_leaves_the_mask_and_the_points(device, scene):
    """(b): the slab over the object's left third from frame 2 on."""
    opt = OC.OcclusionMask(lookup=lookup_of(scene, slab=True), sensor_depth_scale=scene["scale"])
    on, snaps = run(device, scene, "occ_slab", slab=True, occlusion=opt)
    off, _ = run(device, scene, "off_slab", slab=True)
    seen = 0
    for k, (n, snap) in enumerate(zip(NAMES, snaps)):
        ret = on.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret)
        if snap is None:
            assert not ret["occlusion_applied"]
            continue
        check_snapshot(snap, on._occ_conf.delta, scene["scale"])
        assert ret["n_occluder_pixels"] == snap["record"][4] and ret["n_points_gated"] == snap["record"][9] - snap["record"][10]
        if k >= SLAB_FROM and seen == 0:  # the first frame that runs a pass on a slab image
            seen += 1
            assert ret["occluded_fraction"] > 0 and ret["n_points_gated"] > 0, (n, snap["record"])
            assert ret["n_occluder_pixels"] > 0 and (snap["mask"] < snap["mask_in"]).any()
        elif k < SLAB_FROM:
            assert ret["n_occluder_pixels"] == 0
    assert seen == 1
    gt = scene["obj"][0]["gt_poses"]
    for label, tr in (("on ", on), ("off", off)):
        tra = trans_errors(tr, gt)
        print(f"slab sequence, occlusion {label}: tracked {sum(bool(tr.pose_history[n]['tracked']) for n in NAMES)}/{N}; "
              "translation error " + " ".join(f"{e:.5f}" for e in tra) + f" mean {np.mean(tra):.5f}")
    print("slab sequence, per frame (applied, occluded_fraction, n_occluder_pixels, n_points_gated):",
          [tuple(on.pose_history[n][key] for key in ("occlusion_applied", "occluded_fraction", "n_occluder_pixels",
                                                     "n_points_gated")) for n in NAMES])


def test_depth_refinement_runs_behind_the_lm(device, scene):
    """(c): depth refinement on against off, on the template's points.

    The mean translation error on <= off is asserted as tests/test_tracker_depth_refine_gpu.py asserts it for "render"
    points."""
    off, _ = run(device, scene, ("off", False))
    opt = DR.DepthRefine(lookup=lookup_of(scene), sensor_depth_scale=scene["scale"])
    on, _ = run(device, scene, "depth", depth_refine=opt)
    assert not on.render_ahead and on.renders_ahead_used == 0 and on.sensor_uploads == N
    for n in NAMES:
        ret = on.pose_history[n]
        assert set(DR.HISTORY_KEYS) <= set(ret) and set(ret) - set(DR.HISTORY_KEYS) == set(off.pose_history[n])
        if ret["depth_refined"]:
            assert ret["tracked"] and ret["depth_cost_after"] <= ret["depth_cost_before"]
            assert ret["depth_n_valid"] >= 10 and ret["depth_iters"] >= 1
        elif ret["success"]:
            assert np.array_equal(bits(ret["T_refined"]), bits(ret["T_lm"]))
    first = on.pose_history[NAMES[0]]  # the LM of the first frame ran on what the run without the option ran on
    assert np.array_equal(bits(first["T_lm"]), bits(off.pose_history[NAMES[0]]["T_refined"]))
    assert any(on.pose_history[n]["depth_refined"] for n in NAMES)
    gt = scene["obj"][0]["gt_poses"]
    e_on, e_off = trans_errors(on, gt), trans_errors(off, gt)
    print("translation error per frame, depth refinement on :", " ".join(f"{e:.5f}" for e in e_on), "mean %.5f" % np.mean(e_on))
    print("translation error per frame, depth refinement off:", " ".join(f"{e:.5f}" for e in e_off), "mean %.5f" % np.mean(e_off))
    print("depth cost before -> after:", [(on.pose_history[n]["depth_cost_before"], on.pose_history[n]["depth_cost_after"],
                                           on.pose_history[n]["depth_refined"]) for n in NAMES])
    assert np.mean(e_on) <= np.mean(e_off)


def test_both_options_share_one_upload(device, scene):
    """(d)"""
    look = lookup_of(scene, slab=True)
    both, snaps = run(device, scene, "both", slab=True, occlusion=OC.OcclusionMask(lookup=look, sensor_depth_scale=scene["scale"]),
                      depth_refine=DR.DepthRefine(lookup=look, sensor_depth_scale=scene["scale"]))
    assert both.sensor_uploads == N and not both.render_ahead
    for n, snap in zip(NAMES, snaps):
        ret = both.pose_history[n]
        assert set(OC.HISTORY_KEYS) <= set(ret) and set(DR.HISTORY_KEYS) <= set(ret)
        if snap is not None:
            check_snapshot(snap, both._occ_conf.delta, scene["scale"])
    assert any(s is not None for s in snaps)
    with pytest.raises(ValueError, match="same"):
        mesh_tracker(device, scene["obj"], reference_points="template",
                     occlusion=OC.OcclusionMask(lookup=look, sensor_depth_scale=scene["scale"]),
                     depth_refine=DR.DepthRefine(lookup=lookup_of(scene), sensor_depth_scale=scene["scale"]))


def test_the_refusals(device, scene):
    """(e): with the SfM points both options stay refused, and the message says what to pass."""
    look = lookup_of(scene)
    for points in ({}, {"reference_points": "sfm"}):
        with pytest.raises(ValueError, match="mesh template.*occlusion.*reference_points='template'"):
            mesh_tracker(device, scene["obj"], occlusion=OC.OcclusionMask(lookup=look, sensor_depth_scale=scene["scale"]), **points)
        with pytest.raises(ValueError, match="mesh template.*depth_refine.*reference_points='template'"):
            mesh_tracker(device, scene["obj"], depth_refine=DR.DepthRefine(lookup=look, sensor_depth_scale=scene["scale"]), **points)
    small = OC.OcclusionMask(lookup=lambda name: scene["sensor"][0][:-1], sensor_depth_scale=scene["scale"])
    tr = mesh_tracker(device, scene["obj"], reference_points="template", occlusion=small)
    with pytest.raises(ValueError, match="sensor depth image"):
        tr.run_single_frame((NAMES[0], scene["frames"][0]))
