"""Lock-step tracking of two mesh objects that share ONE image: MultiObjectTracker(mutual_occlusion=MutualOcclusion(...)).
The query frames are the two meshes rendered at ground truth and composited by depth on the host.  Per-image UNet plan
and the solo LM grid: the configuration whose poses are documented as bit-identical to solo runs."""
import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd import occlusion as OC
from pixtrack_amd.geometry import Camera, Pose
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.multi_object_tracker import MUTUAL_HISTORY_KEYS, MultiObjectTracker, MutualOcclusion
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets
from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations
from test_multi_object_gpu import _poses
from test_tracker_mesh_template_gpu import TRACKER_KEYS

pytestmark = pytest.mark.gpu

W, H, N_FRAMES, GRID, R_GROW = 160, 96, 5, 32, 2
NAMES = [f"{i:06d}.png" for i in range(N_FRAMES)]
# camera-frame shifts of the two objects' ground-truth translations.  Alone, an object fills the image's height at the
# centre.  Overlapping: the first stays in front, the second stands 1.3 behind it, its left third behind the first.
# Disjoint: both 1.5 further away, one to either side - no pixel shows both.
OVERLAPPING = ((-0.20, 0.0, 0.0), (0.75, 0.0, 1.3))
DISJOINT = ((-1.0, 0.0, 1.5), (1.0, 0.0, 1.5))


@pytest.fixture(scope="module")
def objects(device, tmp_path_factory):
    """Two mesh objects (320 triangles each: the numpy rasteriser draws them per frame below) and their renderers."""
    objs = []
    for k in range(2):
        assets = make_mesh_tracking_assets(seed=1041 + k, width=W, height=H, n_frames=N_FRAMES, subdivisions=2,
                                           out_dir=tmp_path_factory.mktemp(f"scene_object{k}"), device=device)
        V, F = assets["mesh"][:2]
        objs.append((assets, R.MeshRenderer(V, F, device, **assets["mesh_shading"])))
    return dict(objs=objs, runs={})


def shifted_poses(assets, shift):
    out = []
    for Rg, tg in assets["gt_poses"]:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rg, tg + np.asarray(shift, np.float64)
        out.append(T)
    return out


def composite_frames(objs, poses, noise_sigma=2.0, seed=5):
    """Per frame: each object at its pose, 4 x 4 samples per pixel, premultiplied over black; where both are seen, the
    one whose S = 1 depth is smaller goes on top.  float32 HWC 0..255 device tensors."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    frames = []
    for i in range(N_FRAMES):
        rgba, z = [], []
        for (assets, renderer), T in zip(objs, poses):
            cam = Camera.from_colmap(assets["query_camera"])
            out = renderer.render_frame([(R.view_record(cam, T[i]), W, H, 4, ("rgba",)), (R.view_record(cam, T[i]), W, H, 1, ("depth",))],
                                        download_records=False)
            rgba.append(out[0]["rgba"])
            z.append(torch.where(out[1]["depth"][..., 3] > 0, out[1]["depth"][..., 0], torch.full_like(out[1]["depth"][..., 0], 1e30)))
        first_on_top = (z[0] <= z[1])[..., None]
        top = torch.where(first_on_top, rgba[0], rgba[1])
        below = torch.where(first_on_top, rgba[1], rgba[0])
        img = (top[..., :3] + (1.0 - top[..., 3:]) * below[..., :3]) * 255.0
        img = (img + (torch.randn(img.shape, generator=g) * noise_sigma).to(img.device)).clamp_(0, 255).round_()
        frames.append(img.contiguous())
    return frames


def tracker(device, obj, start):
    assets, renderer = obj
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                             template=MeshTemplate(renderer, supersample=2))
    for opt in tr.localizer.optimizer:
        opt.conf.n_workgroups = GRID
    tr.pose = Pose.from_Rt(start[:3, :3], start[:3, 3])  # the cold start refines from here (the object is not centred)
    return tr


def snapshot(tr):
    """The frame's mutual-occlusion pass, downloaded while its buffers still hold this frame."""
    frame = tr.last_mutual_occlusion
    if frame is None:
        return None
    torch.cuda.synchronize(tr.device)
    snap = {k: frame[k].cpu().numpy().copy() for k in ("occluder", "mask")}
    snap["is_query_mask"] = tr.localizer.refiner.query_mask is frame["mask"]
    snap["record"], snap["scene_record"] = frame["record"], frame["scene_record"]
    snap["gates"] = [dict(p3d=g["p3d"].cpu().numpy().copy(), valid_in=None if g["valid_in"] is None else
                          g["valid_in"].cpu().numpy().copy(), valid=g["valid"].cpu().numpy().copy(), T_init=g["T_init"],
                          camera=g["camera"]) for g in frame["gates"]]
    return snap


def run(device, objects, shifts, option, solo_step=None):
    """One lock-step run over the composite sequence -> (trackers, per step: the start poses and the snapshots).
    ``solo_step``: on that step the second tracker is sent through run_single_frame (a cold start from its pose)."""
    key = (shifts, None if option is None else (tuple(option.scenes), option.r_grow), solo_step)
    if key not in objects["runs"]:
        objs = objects["objs"]
        poses = [shifted_poses(assets, s) for (assets, _), s in zip(objs, shifts)]
        frames = objects["runs"].setdefault(("frames", shifts), composite_frames(objs, poses))
        trackers = [tracker(device, obj, p[0]) for obj, p in zip(objs, poses)]
        multi = MultiObjectTracker(trackers, lm_workgroups=GRID, per_image_plan=True, n_groups=1, mutual_occlusion=option)
        steps = []
        for i in range(N_FRAMES):
            if i == solo_step:
                trackers[1].cold_start = True
            starts = [tr.pose for tr in trackers]
            multi.run_single_frames([(NAMES[i], frames[i])] * 2)
            steps.append((starts, [snapshot(tr) if option is not None else None for tr in trackers]))
        torch.cuda.synchronize(device)
        objects["runs"][key] = (trackers, steps, poses, multi)
    return objects["runs"][key]


def report(label, trackers, poses):
    for j, tr in enumerate(trackers):
        errs = []
        for i, n in enumerate(NAMES):
            ret = tr.pose_history[n]
            Rt, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
            errs.append((geodesic_distance_for_rotations(Rt, poses[j][i][:3, :3]), float(np.linalg.norm(t - poses[j][i][:3, 3]))))
        print(f"{label}, object {j}: tracked {sum(bool(tr.pose_history[n]['tracked']) for n in NAMES)}/{N_FRAMES}; rotation error "
              "(rad) " + " ".join(f"{e[0]:.4f}" for e in errs) + "; translation error " + " ".join(f"{e[1]:.4f}" for e in errs))


def test_without_the_option_nothing_is_added(device, objects):
    trackers, _, poses, multi = run(device, objects, OVERLAPPING, None)
    report("overlapping, option off", trackers, poses)
    assert multi.mutual_occlusion is None and multi.lockstep_frames >= 2
    for tr in trackers:
        assert tr.mutual_occlusion is False and tr.localizer.refiner.point_gate is None and tr.last_mutual_occlusion is None
        assert all(not set(MUTUAL_HISTORY_KEYS) & set(tr.pose_history[n]) for n in NAMES)


def test_disjoint_objects_track_bit_identically_with_and_without_the_option(device, objects):
    off, _, poses, _ = run(device, objects, DISJOINT, None)
    on, steps, _, multi = run(device, objects, DISJOINT, MutualOcclusion(scenes=["table", "table"], r_grow=R_GROW))
    report("disjoint, option on", on, poses)
    applied = 0
    for a, b in zip(on, off):
        assert np.array_equal(_poses(a, NAMES).view(np.uint64), _poses(b, NAMES).view(np.uint64))
        for n in NAMES:
            ret = a.pose_history[n]
            assert set(MUTUAL_HISTORY_KEYS) <= set(ret) and set(ret) - set(MUTUAL_HISTORY_KEYS) == set(b.pose_history[n])
            assert ret["n_mutually_hidden_pixels"] == 0 and ret["n_mutual_occluder_pixels"] == 0 and ret["n_points_gated_mutual"] == 0
            applied += bool(ret["mutual_occlusion_applied"])
    assert applied >= 4 and multi.lockstep_frames >= 4  # the scene was drawn: two objects on at least two steps
    assert not on[0].pose_history[NAMES[0]]["mutual_occlusion_applied"]  # the cold starts ran alone


def test_overlapping_objects(device, objects):
    objs = objects["objs"]
    off, _, poses, _ = run(device, objects, OVERLAPPING, None)
    on, steps, _, multi = run(device, objects, OVERLAPPING, MutualOcclusion(scenes=[0, 0], r_grow=R_GROW))
    report("overlapping, option on", on, poses)
    checked = 0
    for i, (starts, snaps) in enumerate(steps):
        rets = [tr.pose_history[NAMES[i]] for tr in on]
        assert rets[0]["mutual_occlusion_applied"] == rets[1]["mutual_occlusion_applied"] == (snaps[0] is not None) == (snaps[1] is not None)
        if snaps[0] is None:
            for ret in rets:
                assert (ret["n_mutually_hidden_pixels"], ret["n_mutual_occluder_pixels"], ret["n_points_gated_mutual"],
                        ret["mutually_hidden_fraction"]) == (0, 0, 0, None)
            continue
        checked += 1
        items = [(assets["mesh"][0], assets["mesh"][1], assets["mesh_shading"],
                  tr.template.requests(start, tr.camera, tr._reference_camera())[:1])
                 for (assets, _), tr, start in zip(objs, on, starts)]
        want = R.scene_reference(items, [[0], [0]], R_GROW)
        for ret, snap, w in zip(rets, snaps, want):
            rec = w[0]["records"]
            assert np.array_equal(snap["occluder"], w[0]["occluder"])
            assert ret["n_mutually_hidden_pixels"] == int(rec[R.W_HIDDEN]) == snap["scene_record"][10]
            assert ret["n_mutual_occluder_pixels"] == int(rec[R.W_OCCLUDER]) == int(snap["occluder"].sum())
            assert ret["mutually_hidden_fraction"] == int(rec[R.W_HIDDEN]) / int(rec[R.W_COVERED])
            # the mask holds no pixel of G, and it is the mask the query went through the UNet with
            assert not (snap["mask"] & snap["occluder"]).any() and snap["is_query_mask"] and snap["mask"].any()
            assert snap["record"][1] == int(snap["mask"].sum()) <= snap["record"][0]
            # the gate: pxt_points_visible on G at the start pose
            assert len(snap["gates"]) == 1
            g = snap["gates"][0]
            pts = OC.points_visible_reference(g["p3d"], g["valid_in"], g["T_init"], g["camera"], w[0]["occluder"])
            keep = ~pts["fragile"]  # (a point within 1e-3 px of a texel boundary may round either way)
            assert pts["fragile"].sum() <= 0.02 * len(keep) and np.array_equal(g["valid"][keep], pts["valid"][keep])
            assert snap["record"][8:11] == [len(keep), pts["counts"][1], int(g["valid"].sum())]
            assert ret["n_points_gated_mutual"] == pts["counts"][1] - int(g["valid"].sum())
            assert abs(ret["n_points_gated_mutual"] - (pts["counts"][1] - pts["counts"][2])) <= int(pts["fragile"].sum())
        # the front object has nothing hidden; the one behind it has
        assert rets[0]["n_mutually_hidden_pixels"] == 0 and rets[0]["n_mutual_occluder_pixels"] == 0 and rets[0]["n_points_gated_mutual"] == 0
        assert rets[1]["n_mutually_hidden_pixels"] > 50 and rets[1]["n_mutual_occluder_pixels"] > rets[1]["n_mutually_hidden_pixels"]
        assert (snaps[1]["record"][1] < snaps[1]["record"][0]) and rets[1]["n_points_gated_mutual"] > 0
    assert checked >= 2 and steps[0][1] == [None, None]  # the cold starts ran alone: no scene on step 0
    # ... so the front object's poses are those of the run without the option, bit for bit
    assert np.array_equal(_poses(on[0], NAMES).view(np.uint64), _poses(off[0], NAMES).view(np.uint64))
    report("overlapping, option off (again)", off, poses)


def test_a_member_that_runs_alone_leaves_the_scene_for_that_step(device, objects):
    solo_step = N_FRAMES - 1
    on, steps, _, multi = run(device, objects, OVERLAPPING, MutualOcclusion(scenes=[0, 0], r_grow=R_GROW), solo_step=solo_step)
    assert multi.solo_frames == 3  # the two cold starts and the second tracker's last frame
    for tr in on:
        assert tr.pose_history[NAMES[solo_step]]["mutual_occlusion_applied"] is False
        assert tr.pose_history[NAMES[solo_step]]["n_mutually_hidden_pixels"] == 0
    assert steps[solo_step][1] == [None, None]
    assert on[1].pose_history[NAMES[solo_step - 1]]["mutual_occlusion_applied"] is True


def test_what_the_constructor_refuses(device, objects):
    objs = objects["objs"]
    start = shifted_poses(objs[0][0], (0, 0, 0))[0]
    trackers = [tracker(device, obj, start) for obj in objs] + [tracker(device, objs[0], start)]
    cam = Camera.from_colmap(objs[0][0]["query_camera"])
    option = MutualOcclusion(scenes=[0, 0, None])
    # the cameras a scene's trackers already have are checked
    trackers[0].camera, trackers[1].camera = cam, cam.scale(0.5)
    with pytest.raises(ValueError, match="different query cameras"):
        MultiObjectTracker(trackers, mutual_occlusion=option)
    trackers[1].camera = cam
    # a NeRF-template tracker in a scene
    template, trackers[1].template = trackers[1].template, None
    with pytest.raises(ValueError, match="no mesh template"):
        MultiObjectTracker(trackers, mutual_occlusion=option)
    trackers[1].template = template
    assert all(tr.mutual_occlusion is False and tr.localizer.refiner.point_gate is None for tr in trackers)  # nothing was touched
    # groups: a scene stays together (tracker 1 follows tracker 0), or the placement is refused
    multi = MultiObjectTracker(trackers, n_groups=2, mutual_occlusion=MutualOcclusion(scenes=[None, 0, 0]))
    assert [g.members for g in multi.groups] == [[0], [1, 2]]
    assert [tr.mutual_occlusion for tr in trackers] == [False, True, True]
    multi.groups[0].members, multi.groups[1].members = [0, 1], [2]
    with pytest.raises(ValueError, match="different groups"):
        multi._check_scene_groups()
    # the sensor option still refuses a mesh template
    with pytest.raises(ValueError, match="mesh template is not combined with occlusion"):
        PixLocPoseTrackerR9._check_template(template, None, "sfm", None, object())
