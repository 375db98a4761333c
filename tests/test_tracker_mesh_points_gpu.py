"""reference_points="template": a mesh-template tracker refined on a lattice of its own frame's depth plane
(pxt_points_from_depth_views, tests/test_mesh_points_gpu.py) instead of the SfM points of the nearest mapping image -
the solo r9 tracker on the synthetic mesh object of test_tracker_mesh_template_gpu.py, and lock-step tracking of three
mesh objects with ONE points call per step and group (test_multi_object_mesh_gpu.py's set-up and bars).  Off (the
default, and "sfm") nothing changes."""
import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd import refiner as refiner_module
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers import multi_object_tracker as multi_module
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, make_tracking_assets, render_mesh_query_frames, render_query_frames
from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations
from test_multi_object_gpu import _poses
from test_tracker_mesh_template_gpu import TRACKER_KEYS

pytestmark = pytest.mark.gpu

K, W, H, N_FRAMES = 3, 128, 96, 6
NAMES = [f"{i:06d}.png" for i in range(N_FRAMES)]


@pytest.fixture(scope="module")
def objects(device, tmp_path_factory):
    """Three mesh objects - the first is test_tracker_mesh_template_gpu.py's - as (assets, renderer, query frames), and
    the solo runs per (object, points, LM grid), made once."""
    objs = []
    for k in range(K):
        assets = make_mesh_tracking_assets(seed=1031 + k, width=W, height=H, n_frames=N_FRAMES,
                                           out_dir=tmp_path_factory.mktemp(f"mesh_points_object{k}"), device=device)
        V, F = assets["mesh"][:2]
        renderer = R.MeshRenderer(V, F, device, **assets["mesh_shading"])
        objs.append((assets, renderer, render_mesh_query_frames(assets, renderer)))
    return dict(objs=objs, solo={})


def mesh_tracker(device, obj, lm_grid=0, **kw):
    assets, renderer, _ = obj
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                             template=MeshTemplate(renderer, supersample=2), **kw)
    if lm_grid:
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = lm_grid
    return tr


def solo(device, objects, j, points, lm_grid=0, force=None):
    """(tracker, _poses) of object j's solo run; ``points`` None: no argument.  ``force`` = (frame, reference ids)."""
    key = (j, points, lm_grid, None if force is None else (force[0], tuple(force[1])))
    if key not in objects["solo"]:
        tr = mesh_tracker(device, objects["objs"][j], lm_grid, **({} if points is None else {"reference_points": points}))
        for i in range(N_FRAMES if force is None else force[0] + 1):
            if force is not None and force[0] == i:
                tr.reference_ids = list(force[1])
            tr.run_single_frame((NAMES[i], objects["objs"][j][2][i]))
        torch.cuda.synchronize()
        objects["solo"][key] = (tr, _poses(tr, NAMES[:len(tr.pose_history)]))
    return objects["solo"][key]


def errors(tr, gt):
    rot, trans = [], []
    for i, name in enumerate(NAMES):
        Rt, t = tr.pose_history[name]["T_refined"].numpy()
        rot.append(geodesic_distance_for_rotations(Rt, gt[i][0]))
        trans.append(float(np.linalg.norm(t - gt[i][1])))
    return max(rot), max(trans)


# ----------------------------------------------------------------------------------------------------------------------
# solo
# ----------------------------------------------------------------------------------------------------------------------
def test_solo_tracking_follows_ground_truth(device, objects):
    gt = objects["objs"][0][0]["gt_poses"]
    tr, _ = solo(device, objects, 0, "template")
    sfm, _ = solo(device, objects, 0, "sfm")
    (r_t, t_t), (r_s, t_s) = errors(tr, gt), errors(sfm, gt)
    points = [tr.pose_history[n]["n_reference_points"] for n in NAMES]
    strides = [tr.pose_history[n]["reference_point_stride"] for n in NAMES]
    print(f"max rotation error [rad]: template {r_t:.6f} sfm {r_s:.6f}; max translation error: template {t_t:.6f} sfm "
          f"{t_s:.6f}; points per frame {points}, stride {strides}")
    for n in NAMES:
        ret = tr.pose_history[n]
        assert ret["tracked"] and ret["success"] and ret["template"] == "mesh"
        assert 0 < ret["n_reference_points"] <= 2048 and ret["reference_point_stride"] >= 1
    assert r_t < 2e-2 and t_t < 2e-2
    assert tr.misses == N_FRAMES - 1 and tr.relocalization_count == 1 and tr.template_frames_batched == 0


def test_pose_does_not_depend_on_the_mapping_image(device, objects):
    """One steady frame (index 2) with the reference id forced to two mapping images that share camera 1."""
    dbs = objects["objs"][0][0]["model3d"].dbs
    assert {dbs[i].camera_id for i in (1, 2)} == {1}
    bits = []
    for ref in (1, 2):
        tr, poses = solo(device, objects, 0, "template", force=(2, [ref]))
        assert tr.pose_history[NAMES[2]]["success"]
        bits.append(poses[2].view(np.uint64))
    assert np.array_equal(bits[0], bits[1])


def test_the_features_are_the_samplers_on_the_whole_reference_image(device, objects):
    from pixtrack_amd.geometry import Camera, Pose

    assets = objects["objs"][0][0]
    tr = mesh_tracker(device, objects["objs"][0], reference_points="template")
    tr.camera = Camera.from_colmap(assets["query_camera"])
    pose = Pose.from_Rt(*assets["gt_poses"][1])
    _, ref_u8 = tr._mask_and_reference(pose, from_slot=False)
    held, depth, view20 = tr._own.pose, tr._own.depth, tr._own.view
    assert held is pose and tuple(depth.shape) == (H, W, 4) and view20.shape == (20,)
    # the record is the one the plane was drawn with: the template's own request for this pose
    assert np.array_equal(view20, tr.template.requests(pose, tr.camera, tr._reference_camera(), want_depth=True)[0][0])
    refiner = tr.localizer.refiner
    refiner.feature_extractor.unstage()
    dbids = tr.reference_ids
    feats = refiner.extract_reference_features(dbids, pose, ref_u8, depth=depth, depth_view=view20)["1"]
    torch.cuda.synchronize()
    n_max = int(refiner.conf.reference_points_max)
    want_p, want_v, want_r = R.points_reference(depth.cpu().numpy(), view20, float(refiner.conf.reference_points_min_alpha),
                                                int(refiner.conf.reference_points_erode), n_max)
    n_points = int(want_r[2])
    assert feats.points_record.tolist() == want_r.tolist() and 100 <= n_points <= n_max
    assert np.array_equal(feats.p3d.cpu().numpy().view(np.int32), want_p.view(np.int32))
    assert np.array_equal(feats.slot_valid.cpu().numpy(), want_v)
    valid = feats.valid.cpu().numpy()
    assert not valid[n_points:].any() and valid[:n_points].sum() >= n_points // 2
    assert feats.p3dids_all == list(range(n_max))
    # the packed features are those of the sampler given the same points, on the whole image (no window)
    maps, scales = refiner.dense_feature_extraction(ref_u8, "ref", 1)
    want = refiner.interp_sparse_observations(maps, scales, dbids[0], feats.p3dids_all, pose, feats.p3d)
    torch.cuda.synchronize()
    assert torch.equal(want.valid, feats.valid)
    keep = feats.valid.bool()
    for a, b in zip(want.packed, feats.packed):
        assert torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32))
    # points extracted elsewhere for this pose are taken as they are: nothing is launched for them
    calls = []
    original = refiner.points_from_template
    refiner.points_from_template = lambda *a: calls.append(a) or original(*a)
    again = refiner.extract_reference_features(dbids, pose, ref_u8, points=(feats.p3d, feats.slot_valid, feats.points_record))["1"]
    torch.cuda.synchronize()
    assert not calls and again.p3d is feats.p3d and torch.equal(again.valid, feats.valid)
    with pytest.raises(ValueError):
        refiner.extract_reference_features(dbids, pose, ref_u8)  # the option needs the depth plane or the points


def test_the_default_is_untouched(device, objects):
    (a, pa), (b, pb) = solo(device, objects, 0, None), solo(device, objects, 0, "sfm")
    assert np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
    for n in NAMES:
        assert list(a.pose_history[n]) == list(b.pose_history[n]) and "n_reference_points" not in a.pose_history[n]
        assert "reference_point_stride" not in a.pose_history[n]
    assert a.localizer.refiner.last_points_record is None and a._primed.points is None


# ----------------------------------------------------------------------------------------------------------------------
# lock-step
# ----------------------------------------------------------------------------------------------------------------------
class CountingOps:
    """``torch.ops.pixtrack`` with the views of every points_from_depth_views call noted."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name != "points_from_depth_views":
            return fn

        def counted(depth, *args):
            self.calls.append(len(depth))
            return fn(depth, *args)

        return counted


def check_against_solo(got, want, per_image_plan, what):
    if per_image_plan:
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, np.abs(got - want).max())
    else:
        print(f"{what}: lock-step against solo, max |difference| {np.abs(got[:, :12] - want[:, :12]).max():.3g}")
        assert np.abs(got[:, :12] - want[:, :12]).max() < 1e-3, (what, np.abs(got - want).max())
        assert np.array_equal(got[:, 12], want[:, 12])


@pytest.mark.parametrize("per_image_plan,lm_grid,n_groups", [(True, 32, 1), (False, 0, 1), (True, 32, 2)])
def test_lockstep_equals_solo_runs(device, objects, monkeypatch, per_image_plan, lm_grid, n_groups):
    want = [solo(device, objects, j, "template", lm_grid)[1] for j in range(K)]
    in_step, alone = CountingOps(multi_module.ops), CountingOps(refiner_module.ops)
    monkeypatch.setattr(multi_module, "ops", in_step)
    monkeypatch.setattr(refiner_module, "ops", alone)
    trackers = [mesh_tracker(device, obj, lm_grid, reference_points="template") for obj in objects["objs"]]
    multi = MultiObjectTracker(trackers, lm_workgroups=lm_grid, per_image_plan=per_image_plan, n_groups=n_groups)
    for i in range(N_FRAMES):
        ok = multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in objects["objs"]])
        assert all(ok), (i, ok)
    torch.cuda.synchronize()
    assert multi.solo_frames == K and multi.lockstep_frames == K * (N_FRAMES - 1)  # only the cold starts ran alone
    # one points call per step and group (group g holds trackers g, g + n_groups, ...); a cold start makes its own
    sizes = [len(range(g, K, n_groups)) for g in range(n_groups)]
    assert in_step.calls == sizes * (N_FRAMES - 1) and alone.calls == [1] * K
    assert multi.points_calls == n_groups * (N_FRAMES - 1)
    for j, tr in enumerate(trackers):
        check_against_solo(_poses(tr, NAMES), want[j], per_image_plan, f"object {j}")
        assert tr.template_frames_batched >= 4 and tr._primed.points is None
        gt = objects["objs"][j][0]["gt_poses"]
        r_err, t_err = errors(tr, gt)
        assert r_err < 2e-2 and t_err < 2e-2, (j, r_err, t_err)
        for n in NAMES:
            ret = tr.pose_history[n]
            assert ret["tracked"] and 0 < ret["n_reference_points"] <= 2048 and ret["reference_point_stride"] >= 1


@pytest.mark.parametrize("per_image_plan,lm_grid", [(True, 32), (False, 0)])
def test_a_mixed_set_runs_in_one_tracker(device, objects, per_image_plan, lm_grid):
    """One "sfm" mesh tracker, one "template" mesh tracker and one NeRF tracker: every member against its own solo run."""
    assets = make_tracking_assets(seed=1011, width=W, height=H, n_frames=N_FRAMES, n_points=3000)

    def nerf_tracker():
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
        tr.spp = 2
        if lm_grid:
            for opt in tr.localizer.optimizer:
                opt.conf.n_workgroups = lm_grid
        return tr

    nerf = nerf_tracker()
    nerf_frames = render_query_frames(assets, nerf.testbed)
    decisions = []
    for i in range(N_FRAMES):
        nerf.run_single_frame((NAMES[i], nerf_frames[i]))
        decisions.append(bool(nerf.success))
    torch.cuda.synchronize()
    want = [solo(device, objects, 0, "sfm", lm_grid)[1], solo(device, objects, 1, "template", lm_grid)[1], _poses(nerf, NAMES)]
    trackers = [mesh_tracker(device, objects["objs"][0], lm_grid), mesh_tracker(device, objects["objs"][1], lm_grid,
                                                                                reference_points="template"), nerf_tracker()]
    frames = [objects["objs"][0][2], objects["objs"][1][2], nerf_frames]
    multi = MultiObjectTracker(trackers, lm_workgroups=lm_grid, per_image_plan=per_image_plan, n_groups=1)
    for i in range(N_FRAMES):
        assert multi.run_single_frames([(NAMES[i], fr[i]) for fr in frames]) == [True, True, decisions[i]], i
    torch.cuda.synchronize()
    assert multi.solo_frames == 3 and multi.lockstep_frames == 3 * (N_FRAMES - 1) and multi.points_calls == N_FRAMES - 1
    for tr, w, what in zip(trackers, want, ("sfm mesh", "template mesh", "nerf")):
        check_against_solo(_poses(tr, NAMES), w, per_image_plan, what)
    assert "n_reference_points" not in trackers[0].pose_history[NAMES[2]] and "n_reference_points" in trackers[1].pose_history[NAMES[2]]
    assert trackers[0].template_frames_batched >= 4 and trackers[1].template_frames_batched >= 4


def test_render_points_are_still_refused(device, objects):
    assets = make_tracking_assets(seed=1011, width=W, height=H, n_frames=2, n_points=3000)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets, reference_points="render")
    with pytest.raises(ValueError, match="reference_points='render'"):
        MultiObjectTracker([tr])
    with pytest.raises(ValueError, match="mesh template.*reference_points"):
        mesh_tracker(device, objects["objs"][0], reference_points="render")
