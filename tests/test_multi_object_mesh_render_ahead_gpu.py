"""Lock-step tracking from mesh templates built with render_ahead=True: behind a step's batched LM launch ONE
MeshTemplate.frames_ahead call draws the next frames of all the group's mesh trackers from view records formed on the
device; the next step's head-of-step call draws only the trackers that hold no verified frame.  Per object the poses are
bit-identical to the run with the option off."""
import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker, MutualOcclusion
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames
from test_multi_object_gpu import _poses
from test_tracker_mesh_template_gpu import TRACKER_KEYS

pytestmark = pytest.mark.gpu

K, W, H, N_FRAMES, LM_GRID = 3, 128, 96, 8, 32
NAMES = [f"{i:06d}.png" for i in range(N_FRAMES)]


@pytest.fixture(scope="module")
def objects(device, tmp_path_factory):
    objs = []
    for k in range(K):
        assets = make_mesh_tracking_assets(seed=1031 + k, width=W, height=H, n_frames=N_FRAMES,
                                           out_dir=tmp_path_factory.mktemp(f"mesh_ahead{k}"), device=device)
        V, F = assets["mesh"][:2]
        renderer = R.MeshRenderer(V, F, device, **assets["mesh_shading"])
        objs.append((assets, renderer, render_mesh_query_frames(assets, renderer)))
    return dict(objs=objs, runs={})


def run(device, objects, ahead, points="sfm", cold=None, mutual=None):
    """One lock-step sequence -> (the multi tracker, the trackers, per step the counters after it, the poses per object).
    ``cold`` = (step, object): that tracker is sent back to a cold start before that step."""
    key = (ahead, points, cold, None if mutual is None else tuple(mutual.scenes))
    if key in objects["runs"]:
        return objects["runs"][key]
    trackers = []
    for assets, renderer, _ in objects["objs"]:
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                                 template=MeshTemplate(renderer, supersample=2, render_ahead=ahead), reference_points=points)
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = LM_GRID
        trackers.append(tr)
    multi = MultiObjectTracker(trackers, lm_workgroups=LM_GRID, per_image_plan=True, mutual_occlusion=mutual)
    steps = []
    for i in range(N_FRAMES):
        if cold is not None and cold[0] == i:
            trackers[cold[1]].cold_start = True
        multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in objects["objs"]])
        steps.append((multi.mesh_ahead_calls, multi.mesh_prime_calls, [tr.renders_ahead_used for tr in trackers],
                      [tr.template_frames_batched for tr in trackers]))
    torch.cuda.synchronize()
    objects["runs"][key] = (multi, trackers, steps, [_poses(tr, NAMES) for tr in trackers])
    return objects["runs"][key]


def same(got, want):
    for j, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (j, np.abs(a - b).max())


@pytest.mark.parametrize("points", ["sfm", "template"])
def test_one_posed_call_serves_the_group_and_the_poses_are_unchanged(device, objects, points):
    off_multi, off_trackers, off_steps, want = run(device, objects, False, points)
    multi, trackers, steps, got = run(device, objects, True, points)
    same(got, want)
    assert all(p[:, 12].all() for p in got)
    assert off_multi.mesh_ahead_calls == 0 and off_multi.mesh_prime_calls == N_FRAMES - 1
    assert all(tr.renders_ahead_used == 0 and tr.template_frames_batched >= N_FRAMES - 2 for tr in off_trackers)
    # step 0: three cold starts, alone.  Step 1: the head-of-step call draws all three, one posed call behind the LM launch.
    # From step 2 on every frame was drawn ahead: no head-of-step call, one posed call per step
    assert steps[0][:2] == (0, 0) and steps[1][:2] == (1, 1)
    for i in range(2, N_FRAMES):
        assert steps[i][0] == steps[i - 1][0] + 1 and steps[i][1] == 1, (i, steps[i])
        assert steps[i][2] == [i - 1] * K, (i, steps[i])
    for tr in trackers:
        assert tr.render_ahead is True and tr.renders_ahead_rejected == 0 and tr.renders_ahead_dropped == 0
        assert tr.renders_ahead_stale == 0 and tr.template_frames_batched == 1
    if points == "template":  # the points of a step still come from ONE call, whoever drew the planes
        assert multi.points_calls == off_multi.points_calls == N_FRAMES - 1
        for tr, ref in zip(trackers, off_trackers):
            for name in NAMES:
                assert tr.pose_history[name]["n_reference_points"] == ref.pose_history[name]["n_reference_points"]


def test_a_cold_start_is_drawn_by_the_head_of_step_call(device, objects):
    cold = (4, 1)
    _, _, _, want = run(device, objects, False, cold=cold)
    multi, trackers, steps, got = run(device, objects, True, cold=cold)
    same(got, want)
    assert multi.solo_frames == K + 1
    # step 4: tracker 1 runs alone, the others were drawn ahead; step 5: the head-of-step call draws tracker 1 alone
    assert steps[4][1] == steps[3][1] and steps[5][1] == steps[4][1] + 1 and steps[6][1] == steps[5][1]
    assert steps[5][3][1] == steps[4][3][1] + 1 and steps[5][3][0] == steps[4][3][0] and steps[5][3][2] == steps[4][3][2]
    assert steps[5][2][0] == steps[4][2][0] + 1 and steps[5][2][1] == steps[4][2][1] and steps[6][2][1] == steps[5][2][1] + 1
    assert all(tr.renders_ahead_rejected == 0 and tr.renders_ahead_dropped == 0 for tr in trackers)


def test_mutual_occlusion_draws_nothing_ahead(device, objects):
    option = lambda: MutualOcclusion(scenes=[0, 0, None], r_grow=1)
    off_multi, _, _, want = run(device, objects, False, mutual=option())
    multi, trackers, steps, got = run(device, objects, True, mutual=option())
    same(got, want)
    assert multi.mesh_ahead_calls == 0 and multi.mesh_prime_calls == off_multi.mesh_prime_calls == N_FRAMES - 1
    assert all(tr.renders_ahead_used == 0 and tr.renders_ahead_rejected == 0 for tr in trackers)
