"""Lock-step tracking of mesh objects with the sensor options: two mesh-template trackers with
``reference_points="template"``, ``occlusion`` and ``depth_refine`` on, ONE shared lookup - the two objects of one RGB-D
stream.  Per step and group the sensor image is staged once, ONE pxt_occlusion_mask_views call serves every tracker
that takes a mask and ONE pxt_depth_refine call every tracker that asked.

The configuration is the one documented as bit-identical to solo runs (per-image UNet plan, solo LM grid,
tests/test_multi_object_mesh_gpu.py): per object the poses and the options' history keys equal the solo tracker's with
the same options, bit for bit.

The shared sensor image holds object 0's depth where object 0 covers the pixel, else object 1's, else a far
background: exact for object 0, and for object 1 partly another surface - an occluder where it lies in front."""
import numpy as np
import pytest
import torch

from pixtrack_amd import depth_refinement as DR
from pixtrack_amd import occlusion as OC
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from test_multi_object_gpu import _poses
from test_tracker_mesh_sensor_gpu import MAX_COUNT, NAMES, counts_of, mesh_object, mesh_tracker

pytestmark = pytest.mark.gpu

STEPS = 4
GRID = 32
KEYS = OC.HISTORY_KEYS + tuple(k for k in DR.HISTORY_KEYS if k != "T_lm")


@pytest.fixture(scope="module")
def pair(device, tmp_path_factory):
    objs = [mesh_object(device, 1031 + k, tmp_path_factory.mktemp(f"mesh_sensor_pair{k}")) for k in range(2)]
    z0, z1 = objs[0][3], objs[1][3]
    z = np.where(z0 > 0, z0, z1)
    scale = float(z.max() / MAX_COUNT)
    images = counts_of(z, scale)
    # ONE absolute conf for both objects: pxt_depth_refine takes one conf per call, and a relative conf resolves to each
    # object's own extent
    conf = DR.DepthRefineConf.from_sfm_scale(DR.points_extent(objs[0][0]["mesh"][0]))
    return dict(objs=objs, images=images, scale=scale, conf=conf, solo={})


def options(pair, relative=False):
    """A fresh lookup object and the two options that name it."""
    look = {n: pair["images"][k] for k, n in enumerate(NAMES)}.get
    conf = {} if relative else {"conf": pair["conf"]}
    return dict(occlusion=OC.OcclusionMask(lookup=look, sensor_depth_scale=pair["scale"]),
                depth_refine=DR.DepthRefine(lookup=look, sensor_depth_scale=pair["scale"], **conf))


def tracker(device, pair, j, opts):
    return mesh_tracker(device, pair["objs"][j], GRID, reference_points="template", **opts)


def solo(device, pair, j):
    if j not in pair["solo"]:
        tr = tracker(device, pair, j, options(pair))
        for i in range(STEPS):
            tr.run_single_frame((NAMES[i], pair["objs"][j][2][i]))
        torch.cuda.synchronize()
        pair["solo"][j] = tr
    return pair["solo"][j]


def same_value(a, b):
    if a is None or b is None or isinstance(a, bool):
        return a is b or a == b
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_lockstep_equals_solo_runs_with_both_options(device, pair):
    want = [solo(device, pair, j) for j in range(2)]
    shared = options(pair)  # ONE lookup for both trackers
    trackers = [tracker(device, pair, j, shared) for j in range(2)]
    multi = MultiObjectTracker(trackers, lm_workgroups=GRID, per_image_plan=True, n_groups=1)
    for i in range(STEPS):
        before = (multi.occlusion_view_calls, multi.depth_refine_calls, multi.sensor_uploads, multi.lockstep_frames)
        multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in pair["objs"]])
        rets = [tr.pose_history[NAMES[i]] for tr in trackers]
        in_step = multi.lockstep_frames - before[3]
        masks = sum(bool(r["occlusion_applied"]) for r in rets) if in_step else 0
        assert multi.occlusion_view_calls - before[0] == (1 if masks else 0), i
        assert multi.depth_refine_calls - before[1] == (1 if in_step else 0), i
        assert multi.sensor_uploads - before[2] == (1 if in_step else 0), i  # one image for both trackers
    torch.cuda.synchronize()
    assert multi.solo_frames == 2 and multi.lockstep_frames == 2 * (STEPS - 1)  # only the cold starts ran alone
    assert multi.occlusion_view_calls >= 1 and multi.depth_refine_calls == STEPS - 1 and multi.sensor_uploads == STEPS - 1
    assert [tr.sensor_uploads for tr in trackers] == [1, 1]  # the cold starts staged their own
    for j, (tr, ref) in enumerate(zip(trackers, want)):
        got, exp = _poses(tr, NAMES[:STEPS]), _poses(ref, NAMES[:STEPS])
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (j, np.abs(got - exp).max())
        assert tr._primed.occlusion is None and tr._primed.points is None
        for n in NAMES[:STEPS]:
            a, b = tr.pose_history[n], ref.pose_history[n]
            assert set(a) == set(b)
            for key in KEYS:
                assert same_value(a[key], b[key]), (j, n, key, a[key], b[key])
            if a.get("success"):
                assert np.array_equal(a["T_lm"].as12().double().numpy().view(np.uint64),
                                      b["T_lm"].as12().double().numpy().view(np.uint64)), (j, n)
    assert any(tr.pose_history[n]["occlusion_applied"] for tr in trackers for n in NAMES[:STEPS])
    assert any(tr.pose_history[n]["depth_cost_before"] is not None for tr in trackers for n in NAMES[:STEPS])


def test_a_tracker_alone_in_a_step_and_two_lookups(device, pair):
    """A step in which one tracker sits out still completes - the other one's pass is a one-view call; two lookup
    objects (equal content) are two uploads per step."""
    trackers = [tracker(device, pair, j, options(pair)) for j in range(2)]  # a lookup object each
    multi = MultiObjectTracker(trackers, lm_workgroups=GRID, per_image_plan=True, n_groups=1)
    frames = lambda i: [(NAMES[i], obj[2][i]) for obj in pair["objs"]]
    multi.run_single_frames(frames(0))
    multi.run_single_frames(frames(1))
    assert multi.sensor_uploads == 2 and multi.depth_refine_calls == 1
    calls = multi.occlusion_view_calls
    step = frames(2)
    step[1] = None  # tracker 1 sits this step out
    out = multi.run_single_frames(step)
    assert out[1] is None and out[0] is not None
    assert multi.sensor_uploads == 3 and multi.depth_refine_calls == 2
    assert multi.occlusion_view_calls - calls == (1 if trackers[0].pose_history[NAMES[2]]["occlusion_applied"] else 0)
    want = solo(device, pair, 0)
    got, exp = _poses(trackers[0], NAMES[:3]), _poses(want, NAMES[:3])
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    torch.cuda.synchronize()



def test_confs_that_differ_go_out_in_a_call_each(device, pair):
    """Relative confs resolve to each object's own extent: one pxt_depth_refine call per distinct conf."""
    shared = options(pair, relative=True)
    trackers = [tracker(device, pair, j, shared) for j in range(2)]
    assert trackers[0]._depth_conf != trackers[1]._depth_conf
    multi = MultiObjectTracker(trackers, lm_workgroups=GRID, per_image_plan=True, n_groups=1)
    for i in range(2):
        multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in pair["objs"]])
    torch.cuda.synchronize()
    assert multi.depth_refine_calls == 2 and multi.sensor_uploads == 1 and multi.lockstep_frames == 2
    assert all("depth_refined" in tr.pose_history[NAMES[1]] for tr in trackers)


def test_frames_drawn_ahead_join_the_one_occlusion_call(device, pair):
    """Occlusion alone leaves the templates' render_ahead usable: the planes of frames drawn ahead, behind the last
    step's LM launch, go through the step's ONE views call too, and the poses stay the solo runs' (which render ahead
    as well) bit for bit."""
    def make(j, opts):
        return mesh_tracker(device, pair["objs"][j], GRID, render_ahead=True, reference_points="template",
                            occlusion=opts["occlusion"])

    want = []
    for j in range(2):
        tr = make(j, options(pair))
        for i in range(STEPS):
            tr.run_single_frame((NAMES[i], pair["objs"][j][2][i]))
        want.append(tr)
    shared = options(pair)
    trackers = [make(j, shared) for j in range(2)]
    multi = MultiObjectTracker(trackers, lm_workgroups=GRID, per_image_plan=True, n_groups=1)
    for i in range(STEPS):
        multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in pair["objs"]])
    torch.cuda.synchronize()
    assert sum(tr.renders_ahead_used for tr in trackers) > 0 and multi.mesh_ahead_calls > 0
    assert multi.occlusion_view_calls == sum(any(tr.pose_history[NAMES[i]]["occlusion_applied"] for tr in trackers)
                                             for i in range(1, STEPS))
    assert multi.depth_refine_calls == 0 and multi.sensor_uploads == STEPS - 1
    for j, (tr, ref) in enumerate(zip(trackers, want)):
        got, exp = _poses(tr, NAMES[:STEPS]), _poses(ref, NAMES[:STEPS])
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (j, np.abs(got - exp).max())
        for n in NAMES[:STEPS]:
            for key in OC.HISTORY_KEYS:
                assert same_value(tr.pose_history[n][key], ref.pose_history[n][key]), (j, n, key)
