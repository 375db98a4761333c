"""relocalizer="mesh": the relocaliser for a mesh-template tracker, and its depth stage.

The object is make_mesh_tracking_assets' synthetic mesh at 640 x 480 (the size of tests/test_relocalize_gpu.py); the bank holds its 42 mapping views at 8 rolls (45
degrees apart), drawn by the template.  The sensor frames are uint16 counts of the mesh's own depth render at the ground
truth, 0 off the object (the helper of tests/test_tracker_mesh_sensor_gpu.py, restated).  The cases and bounds are those
of tests/test_relocalize_gpu.py (ROT_TOL / TRANS_TOL restated), with ground truths rolled to within 5 degrees of a banked
roll, as there.

Only distance factor 1.0 is asserted end to end: the synthetic UNet's descriptors are not scale-invariant
(make_mesh_tracking_assets) and the bank's features are drawn at the mapping distance."""
import math

import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd import relocalizer as RL
from pixtrack_amd.geometry import Camera, Pose
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, perturb_pose, render_mesh_query_frames, rodrigues
from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 2e-2, 0.05  # tests/test_relocalize_gpu.py's
W, H = 640, 480
ROLLS = 8
TRACKER_KEYS = ("model3d", "weights", "covis", "upright_ref_img")
SENSOR_SCALE = 1e-4  # SfM units per count: the object sits 3-4 units away
GRID, DISTANCES = (4, 3), (0.8, 1.0, 1.25)
# how many placements go on to the feature scorer.  Measured at 320 x 240 with a 5 x 4 grid and the default 512: the
# depth stage ranked the right placement 0th to 4th of 20 496 on all six frames of (b), but on one of them the feature
# scorer then ranked it 20th of the 512, outside the K = 8 that are refined, and the frame ended 2.95 rad away; with 64
# it ranked 0th to 4th
N_GEOMETRIC = 64


def mesh_tracker(device, assets, renderer, **kw):
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                               template=MeshTemplate(renderer, supersample=2), **kw)


def frames_at(assets, renderer, poses, seed=5, cold=()):
    a = dict(assets)
    a["gt_poses"] = poses
    return render_mesh_query_frames(a, renderer, seed=seed, cold_start_indices=cold)


def sensor_at(assets, renderer, pose):
    """uint16 counts of the mesh's depth at ``pose`` = (R, t) seen by the query camera; 0 off the object."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = pose
    camera = Camera.from_colmap(assets["query_camera"])
    g = renderer.render_frame([(R.view_record(camera, T), W, H, 1, ("depth",))], download_records=False)[0]["depth"].cpu().numpy()
    z = np.where(g[..., 3] > 0, g[..., 0], 0.0)  # depth_q = 1: the depth itself
    assert z.max() / SENSOR_SCALE < 65535
    return np.rint(z / SENSOR_SCALE).astype(np.uint16)


def err(pose, Rg, tg):
    Rp, tp = pose.numpy()
    return geodesic_distance_for_rotations(Rp, Rg), float(np.linalg.norm(np.asarray(tp) - tg))


def rolled(Rv, tv, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return Rz @ Rv, Rz @ tv


def about_axis(assets, pose, deg):
    """The pose after the object turned by ``deg`` about its long axis (the orbit's axis) through its centre."""
    Rp, tp = pose
    c = assets["center"]
    dR = rodrigues(np.array([0.0, 0.0, 1.0]) * math.radians(deg))
    return Rp @ dR, Rp @ (c - dR @ c) + tp


def reset_cold(tr, relocalizer):
    tr.relocalizer = relocalizer
    tr.pose, tr.cold_start, tr.success, tr._lost, tr._accepted_pose = None, True, True, False, None
    tr.cost_threshold, tr.dynamic_id, tr.cache_hit = None, None, False
    tr._reference_by_side = False  # (as a fresh tracker: set by a relocalisation with relocalizer="mesh")
    tr.reference_ids = tr._initial_reference_ids({"upright_ref_img": tr.localizer.model3d.dbs[1].name})


# test_localize_far_from_the_upright_view's case set - three mapping views 90 degrees or more from the upright view 1,
# each rolled by 40 and 130 degrees - in THIS model's view order: the mesh builder's views 5, 9 and 16 are 120, 152 and
# 122 degrees from its view 1 (its view 13, the third view of the NeRF assets' set, is only 35 degrees away)
FAR_VIEWS, FAR_ROLLS = (5, 9, 16), (40.0, 130.0)


def far_poses(assets, dbs, seed=21):
    """Ground truths near the mapping views FAR_VIEWS, rolled in-plane by 40 and 130 degrees, then perturbed by up to 5
    degrees / 1 cm -> [(R, t)], [(view, nearest banked roll)]."""
    rng = np.random.default_rng(seed)
    gts, owners = [], []
    for v in FAR_VIEWS:
        for roll in FAR_ROLLS:
            Rr, tr_ = rolled(dbs[v].qvec2rotmat(), dbs[v].tvec, roll)
            gts.append(perturb_pose(Rr, tr_, rng, float(rng.uniform(0, 5)), float(rng.uniform(0, 0.01)), assets["center"]))
            owners.append((v, int(round(roll / (360.0 / ROLLS))) % ROLLS))
    return gts, owners


def moved_to(assets, camera10, pose, pixel):
    """``pose`` with the object's centre moved onto ``pixel`` at its own depth."""
    Rp, tp = pose
    fx, fy, cx, cy = camera10[2:6]
    c = Rp @ assets["center"] + tp
    placed = c[2] * np.array([(pixel[0] - cx) / fx, (pixel[1] - cy) / fy, 1.0])
    return Rp, tp + placed - c


def row(ret, pose, gt):
    """What a frame did: tracked (refiner AND gate), its pose against the ground truth, its refined pose (before the gate)."""
    rot, tra = err(pose, *gt)
    refined = ret.get("T_refined")
    rrot, rtra = err(refined, *gt) if refined is not None else (float("inf"), float("inf"))
    return {"tracked": bool(ret["tracked"]), "close": rot < ROT_TOL and tra < TRANS_TOL, "rot": round(rot, 4),
            "refined_close": bool(ret["success"]) and rrot < ROT_TOL and rtra < TRANS_TOL, "cost": float(ret["cost"]),
            "relocalised": bool(ret.get("relocalized", False)), "n_placed": ret.get("reloc_n_placed")}


def track(tr, frames, names_from=0):
    for i, fr in enumerate(frames):
        name = f"{names_from + i:06d}.png"
        tr.run_single_frame((name, fr))
        yield tr.pose_history[name], tr.pose


@pytest.fixture(scope="module")
def scene(device, tmp_path_factory):
    """The object, its renderer and ONE tracker with relocalizer="mesh" and a depth stage; the stage runs on the frames
    whose names the ``sensors`` dict holds, every other frame is relocalised on features alone."""
    assets = make_mesh_tracking_assets(seed=1031, width=W, height=H, n_frames=20, out_dir=tmp_path_factory.mktemp("mesh_reloc"),
                                       device=device)
    V, F = assets["mesh"][:2]
    renderer = R.MeshRenderer(V, F, device, **assets["mesh_shading"])
    sensors = {}
    depth = RL.RelocDepth(lookup=sensors.get, sensor_depth_scale=SENSOR_SCALE, grid=GRID, distances=DISTANCES, depth_points=128,
                          n_geometric=N_GEOMETRIC)
    tr = mesh_tracker(device, assets, renderer, relocalizer="mesh", reloc_depth=depth, reloc_options=dict(rolls=ROLLS))
    return dict(assets=assets, renderer=renderer, tr=tr, sensors=sensors)


def test_localize_far_from_the_upright_view(scene):
    """(a) RGB only."""
    assets, renderer, tr = scene["assets"], scene["renderer"], scene["tr"]
    dbs = tr.localizer.model3d.dbs
    gts, _ = far_poses(assets, dbs)
    frames = frames_at(assets, renderer, gts)
    reloc = tr.relocalizer
    own, primed = tr._own, tr._primed
    for k, ((Rg, tg), fr) in enumerate(zip(gts, frames)):
        tr.camera = tr.get_query_camera(fr)
        res = reloc.localize(fr, tr.camera)
        assert res.pose is not None and res.n_hypotheses == reloc.n_views * ROLLS == len(reloc.views) == 42 * ROLLS
        assert res.n_placed is None and res.n_geometric is None
        rot, tra = err(res.pose, Rg, tg)
        print(f"far {k}: rot {rot:.4f} trans {tra:.4f} view {res.view_id}")
        assert rot < ROT_TOL and tra < TRANS_TOL, (k, rot, tra, res.view_id, [c["cost"] for c in res.candidates])
    assert tr._own is own and tr._primed is primed  # the bank's views were drawn beside the frame's planes
    # the default cold start (upright pose, then refine at scales [4, 1]) on the same frames does not get there
    try:
        for k, ((Rg, tg), fr) in enumerate(zip(gts, frames)):
            reset_cold(tr, None)
            tr.run_single_frame((f"{k:06d}.png", fr))
            rot, _ = err(tr.pose, Rg, tg)
            print(f"far {k}: the default cold start ends {rot:.3f} rad away")
            assert rot > 0.3, (k, rot)
    finally:
        reset_cold(tr, reloc)


def test_the_depth_stage_places_an_off_centre_object(scene):
    """(b): the far views at the mapping distance, the object's centre on a grid cell away from the image centre."""
    assets, renderer, tr = scene["assets"], scene["renderer"], scene["tr"]
    dbs = tr.localizer.model3d.dbs
    reloc = tr.relocalizer
    gts, owners = far_poses(assets, dbs)
    camera = Camera.from_colmap(assets["query_camera"])
    cam10 = [float(x) for x in camera.as10().tolist()]
    cells = [(2, 1), (1, 1), (2, 1), (1, 1), (2, 1), (1, 1)]  # the two cells beside the image centre: 80 px (6 degrees) off it
    centres = RL.cell_centres(cam10, GRID)
    moved = [moved_to(assets, cam10, gt, centres[j * GRID[0] + i]) for gt, (i, j) in zip(gts, cells)]
    frames = frames_at(assets, renderer, moved)
    ids = sorted(dbs)
    one = DISTANCES.index(1.0)
    for k, ((Rg, tg), fr, (v, roll), cell) in enumerate(zip(moved, frames, owners, cells)):
        tr.camera = tr.get_query_camera(fr)
        sensor = torch.from_numpy(sensor_at(assets, renderer, (Rg, tg)).view(np.int16)).to(tr.device)
        res = reloc.localize(fr, tr.camera, sensor=sensor)
        entry = ids.index(v) * ROLLS + roll
        assert reloc.views[entry].dbid == v and reloc.views[entry].roll == roll
        want = reloc.placement_index(entry, one, cell)
        kept = reloc.last_geometric.cpu().tolist()
        assert res.n_placed == len(reloc.views) * (1 + len(DISTANCES) * GRID[0] * GRID[1]) and res.n_geometric == N_GEOMETRIC
        assert len(kept) == N_GEOMETRIC and len(set(kept)) == N_GEOMETRIC
        rot, tra = err(res.pose, Rg, tg) if res.pose is not None else (float("inf"), float("inf"))
        placed, fscore = (x.cpu().tolist() for x in reloc.last_feature_scores)
        order = [placed[i] for i in np.argsort(np.asarray(fscore), kind="stable")]
        print(f"moved {k} cell {cell}: the right placement {want} at depth rank {kept.index(want) if want in kept else None} of "
              f"{len(kept)}, feature rank {order.index(want) if want in order else None}; rot {rot:.4f} trans {tra:.4f}; refined "
              f"{[(c['hypothesis'], round(c['cost'], 4)) for c in res.candidates]}")
        assert want in kept, (k, want)
        assert rot < ROT_TOL and tra < TRANS_TOL, (k, rot, tra, [c["cost"] for c in res.candidates])
    # recorded, not asserted: the same frames through the feature-only relocaliser (shifts = 1)
    for k, ((Rg, tg), fr) in enumerate(zip(moved, frames)):
        res = reloc.localize(fr, tr.camera)
        rot, tra = err(res.pose, Rg, tg) if res.pose is not None else (float("inf"), float("inf"))
        print(f"moved {k} without the depth stage: rot {rot:.4f} trans {tra:.4f} ok {rot < ROT_TOL and tra < TRANS_TOL}")


def test_lost_track_recovery(scene, device):
    """(c) Ten frames of the assets' orbit, then the object turns by 120 degrees (a cut), then ten more.  (Behind the cut
    the camera is rolled against every mapping view: with the reference image chosen by rotation the frames after the
    relocalised one ended 0.012, 0.023 and 0.033 rad away; chosen by side, 0.0002 - 0.0005: DESIGN 3.26.)"""
    assets, renderer, tr = scene["assets"], scene["renderer"], scene["tr"]
    gt = assets["gt_poses"]
    gts = gt[:10] + [about_axis(assets, p, 120.0) for p in gt[10:20]]
    frames = frames_at(assets, renderer, gts, seed=8, cold=(0,))
    off_tr = mesh_tracker(device, assets, renderer)
    off = [row(ret, pose, gts[i]) for i, (ret, pose) in enumerate(track(off_tr, frames))]
    reset_cold(tr, tr.relocalizer)
    n0 = tr.relocalization_count
    on = [row(ret, pose, gts[i]) for i, (ret, pose) in enumerate(track(tr, frames))]
    thr_on = tr.cost_threshold
    for name, rows in (("off", off), ("mesh", on)):
        print(name, thr_on, [(i, r["tracked"], r["refined_close"], r["relocalised"], r["rot"], round(r["cost"], 4)) for i, r in enumerate(rows)])
    assert all(r["tracked"] and r["close"] for r in off[:10]), (off, off_tr.cost_threshold)
    assert not any(r["tracked"] and r["close"] for r in off[10:]), (off, off_tr.cost_threshold)  # the track is lost for good
    # With the relocaliser every frame from the second after the cut is on the object.  Whether the tracker ACCEPTS it is
    # the reference's frozen gate (cost <= 1.1 x the cold-start frame's cost, kept as is: DESIGN 3.4): a frame the gate
    # rejects is relocalised on the next one, and the gate is the only reason a frame goes untracked.
    for r in on[:1] + on[11:]:
        assert r["refined_close"] and (r["tracked"] or r["cost"] > thr_on), (on, thr_on)
    assert any(r["relocalised"] for r in on[11:]), (on, thr_on)
    assert tr.relocalization_count - n0 >= 2
    assert all(r["n_placed"] is None for r in on)  # no frame of this sequence has a sensor image
    assert all(("reloc_n_placed" in ret) == bool(ret.get("relocalized")) for ret in tr.pose_history.values())


def test_start_segment_without_a_pose_relocalises_with_and_without_depth(scene):
    """(c) start_segment(None), on features alone and - the frames named in the lookup - through the depth stage, the
    frame's sensor image staged once by the tracker."""
    assets, renderer, tr, sensors = scene["assets"], scene["renderer"], scene["tr"], scene["sensors"]
    dbs = tr.localizer.model3d.dbs
    start = rolled(dbs[9].qvec2rotmat(), dbs[9].tvec, 85.0)
    gts = [about_axis(assets, start, 0.5 * i) for i in range(3)]
    frames = frames_at(assets, renderer, gts, seed=11, cold=(0,))
    for names_from, with_depth in ((300, False), (400, True)):
        if with_depth:
            sensors.update({f"{names_from + i:06d}.png": sensor_at(assets, renderer, g) for i, g in enumerate(gts)})
        tr.start_segment(None)
        n0, u0 = tr.relocalization_count, tr.sensor_uploads
        rows = [row(ret, pose, gts[i]) for i, (ret, pose) in enumerate(track(tr, frames, names_from=names_from))]
        print(with_depth, rows)
        assert rows[0]["relocalised"] and rows[0]["tracked"] and rows[0]["close"], rows
        assert all(r["refined_close"] and (r["tracked"] or r["cost"] > tr.cost_threshold) for r in rows), (rows, tr.cost_threshold)
        assert tr.relocalization_count >= n0 + 1
        assert tr.sensor_uploads - u0 == (len(frames) if with_depth else 0)
        assert (rows[0]["n_placed"] is not None) == with_depth
        if with_depth:
            first = tr.pose_history[f"{names_from:06d}.png"]
            assert first["reloc_n_geometric"] == N_GEOMETRIC and first["reloc_n_placed"] == tr.relocalizer.n_placed


def test_the_option_changes_no_pose_when_nothing_is_relocalised(scene, device):
    """(d): from view 1, every frame tracked - relocalizer="mesh" against the option off, bit for bit."""
    assets, renderer = scene["assets"], scene["renderer"]
    frames = frames_at(assets, renderer, assets["gt_poses"][:6], seed=5, cold=(0,))
    db1 = assets["model3d"].dbs[1]
    runs = []
    for kw in (dict(), dict(relocalizer="mesh", reloc_options=dict(rolls=ROLLS))):
        t2 = mesh_tracker(device, assets, renderer, **kw)
        if kw:  # (the cold start of a tracker with a relocaliser is a relocalisation unless the segment is given its pose)
            t2.start_segment(Pose.from_Rt(db1.qvec2rotmat(), db1.tvec))
        rets = [(ret, pose.numpy()) for ret, pose in track(t2, frames)]
        runs.append((t2, rets))
    (off, a), (on, b) = runs
    assert on.relocalizer is not None and on.relocalizer.bank is None and off.relocalizer is None
    for (ra, pa), (rb, pb) in zip(a, b):
        assert ra["tracked"] and rb["tracked"] and rb["relocalized"] is False and "relocalized" not in ra
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
        assert ra["cost"] == rb["cost"] and "reloc_n_placed" not in rb
