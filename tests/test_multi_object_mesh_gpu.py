"""Lock-step tracking from mesh templates: K PixLocPoseTrackerR9(template=MeshTemplate(...)) states advanced together by
MultiObjectTracker, their frames drawn in one MeshTemplate.frames call per group and step.  Per object the results must
be those of the one-object tracker (test_multi_object_gpu.py holds the NeRF path to the same)."""
import pickle

import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, make_tracking_assets, render_mesh_query_frames, render_query_frames
from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations
from test_multi_object_gpu import _poses
from test_tracker_mesh_template_gpu import TRACKER_KEYS, write_textured_obj

pytestmark = pytest.mark.gpu

K, W, H, N_FRAMES = 3, 128, 96, 6
NAMES = [f"{i:06d}.png" for i in range(N_FRAMES)]


@pytest.fixture(scope="module")
def objects(device, tmp_path_factory):
    """Three mesh objects: (assets, renderer, query frames) each, and the solo runs per LM grid, made once."""
    objs = []
    for k in range(K):
        assets = make_mesh_tracking_assets(seed=1031 + k, width=W, height=H, n_frames=N_FRAMES,
                                           out_dir=tmp_path_factory.mktemp(f"mesh_object{k}"), device=device)
        V, F = assets["mesh"][:2]
        renderer = R.MeshRenderer(V, F, device, **assets["mesh_shading"])
        objs.append((assets, renderer, render_mesh_query_frames(assets, renderer)))
    return dict(objs=objs, solo={})


def mesh_tracker(device, obj, lm_grid=0):
    assets, renderer, _ = obj
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                             template=MeshTemplate(renderer, supersample=2))
    if lm_grid:
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = lm_grid
    return tr


def solo_runs(device, objects, lm_grid):
    if lm_grid not in objects["solo"]:
        runs = []
        for obj in objects["objs"]:
            tr = mesh_tracker(device, obj, lm_grid)
            for i in range(N_FRAMES):
                tr.run_single_frame((NAMES[i], obj[2][i]))
            torch.cuda.synchronize()
            runs.append(_poses(tr, NAMES))
            assert runs[-1][:, 12].all() and tr.template_frames_batched == 0
        objects["solo"][lm_grid] = runs
    return objects["solo"][lm_grid]


@pytest.mark.parametrize("per_image_plan,lm_grid,n_groups", [(True, 32, 1), (True, 32, 2), (False, 0, 1), (False, 0, 2)])
def test_lockstep_equals_solo_runs(device, objects, per_image_plan, lm_grid, n_groups):
    """With the per-image UNet plan and the solo LM grid the lock-step poses, success flags and costs are BIT-identical to
    three solo runs; with the defaults they agree below 1e-3 (test_lockstep_equals_solo_runs' bar, for its reason: another
    split-K partition moves an fp32 sum by an ulp and the LM's pose by a few 1e-4)."""
    solo = solo_runs(device, objects, lm_grid)
    trackers = [mesh_tracker(device, obj, lm_grid) for obj in objects["objs"]]
    multi = MultiObjectTracker(trackers, lm_workgroups=lm_grid, per_image_plan=per_image_plan, n_groups=n_groups)
    for i in range(N_FRAMES):
        ok = multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in objects["objs"]])
        assert all(ok), (i, ok)
    torch.cuda.synchronize()
    assert multi.solo_frames == K and multi.lockstep_frames == K * (N_FRAMES - 1)  # only the cold starts ran alone
    for j, tr in enumerate(trackers):
        got = _poses(tr, NAMES)
        assert tr.template_frames_batched >= 4, tr.template_frames_batched
        assert tr.render_ahead is False and tr.renders_ahead_used == 0
        if per_image_plan:
            assert np.array_equal(got.view(np.uint64), solo[j].view(np.uint64)), (j, np.abs(got - solo[j]).max())
        else:
            print(f"object {j}: lock-step against solo, max |difference| {np.abs(got[:, :12] - solo[j][:, :12]).max():.3g}")
            assert np.abs(got[:, :12] - solo[j][:, :12]).max() < 1e-3, (j, np.abs(got - solo[j]).max())
            assert np.array_equal(got[:, 12], solo[j][:, 12])
        gt = objects["objs"][j][0]["gt_poses"]
        for i in range(N_FRAMES):  # every frame tracked, at the project's bar for synthetic sequences
            ret = tr.pose_history[NAMES[i]]
            Rt, t = ret["T_refined"].numpy()
            r_err, t_err = geodesic_distance_for_rotations(Rt, gt[i][0]), float(np.linalg.norm(t - gt[i][1]))
            assert ret["tracked"] and ret["success"] and ret["template"] == "mesh"
            assert r_err < 2e-2 and t_err < 2e-2, (j, i, r_err, t_err)


def test_the_primed_planes_are_each_trackers_own_frame(device, objects):
    trackers = [mesh_tracker(device, obj) for obj in objects["objs"]]
    for tr, obj in zip(trackers, objects["objs"]):
        tr.run_single_frame((NAMES[0], obj[2][0]))  # the cold start: a pose and a camera
    planes = MeshTemplate.frames([tr.template for tr in trackers], [tr.pose for tr in trackers], [tr.camera for tr in trackers],
                                 [tr._reference_camera() for tr in trackers], workspace=R.FrameBatchWorkspace())
    assert len(planes) == K
    for tr, (nz, ref_u8) in zip(trackers, planes):
        own_nz, own_ref = tr.template.frame(tr.pose, tr.camera, tr._reference_camera())
        torch.cuda.synchronize()
        assert nz.shape == (H, W) and ref_u8.shape == (H, W, 3) and 0.03 < float(nz.float().mean()) < 0.9 and int(ref_u8.max()) > 150
        assert torch.equal(nz, own_nz) and torch.equal(ref_u8, own_ref)
        # a tracker takes primed planes at the primed pose object alone
        tr.prime(tr.pose, depth_nz=nz, ref_u8=ref_u8)
        mask, ref = tr._mask_and_reference(tr.pose, from_slot=False)
        frame_part_gone = lambda: tr._primed.depth_nz is None and tr._primed.ref_u8 is None and tr._primed.mutual is None
        assert ref is ref_u8 and frame_part_gone() and tr.template_frames_batched == 1
        assert torch.equal(mask, tr._mask_of(own_nz))
        tr.prime(object(), depth_nz=nz, ref_u8=ref_u8)
        mask, ref = tr._mask_and_reference(tr.pose, from_slot=False)
        torch.cuda.synchronize()
        assert ref is not ref_u8 and torch.equal(ref, own_ref) and frame_part_gone() and tr.template_frames_batched == 1
        tr._own = None


def test_nerf_and_mesh_trackers_share_one_lock_step_tracker(device, objects):
    """One NeRF object and two mesh objects: each kind takes its own render path, the UNet and LM batches are shared.
    Per-image plan and equal LM grids: every object's poses, decisions and costs are bit-identical to its solo run."""
    grid = 32
    solo = solo_runs(device, objects, grid)
    assets = make_tracking_assets(seed=1011, width=W, height=H, n_frames=N_FRAMES, n_points=3000)

    def nerf_tracker():
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
        tr.spp = 2
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = grid
        return tr

    nerf = nerf_tracker()
    nerf_frames = render_query_frames(assets, nerf.testbed)
    decisions = []
    for i in range(N_FRAMES):
        nerf.run_single_frame((NAMES[i], nerf_frames[i]))
        decisions.append(bool(nerf.success))
    torch.cuda.synchronize()
    nerf_solo = _poses(nerf, NAMES)
    assert sum(decisions) >= N_FRAMES - 1 and nerf.renders_ahead_used >= 1, (decisions, nerf.renders_ahead_used)
    trackers = [mesh_tracker(device, objects["objs"][0], grid), nerf_tracker(), mesh_tracker(device, objects["objs"][1], grid)]
    frames = [objects["objs"][0][2], nerf_frames, objects["objs"][1][2]]
    multi = MultiObjectTracker(trackers, lm_workgroups=grid, per_image_plan=True, n_groups=1)
    for i in range(N_FRAMES):
        assert multi.run_single_frames([(NAMES[i], fr[i]) for fr in frames]) == [True, decisions[i], True], i
    torch.cuda.synchronize()
    assert multi.solo_frames == 3 and multi.lockstep_frames == 3 * (N_FRAMES - 1)
    for tr, want in zip(trackers, (solo[0], nerf_solo, solo[1])):
        got = _poses(tr, NAMES)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    assert trackers[0].template_frames_batched >= 4 and trackers[2].template_frames_batched >= 4
    assert trackers[1].template_frames_batched == 0 and trackers[1].renders_ahead_used == nerf.renders_ahead_used


def test_the_command_line_on_two_mesh_objects(device, objects, tmp_path, monkeypatch, capsys):
    """--template mesh with one mesh, reference model and upright image per object: no snapshot, no nerf2sfm.pkl, no
    OBJ_AABB.  Poses equal the in-process lock-step run within 1e-3, as test_multi_object_cli_on_disk_assets holds the
    NeRF path."""
    from PIL import Image

    from pixtrack_amd.pose_trackers import multi_object_tracker as mcli

    two = objects["objs"][:2]
    trackers = [mesh_tracker(device, obj) for obj in two]
    multi = MultiObjectTracker(trackers, n_groups=2)
    for i in range(N_FRAMES):
        assert all(multi.run_single_frames([(NAMES[i], obj[2][i]) for obj in two]))
    torch.cuda.synchronize()
    objs, queries, outs, meshes = [], [], [], []
    for j, (assets, _, frames) in enumerate(two):
        obj, query, mesh_dir = tmp_path / f"obj{j}", tmp_path / f"query{j}", tmp_path / f"mesh{j}"
        (obj / "pixtrack").mkdir(parents=True)
        query.mkdir()
        mesh_dir.mkdir()
        torch.save(assets["weights"], obj / "pixtrack" / "pixloc_megadepth.pt")
        meshes.append(write_textured_obj(mesh_dir, *assets["mesh"]))
        for i, fr in enumerate(frames):
            Image.fromarray(np.clip(np.rint(fr.cpu().numpy()), 0, 255).astype(np.uint8)).save(query / NAMES[i])
        objs.append(obj); queries.append(query); outs.append(tmp_path / f"out{j}")
    for name in ("UPRIGHT_REF_IMG", "OBJ_AABB", "PIXTRACK_WEIGHTS"):
        monkeypatch.delenv(name, raising=False)
    capsys.readouterr()
    mcli.main(["--object_path", *map(str, objs), "--query", *map(str, queries), "--out_dir", *map(str, outs), "--debug", "1",
               "--template", "mesh", "--mesh", *map(str, meshes), "--reference_sfm", *[str(a["reference_dir"]) for a, _, _ in two],
               "--upright_ref_img", *[a["upright_ref_img"] for a, _, _ in two]])
    text = capsys.readouterr().out
    assert text.count("Cache hits: 0, misses: %d" % (N_FRAMES - 1)) == 2 and text.rstrip().endswith("Done")
    for j, tr in enumerate(trackers):
        with open(outs[j] / "poses.pkl", "rb") as f:
            poses = pickle.load(f)
        assert len(poses) == N_FRAMES and (outs[j] / "trackers.pkl").is_file()
        for i, key in enumerate(poses):
            assert str(key).endswith(NAMES[i]) and poses[key]["tracked"] and poses[key]["template"] == "mesh"
            Rc, tc = poses[key]["T_refined"].numpy()
            R0, t0 = tr.pose_history[NAMES[i]]["T_refined"].numpy()
            assert geodesic_distance_for_rotations(Rc, R0) < 1e-3 and np.linalg.norm(tc - t0) < 1e-3
