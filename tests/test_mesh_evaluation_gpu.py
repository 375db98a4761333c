"""Mesh-based pose evaluation: the rasteriser's images through pxt_depth_agreement / pxt_sensor_vsd against the numpy
restatements on the restated images, the command line on a mesh extracted from the synthetic NeRF, and the extracted
mesh against its NeRF."""
import json

import numpy as np
import pytest
import torch

from pixtrack_amd import mesh as M
from pixtrack_amd import mesh_evaluation as ME
from pixtrack_amd import mesh_render as R
from pixtrack_amd import render_evaluation as RE
from pixtrack_amd import sensor_evaluation as SE
from pixtrack_amd.geometry import Camera, Pose
from test_mesh_raster_host import rotation

pytestmark = pytest.mark.gpu

W, H, N = 96, 72, 4
NEAR = ME.DEFAULT_NEAR
AGREE_EXACT = [0, 1, 2, 3, 5, 6, 7] + list(range(8, 24))   # word 4 is a float sum: see sum_close
SENSOR_EXACT = [0, 1, 2, 3] + list(range(5, 32))


def sum_close(word4, sums, n_terms):
    """Word 4 holds a float32 sum of n non-negative float32 terms in the kernel's own order: whatever that order, it is
    within n * 2^-24 (relative) of the exact sum."""
    got = np.ascontiguousarray(word4).view(np.float32).astype(np.float64)
    return bool((np.abs(got - sums) <= np.maximum(n_terms, 1) * 2.0 ** -24 * np.abs(sums) + 1e-30).all())


@pytest.fixture(scope="module")
def scene(device):
    """An ellipsoid of 1280 triangles (no symmetry the poses could hide in), a camera whose fx != fy and whose principal
    point is off centre, N ground-truth poses, the restatement's images of them, and sensor images made of those."""
    V, F = R.icosphere(3)
    V = V * np.asarray([0.1, 0.07, 0.05])
    diameter = 0.2
    camera = Camera(torch.tensor([float(W), float(H), 236.0, 222.0, 44.3, 38.6]))
    T_gt = np.tile(np.eye(4), (N, 1, 1))
    for k in range(N):
        T_gt[k, :3, :3], T_gt[k, :3, 3] = rotation(30 + k), (0.01 * k, -0.01, 1.1 + 0.02 * k)
    views = np.stack([R.view_record(camera, T_gt[k], NEAR, 1.0) for k in range(N)])
    gt_ref = R.rasterize_reference(V, F, views, W, H)[0]
    on = gt_ref[..., 3] == 1.0
    ray = ME.mesh_ray_factors(camera)
    z = np.where(on, gt_ref[..., 0].astype(np.float64), 0.0)  # a depth sensor stores camera-axis depth
    depth_scale = float(z.max() / 20000)  # mesh units per raw count
    counts = np.rint(z / depth_scale)
    assert on.sum(axis=(1, 2)).min() > 300 and depth_scale < 0.01 * SE.DEFAULT_DELTA
    free = np.where(on, counts, 3 * counts.max()).astype(np.uint16)  # the object in front of a far background
    occluded, slab = free.copy(), np.zeros((N, H, W), bool)
    for k in range(N):  # a slab in front of the object's left third (and of everything left of it)
        cols = np.nonzero(on[k].any(axis=0))[0]
        slab[k, :, :cols[0] + (cols[-1] - cols[0] + 1) // 3] = True
    occluded[slab] = int(counts[on].min() // 2)
    return dict(V=V, F=F, diameter=diameter, camera=camera, T_gt=T_gt, gt_ref=gt_ref, on=on, ray=ray,
                depth_scale=depth_scale, free=free, occluded=occluded, slab=slab, renderer=R.MeshRenderer(V, F, device))


def perturbed(scene, seed, rot_deg, trans):
    from pixtrack_amd.synthetic import perturb_pose

    rng = np.random.default_rng(seed)
    T = scene["T_gt"].copy()
    for k in range(N):
        T[k, :3, :3], T[k, :3, 3] = perturb_pose(T[k, :3, :3], T[k, :3, 3], rng, rot_deg, trans, np.zeros(3))
    return T


def reference_images(scene, T):
    views = np.stack([R.view_record(scene["camera"], T[k], NEAR, 1.0) for k in range(N)])
    return R.rasterize_reference(scene["V"], scene["F"], views, W, H)[0]


# ------------------------------------------------------------------------------------------ images through the comparison
def test_raster_images_through_depth_agreement(device, scene):
    d = scene["diameter"]
    T_est = perturbed(scene, 5, 4.0, 0.03 * d)
    taus, tq = RE._thresholds(d, None, 1.0)
    est, _, rec_e = scene["renderer"].render_depth(np.stack([R.view_record(scene["camera"], T, NEAR, 1.0) for T in T_est]), W, H)
    gt, _, rec_g = scene["renderer"].render_depth(np.stack([R.view_record(scene["camera"], T, NEAR, 1.0) for T in scene["T_gt"]]), W, H)
    est_ref = reference_images(scene, T_est)
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), scene["gt_ref"].view(np.uint32))
    assert np.array_equal(est.cpu().numpy().view(np.uint32), est_ref.view(np.uint32))
    got = RE.depth_agreement(est, gt, tq, ME.MIN_ALPHA, device)
    want, sums = RE.depth_agreement_reference(est_ref, scene["gt_ref"], ME.MIN_ALPHA, tq)
    np.testing.assert_array_equal(got[:, AGREE_EXACT], want[:, AGREE_EXACT])
    assert sum_close(got[:, 4], sums, want[:, 2])
    assert np.array_equal(got[:, 0], rec_e[:, R.W_COVERED]) and np.array_equal(got[:, 1], rec_g[:, R.W_COVERED])
    res = ME.mesh_pose_errors(scene["renderer"], scene["camera"], T_est, scene["T_gt"], d)
    fig = RE.frame_figures(got, 1.0, n_taus=10, finite_slot=10)
    for key in ("vsd", "iou", "n_est", "n_gt", "n_both", "n_union", "mean_abs_dz", "max_abs_dz"):
        np.testing.assert_array_equal(res[key], fig[key])
    print("4 deg / 3 % of the diameter: vsd", res["vsd"].mean(axis=0), "iou", res["iou"], "mean |dz|", res["mean_abs_dz"])
    assert res["ok"].all() and (np.diff(res["vsd"], axis=1) <= 0).all() and (res["vsd"][:, 0] > 0).all()
    assert (res["vsd"][:, -1] < 0.5).all() and ((res["iou"] > 0.5) & (res["iou"] < 1)).all()


def test_identical_poses_and_a_push_along_the_axis(device, scene):
    d = scene["diameter"]
    same = ME.mesh_pose_errors(scene["renderer"], scene["camera"], scene["T_gt"], scene["T_gt"].copy(), d)
    assert same["ok"].all() and (same["vsd"] == 0.0).all() and (same["iou"] == 1.0).all()
    assert (same["mean_abs_dz"] == 0.0).all() and np.array_equal(same["n_est"], scene["on"].sum(axis=(1, 2)))
    # moved away along the optical axis by more than the largest tau (half the diameter): every overlap pixel is beyond
    # every tau, while the silhouette only shrinks by the ratio of the depths
    pushed = scene["T_gt"].copy()
    pushed[:, 2, 3] += 0.6 * d
    far = ME.mesh_pose_errors(scene["renderer"], [scene["camera"]] * N, pushed, scene["T_gt"], d)
    print("pushed by 0.6 d: iou", far["iou"], "mean |dz|", far["mean_abs_dz"])
    assert (far["vsd"] == 1.0).all() and (far["iou"] > 0.75).all() and (far["iou"] < 1).all()
    assert ((far["mean_abs_dz"] > 0.5 * d) & (far["mean_abs_dz"] < 0.7 * d)).all()
    # a non-finite pose is not drawn: a miss, and only that frame
    bad = pushed.copy()
    bad[1, 0, 0] = np.nan
    res = ME.mesh_pose_errors(scene["renderer"], scene["camera"], bad, scene["T_gt"], d)
    assert not res["ok"][1] and (res["vsd"][1] == 1).all() and res["iou"][1] == 0 and res["ok"][[0, 2, 3]].all()
    np.testing.assert_array_equal(res["iou"][[0, 2, 3]], far["iou"][[0, 2, 3]])


# -------------------------------------------------------------------------------------------------------- the sensor path
def test_sensor_records_and_the_visible_fraction(device, scene):
    from pixtrack_amd.ops import ops

    d = scene["diameter"]
    T_est = perturbed(scene, 6, 3.0, 0.02 * d)
    est_ref = reference_images(scene, T_est)
    taus, tq = RE._thresholds(d, None, 1.0)
    sensor_q, delta_q = float(np.float32(scene["depth_scale"])), float(np.float32(SE.DEFAULT_DELTA))
    want, sums = SE.sensor_vsd_reference(est_ref, scene["gt_ref"], scene["occluded"], scene["ray"], (0, 0), ME.MIN_ALPHA,
                                         sensor_q, delta_q, tq)
    views = lambda T: np.stack([R.view_record(scene["camera"], T[k], NEAR, 1.0) for k in range(N)])
    est = scene["renderer"].render_depth(views(T_est), W, H)[0]
    gt = scene["renderer"].render_depth(views(scene["T_gt"]), W, H)[0]
    records = torch.zeros(N, SE.RECORD, dtype=torch.int32, device=device)
    from pixtrack_amd import _lib
    ws = torch.empty(int(_lib.lib().pxt_sensor_vsd_workspace_bytes(N, W, H)), dtype=torch.uint8, device=device)
    ops.sensor_vsd(est, gt, torch.from_numpy(scene["occluded"].view(np.int16)).to(device),
                   torch.from_numpy(scene["ray"]).to(device), [0, 0], ME.MIN_ALPHA, sensor_q, delta_q, tq, records, ws)
    got = records.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[:, SENSOR_EXACT], want[:, SENSOR_EXACT])
    assert sum_close(got[:, 4], sums, want[:, 2])
    res = ME.mesh_sensor_pose_errors(scene["renderer"], scene["camera"], T_est, scene["T_gt"], list(scene["occluded"]),
                                     scene["depth_scale"], d)
    fig = SE.sensor_frame_figures(got, 1.0, n_taus=10, finite_slot=10)
    for key in ("vsd", "visib_fract", "n_vis_est", "n_vis_gt", "n_inter", "n_union", "n_sil_gt", "mean_abs_dd", "max_abs_dd"):
        np.testing.assert_array_equal(res[key], fig[key])
    assert res["shift"] == (0, 0) and res["residual_px"] == 0.0 and res["ok"].all()
    # the visible fraction: the share of the ground truth's silhouette that the slab leaves uncovered
    uncovered = (scene["on"] & ~scene["slab"]).sum(axis=(1, 2)) / scene["on"].sum(axis=(1, 2))
    print("visib_fract", res["visib_fract"], "uncovered", uncovered, "vsd", res["vsd"].mean(axis=0))
    np.testing.assert_array_equal(res["visib_fract"], uncovered)
    assert ((uncovered > 0.4) & (uncovered < 0.9)).all()
    free = ME.mesh_sensor_pose_errors(scene["renderer"], scene["camera"], scene["T_gt"], scene["T_gt"].copy(),
                                      list(scene["free"]), scene["depth_scale"], d)
    assert (free["visib_fract"] == 1.0).all() and (free["vsd"] == 0.0).all()
    with pytest.raises(ValueError, match="uint16"):
        ME.mesh_sensor_pose_errors(scene["renderer"], scene["camera"], T_est, scene["T_gt"],
                                   [im.astype(np.int32) for im in scene["occluded"]], scene["depth_scale"], d)


# ------------------------------------------------------------------------------------- the command line, mesh against NeRF
NW, NH, NF = 160, 120, 6


@pytest.fixture(scope="module")
def extracted(device, tmp_path_factory):
    """The synthetic object on disk, its mesh extracted at 24^3 in the sfm frame by the command line (with
    --check_render 4), and a six-frame poses.pkl: ground truth, estimates a degree and 1 % of the diameter off, one
    frame lost."""
    from pixtrack_amd.symmetry import read_models_info
    from pixtrack_amd.synthetic import make_tracking_assets, perturb_pose, write_object_dir
    from pixtrack_amd.utils.io import dump_reference_pickle

    tmp = tmp_path_factory.mktemp("mesh_eval")
    assets = make_tracking_assets(width=NW, height=NH, n_frames=NF)
    obj, out = tmp / "object", tmp / "model"
    write_object_dir(assets, obj)
    aabb = json.dumps([[float(x) for x in corner] for corner in assets["aabb"]])
    summary = M.main(["--object_path", str(obj), "--obj_aabb", aabb, "--resolution", "24", "--out_dir", str(out),
                      "--device", str(device), "--check_render", "4"])
    info = read_models_info(out / "models_info.json")
    cam = Camera.from_colmap(assets["query_camera"])
    rng = np.random.default_rng(0)
    poses, names = {}, [f"{k:06d}.png" for k in range(NF)]
    for name, (Rg, tg) in zip(names, assets["gt_poses"]):
        Re, te = perturb_pose(Rg, tg, rng, 1.0, 0.01 * info["diameter"], assets["center"])
        poses[name] = {"success": True, "camera": cam, "gt_pose": Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg)),
                       "T_refined": Pose.from_Rt(torch.from_numpy(Re), torch.from_numpy(te))}
    poses[names[3]]["success"] = False
    dump_reference_pickle(poses, str(tmp / "poses.pkl"))
    return dict(tmp=tmp, obj=obj, out=out, aabb=aabb, summary=summary, info=info, assets=assets, names=names, poses=poses,
                camera=cam)


def test_command_line_has_render_evaluations_keys(device, extracted, capsys):
    from PIL import Image

    tmp, names = extracted["tmp"], extracted["names"]
    capsys.readouterr()
    RE.main(["--poses", str(tmp / "poses.pkl"), "--object_path", str(extracted["obj"]), "--obj_aabb", extracted["aabb"],
             "--device", str(device)])
    before = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    common = ["--poses", str(tmp / "poses.pkl"), "--mesh", str(extracted["out"] / "mesh.obj"), "--device", str(device)]
    res = ME.main(common + ["--models_info", str(extracted["out"] / "models_info.json"), "--json", str(tmp / "out.json")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(line)
    assert set(line) == set(before) and "frames" not in line
    assert line["n_frames"] == NF and line["n_success"] == NF - 1 and line["n_evaluated"] == NF - 1
    assert line["diameter"] == extracted["info"]["diameter"] and len(line["vsd_mean"]) == 10 == len(line["taus"])
    assert 0 < line["ar_vsd"] <= (NF - 1) / NF and 0.7 < line["iou_mean"] < 1 and 0 < line["mean_abs_dz_mean"] < 0.05 * line["diameter"]
    lost = res["frames"][names[3]]
    assert lost["vsd"] == [1.0] * 10 and lost["iou"] == 0.0 and not lost["ok"]
    saved = json.loads((tmp / "out.json").read_text())
    assert set(saved["frames"]) == set(names) and set(saved["frames"][names[0]]) == set(res["frames"][names[0]])
    # the diameter a run is not given: the mesh's largest vertex distance, what mesh.py wrote into models_info.json
    ME.main(common)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["diameter"] == pytest.approx(line["diameter"], rel=1e-6)
    # a PLY of the same mesh in millimetres scores the same
    V, F = R.read_mesh(extracted["out"] / "mesh.obj")
    M.write_ply(tmp / "mesh_mm.ply", V * 1000.0, F)
    ME.main(["--poses", str(tmp / "poses.pkl"), "--mesh", str(tmp / "mesh_mm.ply"), "--mesh_scale", "0.001", "--device",
             str(device), "--diameter", str(line["diameter"])])
    mm = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # (vertices rounded twice on the way: a pixel may change hands, and with it at most a couple of the NF x 10 x 10 tests)
    assert mm["ar_vsd"] == pytest.approx(line["ar_vsd"], abs=2.0 / (NF * 100)) and mm["iou_mean"] == pytest.approx(line["iou_mean"], abs=2e-3)
    # --bop and the sensor images: the keys of sensor_evaluation beside them
    views = np.stack([R.view_record(extracted["camera"], RE._poses_4x4([extracted["poses"][k]["gt_pose"]])[0], ME.DEFAULT_NEAR)
                      for k in names])
    gt = R.rasterize_reference(V, F, views, NW, NH)[0]
    on = gt[..., 3] == 1.0
    z = np.where(on, gt[..., 0].astype(np.float64), 0.0)
    depth_scale = float(z.max() / 20000)
    counts = np.where(on, np.rint(z / depth_scale), 60000).astype(np.uint16)
    (tmp / "depth").mkdir()
    for name, img in zip(names, counts):
        Image.fromarray(img).save(tmp / "depth" / (name[:-4] + "-depth.png"))
    ME.main(common + ["--diameter", str(line["diameter"]), "--bop", "--sensor_depth_dir", str(tmp / "depth"),
                      "--sensor_depth_template", "{stem}-depth.png", "--sensor_depth_scale", str(depth_scale)])
    full = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for key in ("vsd_sensor_mean", "visib_fract_mean", "n_below_visibility", "ar_vsd_sensor", "ar_mssd", "ar_mspd", "ar_bop",
                "ar_bop_sensor", "sensor_shift", "sensor_residual_px"):
        assert key in full, key
    assert {k: full[k] for k in line} == line and full["visib_fract_mean"] == 1.0 and full["sensor_shift"] == [0, 0]
    assert 0 < full["ar_vsd_sensor"] <= (NF - 1) / NF


def test_mesh_against_its_nerf(device, extracted, capsys):
    from pixtrack_amd.utils.ingp_utils import initialize_ingp

    check = extracted["summary"]["check_render"]
    print("24^3 by the command line:", check)
    assert check["n_views"] == 4 and 0 < check["iou_mean"] <= 1 and np.isfinite(check["mean_abs_dz_mean"])
    testbed = initialize_ingp(str(extracted["obj"] / "pixtrack/instant-ngp/snapshots/weights.msgpack"),
                              json.loads(extracted["aabb"]), device=str(device))
    mesh = M.extract_mesh(testbed, 32, colors=False)
    keep = (testbed.fov, np.array(testbed._cam_ngp))
    true = ME.mesh_nerf_agreement(testbed, mesh["V"], mesh["F"], n_views=4)
    turned = ME.mesh_nerf_agreement(testbed, mesh["V"], mesh["F"], n_views=4, turn_mesh_view_deg=20.0)
    print("32^3, four views: iou", true["iou"], "mean |dz| (ngp units)", true["mean_abs_dz"], "| turned by 20 deg: iou",
          turned["iou"], "mean |dz|", turned["mean_abs_dz"], "| silhouette pixels", true["n_mesh"], true["n_nerf"])
    assert true["n_views"] == 4 and true["iou"].shape == (4,) and np.isfinite(true["iou"]).all()
    assert np.isfinite(true["mean_abs_dz"]).all() and (true["n_mesh"] > 0).all() and (true["n_nerf"] > 0).all()
    assert true["iou_mean"] > turned["iou_mean"] and np.isfinite(turned["iou"]).all()
    assert testbed.fov == keep[0] and np.array_equal(testbed._cam_ngp, keep[1])  # the testbed's own view is put back
