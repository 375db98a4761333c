"""PixLocPoseTrackerR9 with a mesh template (mesh_template.MeshTemplate): the frame's two images against
mesh_render.frame_reference bit for bit, tracking of the synthetic mesh object against ground truth at the project's bar
for synthetic sequences (2e-2 rad / 2e-2 units, test_tracker_gpu.py), the assets and history surface, the untouched
default and the command line."""
import numpy as np
import pytest
import torch

from pixtrack_amd import mesh_render as R
from pixtrack_amd.geometry import Camera as PixCamera, Pose
from pixtrack_amd.mesh_template import MeshTemplate
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_mesh_tracking_assets, make_tracking_assets, render_mesh_query_frames, render_query_frames
from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

pytestmark = pytest.mark.gpu

N_FRAMES = 6
TRACKER_KEYS = ("model3d", "weights", "covis", "upright_ref_img")


def run(tr, frames):
    states = []
    for i, f in enumerate(frames):
        tr.run_single_frame((f"{i:06d}.png", f))
        states.append((tr.pose.numpy(), tr.success))
    return states


@pytest.fixture(scope="module")
def tracked(device, tmp_path_factory):
    out = tmp_path_factory.mktemp("mesh_object")
    assets = make_mesh_tracking_assets(seed=1031, width=128, height=96, n_frames=N_FRAMES, out_dir=out, device=device)
    V, F = assets["mesh"][:2]
    template = MeshTemplate(R.MeshRenderer(V, F, device, **assets["mesh_shading"]), supersample=2)
    frames = render_mesh_query_frames(assets, template.renderer)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=1, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                             template=template)
    return assets, tr, frames, run(tr, frames)


def frame_planes(tr, pose):
    """What the template draws at ``pose`` and what the tracker makes of it."""
    nz, ref_u8 = tr.template.frame(pose, tr.camera, tr._reference_camera())
    mask, ref_again = tr._mask_and_reference(pose, from_slot=False)
    torch.cuda.synchronize(tr.device)
    assert torch.equal(ref_u8, ref_again) and torch.equal(mask, tr._mask_of(nz))
    assert tr._own.pose is pose and tr._own.ref_u8 is ref_again
    tr._own = None
    return nz.cpu().numpy(), ref_u8.cpu().numpy()


def test_the_frames_two_images_are_the_reference_renders_bit_for_bit(tracked):
    assets, tr, frames, states = tracked
    V, F = assets["mesh"][:2]
    pose = Pose.from_Rt(*assets["gt_poses"][3])
    qcam, rcam = tr.camera, tr._reference_camera()
    q = tr.template.depth_q(pose)
    vq, vr = R.view_record(qcam, pose, tr.template.near, q), R.view_record(rcam, pose, tr.template.near, q)
    size = lambda cam: tuple(int(round(float(x))) for x in cam.size.tolist())
    assert size(qcam) == (128, 96) and size(rcam) == (128, 96) and rcam is not qcam
    # S = 2: two views
    assert tr.template.supersample == 2 and len(tr.template.requests(pose, qcam, rcam)) == 2
    want = R.frame_reference(V, F, assets["mesh_shading"], [(vq, 128, 96, 1, ("depth_nz",)), (vr, 128, 96, 2, ("rgb_u8", "rgba"))])
    nz, ref_u8 = frame_planes(tr, pose)
    assert np.array_equal(nz, want[0]["depth_nz"]) and np.array_equal(ref_u8, want[1]["rgb_u8"])
    alpha = want[1]["rgba"][..., 3]
    assert 0.03 < nz.mean() < 0.9 and ((alpha > 0) & (alpha < 1)).sum() > 100 and ref_u8.max() > 150
    # S = 1 and two cameras that agree (camera 1 x reference_scale is the query camera here): one view with both outputs
    saved = tr.template.supersample, tr._ref_cam_cache
    try:
        tr.template.supersample = 1
        requests = tr.template.requests(pose, qcam, rcam)
        assert len(requests) == 1 and requests[0][3] == 1 and set(requests[0][4]) == {"depth_nz", "rgb_u8"}
        nz1, ref1 = frame_planes(tr, pose)
        one = R.frame_reference(V, F, assets["mesh_shading"], [(vq, 128, 96, 1, ("depth_nz", "rgb_u8"))])[0]
        assert np.array_equal(nz1, one["depth_nz"]) and np.array_equal(ref1, one["rgb_u8"]) and np.array_equal(nz1, nz)
        # S = 1 and cameras that differ (for this check the reference camera is camera 1 x 0.375): two views again
        other = PixCamera.from_colmap(tr.localizer.model3d.cameras[1]).scale(0.375)
        tr._ref_cam_cache = (float(tr.reference_scale), other)
        assert tr._reference_camera() is other and len(tr.template.requests(pose, qcam, other)) == 2
        nz1, ref1 = frame_planes(tr, pose)
        vo = R.view_record(other, pose, tr.template.near, q)
        two = R.frame_reference(V, F, assets["mesh_shading"], [(vo, 96, 72, 1, ("rgb_u8",))])[0]
        assert ref1.shape == (72, 96, 3) and np.array_equal(nz1, nz) and np.array_equal(ref1, two["rgb_u8"])
    finally:
        tr.template.supersample, tr._ref_cam_cache = saved


def test_tracking_follows_ground_truth(tracked):
    assets, tr, frames, states = tracked
    assert set(tr.pose_history) == {f"{i:06d}.png" for i in range(N_FRAMES)}
    for i, ((Rt, t), ok) in enumerate(states):
        Rg, tg = assets["gt_poses"][i]
        r_err, t_err = geodesic_distance_for_rotations(Rt, Rg), float(np.linalg.norm(t - tg))
        ret = tr.pose_history[f"{i:06d}.png"]
        print(f"frame {i}: tracked {ret['tracked']} cost {ret['cost']:.4f} r_err {r_err:.5f} rad t_err {t_err:.5f}")
        assert ok and ret["tracked"] and ret["success"]
        assert r_err < 2e-2 and t_err < 2e-2
    assert tr.misses == N_FRAMES - 1 and tr.relocalization_count == 1


def test_assets_history_and_the_opt_in_reports(tracked, device):
    assets, tr, frames, states = tracked
    assert tr.testbed is None and tr.nerf2sfm is None and tr.render_ahead is False
    assert not any(k in assets for k in ("snapshot", "nerf2sfm", "aabb"))
    for ret in tr.pose_history.values():
        assert ret["template"] == "mesh" and ret["template_supersample"] == 2
    plain_keys = set(tr.pose_history["000002.png"])
    V, F = assets["mesh"][:2]
    template = MeshTemplate(R.MeshRenderer(V, F, device, **assets["mesh_shading"]), supersample=2)
    tr2 = PixLocPoseTrackerR9("", "", "", "/tmp", debug=1, device=device, assets={k: assets[k] for k in TRACKER_KEYS},
                              template=template, uncertainty=True, point_report="summary")
    states2 = run(tr2, frames)
    for (p, ok), (p2, ok2) in zip(states, states2):
        assert ok == ok2 and np.array_equal(p[0], p2[0]) and np.array_equal(p[1], p2[1])
    ret = tr2.pose_history["000002.png"]
    assert plain_keys < set(ret) and {"pose_info", "pose_cov", "observability", "n_valid_points", "n_inliers",
                                      "inlier_ratio"} <= set(ret) - plain_keys
    assert ret["n_valid_points"] > 50 and np.isfinite(np.asarray(ret["pose_cov"])).all()


def test_the_default_template_is_untouched(device):
    assets = make_tracking_assets(seed=1011, width=128, height=96, n_frames=3, n_points=3000)
    runs = []
    for kw in ({}, {"template": "nerf"}):
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=1, device=device, assets=assets, **kw)
        tr.spp = 2
        frames = render_query_frames(assets, tr.testbed)
        states = run(tr, frames)
        assert tr.template is None and tr.testbed is not None and all(ok for _, ok in states)
        runs.append((states, tr.pose_history, tr.render_ahead))
    (a, ha, ra), (b, hb, rb) = runs
    assert ra == rb
    for (pa, _), (pb, _) in zip(a, b):
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    for name in ha:
        assert list(ha[name]) == list(hb[name]) and "template" not in ha[name]
        assert ha[name]["cost"] == hb[name]["cost"]


def write_textured_obj(path, V, F, UV, FUV, tex):
    from PIL import Image

    with open(path / "textured.obj", "w") as f:
        f.write("mtllib textured.mtl\nusemtl material_0\n")
        f.writelines("v %r %r %r\n" % tuple(map(float, v)) for v in V)
        f.writelines("vt %r %r\n" % tuple(map(float, uv)) for uv in UV)
        f.writelines("f %d/%d %d/%d %d/%d\n" % tuple(np.stack([t + 1, k + 1], 1).ravel()) for t, k in zip(F, FUV))
    (path / "textured.mtl").write_text("newmtl material_0\nmap_Kd texture_map.png\n")
    Image.fromarray(tex).save(str(path / "texture_map.png"))
    return path / "textured.obj"


def test_the_command_line_on_a_built_directory_and_the_mesh_file(tracked, tmp_path, monkeypatch, capsys):
    """--template mesh on the ref/ directory mesh_dataset's builder wrote plus the mesh file: no snapshot, no nerf2sfm.pkl,
    no $OBJ_AABB.  Poses equal the in-process run within 1e-3, as test_cli_on_disk_assets holds the NeRF path."""
    import pickle

    from PIL import Image

    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as cli

    assets, tr, frames, states = tracked
    obj, query, out = tmp_path / "obj", tmp_path / "query", tmp_path / "out"
    (obj / "pixtrack").mkdir(parents=True)
    query.mkdir()
    torch.save(assets["weights"], obj / "pixtrack" / "pixloc_megadepth.pt")
    mesh = write_textured_obj(tmp_path, *assets["mesh"])
    for i, fr in enumerate(frames):
        Image.fromarray(np.clip(np.rint(fr.cpu().numpy()), 0, 255).astype(np.uint8)).save(query / f"{i:06d}.png")
    for name in ("UPRIGHT_REF_IMG", "OBJ_AABB", "PIXTRACK_WEIGHTS"):
        monkeypatch.delenv(name, raising=False)
    cli.main(["--object_path", str(obj), "--query", str(query), "--out_dir", str(out), "--debug", "1", "--template", "mesh",
              "--mesh", str(mesh), "--reference_sfm", str(assets["reference_dir"]), "--upright_ref_img", assets["upright_ref_img"]])
    text = capsys.readouterr().out
    assert "Cache hits: 0, misses: %d" % (N_FRAMES - 1) in text and text.rstrip().endswith("Done")
    with open(out / "poses.pkl", "rb") as f:
        poses = pickle.load(f)
    assert len(poses) == N_FRAMES
    for i, key in enumerate(poses):
        assert str(key).endswith(f"{i:06d}.png") and poses[key]["tracked"] and poses[key]["template"] == "mesh"
        Rc, tc = poses[key]["T_refined"].numpy()
        R0, t0 = states[i][0]
        assert geodesic_distance_for_rotations(Rc, R0) < 1e-3 and np.linalg.norm(tc - t0) < 1e-3
