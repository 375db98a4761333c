"""Host side of the mesh-free pose evaluation (pixtrack_amd/render_evaluation.py): the numpy restatement of
pxt_depth_agreement's per-pixel rules, the figures made of its counts, z_scale, the command line - everything that needs
no GPU.  The kernel is tests/test_depth_agreement_gpu.py's."""
import numpy as np
import pytest

from pixtrack_amd import _lib, ops
from pixtrack_amd import render_evaluation as RE


def _image(pixels, shape):
    """[H, W, 4] float32 from (x, alpha) per pixel; the two middle channels hold values nothing may read."""
    a = np.array([[x, 7.0, -3.0, w] for x, w in pixels], np.float32)
    return a.reshape(shape[0], shape[1], 4)


def _f32(word):
    return float(np.array([word], np.uint32).view(np.float32)[0])


def _bits(value):
    return int(np.array([value], np.float32).view(np.uint32)[0])


def test_a_hand_worked_two_by_two_pair():
    # pixel 0: q 2 vs 1.5 -> dq 0.5 (not below 0.5, below 1)   pixel 1: q 1 / 0.5 = 2 vs 3 -> dq 1 (below neither)
    # pixel 2: est x == 0 (invisible), gt visible               pixel 3: est alpha < min_alpha, gt x < 0: neither
    est = _image([(2.0, 1.0), (1.0, 0.5), (0.0, 1.0), (1.0, 0.25)], (2, 2))
    gt = _image([(1.5, 1.0), (3.0, 1.0), (1.0, 1.0), (-1.0, 1.0)], (2, 2))
    rec, sums = RE.depth_agreement_reference(est, gt, 0.5, [0.5, 1.0])
    assert rec.dtype == np.uint32 and rec.shape == (1, 24) and sums.dtype == np.float64 and sums.shape == (1,)
    want = [2, 3, 2, 3, _bits(1.5), _bits(1.0), 2, 1, 0, 1] + [0] * 14
    assert rec[0].tolist() == want
    assert sums[0] == 1.5
    # a batch of two pairs, the second one the first with est and gt swapped: the counts swap, the rest stays
    rec2, sums2 = RE.depth_agreement_reference(np.stack([est, gt]), np.stack([gt, est]), 0.5, [0.5, 1.0])
    assert rec2[0].tolist() == want
    assert rec2[1].tolist() == [3, 2, 2, 3, _bits(1.5), _bits(1.0), 2, 1, 0, 1] + [0] * 14
    assert sums2.tolist() == [1.5, 1.5]


def test_the_threshold_is_strict():
    est, gt = _image([(1.25, 1.0)], (1, 1)), _image([(1.0, 1.0)], (1, 1))
    tq = [np.nextafter(np.float32(0.25), np.float32(0)), 0.25, np.nextafter(np.float32(0.25), np.float32(1))]
    rec, _ = RE.depth_agreement_reference(est, gt, 0.5, tq)
    assert rec[0, 8:11].tolist() == [0, 0, 1] and rec[0, 6] == 3
    assert _f32(rec[0, 4]) == 0.25 and _f32(rec[0, 5]) == 0.25


def test_visibility_rules():
    one = (1.0, 1.0)
    for pixel, visible in (((1.0, 0.5), True), ((1.0, np.nextafter(np.float32(0.5), np.float32(0))), False),
                           ((0.0, 1.0), False), ((-1.0, 1.0), False), ((-0.0, 1.0), False),
                           ((1.0, np.nan), False), ((np.nan, 1.0), False), ((1e-30, 1.0), True)):
        rec, _ = RE.depth_agreement_reference(_image([pixel], (1, 1)), _image([one], (1, 1)), 0.5, [1e30])
        assert rec[0, 0] == int(visible) and rec[0, 1] == 1 and rec[0, 2] == int(visible) and rec[0, 3] == 1, pixel


def test_a_pixel_without_a_finite_difference():
    # inf vs 1: dq = inf; inf vs inf: dq = NaN.  Both count in n_both, neither is below any threshold (+inf included),
    # neither reaches the sum or the max; the third pixel is an ordinary one
    est = _image([(np.inf, 1.0), (np.inf, 1.0), (2.0, 1.0)], (1, 3))
    gt = _image([(1.0, 1.0), (np.inf, 1.0), (1.0, 1.0)], (1, 3))
    rec, sums = RE.depth_agreement_reference(est, gt, 0.5, [3.0, np.inf])
    assert rec[0, :4].tolist() == [3, 3, 3, 3]
    assert rec[0, 8:10].tolist() == [1, 1]
    assert _f32(rec[0, 4]) == 1.0 and _f32(rec[0, 5]) == 1.0 and sums[0] == 1.0
    fig = RE.frame_figures(rec, 2.0, n_taus=1, finite_slot=1, sums=sums)
    assert fig["mean_abs_dz"][0] == 2.0 and fig["max_abs_dz"][0] == 2.0  # one finite pixel, not three
    # nothing finite at all: +0.0 in both float words
    rec, _ = RE.depth_agreement_reference(est[:, :2], gt[:, :2], 0.5, [3.0])
    assert rec[0, 4] == 0 and rec[0, 5] == 0 and rec[0, 2] == 2 and rec[0, 8] == 0


def _record(n_est, n_gt, n_both, total, largest, within):
    r = np.zeros(24, np.uint32)
    r[:4] = n_est, n_gt, n_both, n_est + n_gt - n_both
    r[4], r[5], r[6], r[7] = _bits(total), _bits(largest), len(within), 1
    r[8:8 + len(within)] = within
    return r


def test_frame_figures_from_given_counts():
    rec = np.stack([_record(8, 6, 4, 3.0, 1.5, [1, 2, 4]), _record(0, 0, 0, 0.0, 0.0, [0, 0, 0]),
                    _record(5, 0, 0, 0.0, 0.0, [0, 0, 0])])
    fig = RE.frame_figures(rec, 0.5)
    np.testing.assert_array_equal(fig["n_union"], [10, 0, 5])
    np.testing.assert_allclose(fig["vsd"], [[0.9, 0.8, 0.6], [1, 1, 1], [1, 1, 1]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(fig["iou"], [0.4, 0.0, 0.0], rtol=0, atol=1e-15)
    assert fig["mean_abs_dz"][0] == 0.5 * 3.0 / 4 and fig["max_abs_dz"][0] == 0.75
    assert np.isnan(fig["mean_abs_dz"][1]) and fig["max_abs_dz"][1] == 0.0
    assert fig["ok"].all() and fig["n_est"].tolist() == [8, 0, 5] and fig["n_gt"].tolist() == [6, 0, 0]
    # the empty union is BOP's "not visible": vsd 1, iou 0 (exactly)
    assert (fig["vsd"][1] == 1.0).all() and fig["iou"][1] == 0.0


def test_average_recall_by_hand():
    # frame 0: vsd 0.0 is below all ten thetas, 0.32 below 0.35, 0.4, 0.45, 0.5; frame 1 is a miss -> 14 of 40
    vsd = np.array([[0.0, 0.32], [1.0, 1.0]])
    assert RE.average_recall(vsd) == pytest.approx(14 / 40, abs=1e-15)
    assert RE.average_recall(vsd, thetas=[0.3]) == 0.25
    assert RE.average_recall(np.array([[0.3]]), thetas=[0.3]) == 0.0  # strict
    assert np.isnan(RE.average_recall(np.zeros((0, 2))))


def test_lost_frames_are_misses_and_stay_out_of_the_means():
    vsd = np.array([[0.1, 0.0], [1.0, 1.0], [0.3, 0.2], [1.0, 1.0]])
    iou = np.array([0.9, 0.0, 0.7, 0.0])
    dz = np.array([0.01, np.nan, 0.03, np.nan])
    s = RE.summarize(vsd, iou, dz, [True, False, True, False], thetas=[0.25])
    assert s["n_evaluated"] == 2
    assert s["vsd_mean"] == pytest.approx([0.2, 0.1], abs=1e-15) and s["iou_mean"] == pytest.approx(0.8, abs=1e-15)
    assert s["mean_abs_dz_mean"] == pytest.approx(0.02, abs=1e-15)
    assert s["ar_vsd"] == pytest.approx(3 / 8, abs=1e-15)  # of 4 frames x 2 taus, frames 1 and 3 can never count
    none = RE.summarize(np.ones((2, 2)), np.zeros(2), np.full(2, np.nan), [False, False])
    assert none["n_evaluated"] == 0 and none["ar_vsd"] == 0.0 and np.isnan(none["iou_mean"]) and np.isnan(none["vsd_mean"]).all()


def _depth_to_camera_axis(nerf2sfm, scale, offset, R, t, q, dxn, dyn):
    """q of a Depth render's pixel pushed through the tracker's _depth_view xform (float64 throughout), and the
    camera-axis distance of that SfM point in the pose's camera frame."""
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.ngp import nerf_matrix_to_ngp, ngp_to_sfm_affine
    from pixtrack_amd.utils.ingp_utils import sfm_to_nerf_pose
    from pixtrack_amd.utils.pose_utils import get_camera_in_world_from_pixpose

    A = ngp_to_sfm_affine(nerf2sfm, scale, offset)
    cam = nerf_matrix_to_ngp(sfm_to_nerf_pose(nerf2sfm, get_camera_in_world_from_pixpose(Pose.from_Rt(R, t)))[:3, :], scale, offset)
    M, b = A[:, :3] @ cam[:, :3], A[:, :3] @ cam[:, 3] + A[:, 3]
    depth_scale = 1.0 / scale
    p = b + (q / depth_scale) * (M @ np.array([dxn, dyn, 1.0]))
    return float((R @ p + t)[2])


def test_z_scale_turns_render_depth_into_sfm_camera_depth():
    from pixtrack_amd.ngp import ngp_to_sfm_affine
    from pixtrack_amd.synthetic import make_tracking_assets

    assets = make_tracking_assets(width=160, height=120, n_frames=3, n_points=400)
    snap, nerf2sfm = assets["snapshot"], assets["nerf2sfm"]
    G = ngp_to_sfm_affine(nerf2sfm, float(snap.scale), float(snap.offset))[:, :3]
    norms = np.linalg.norm(G, axis=0)
    assert np.abs(norms - norms[0]).max() <= 1e-12 * norms[0]
    zs = RE.z_scale(snap, nerf2sfm)
    assert zs == pytest.approx(norms[0] * float(snap.scale), rel=1e-12)
    for (R, t), q, dxn, dyn in zip(assets["gt_poses"], (0.37, 1.21, 0.052), (0.0, 0.31, -0.22), (0.0, -0.17, 0.4)):
        z = _depth_to_camera_axis(nerf2sfm, float(snap.scale), float(snap.offset), R, t, q, dxn, dyn)
        assert z == pytest.approx(q * zs, rel=1e-9)

    # a similarity that is none of the identity's: random rotation, centroid and lengths
    class Snap:
        scale, offset = 0.33, 0.5

    rng = np.random.default_rng(3)
    qr, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Rn = np.eye(4)
    Rn[:3, :3] = qr * np.sign(np.linalg.det(qr))
    other = {"centroid": rng.normal(size=3), "avglen": 2.3, "totp": rng.normal(size=3), "R": Rn}
    zs = RE.z_scale(Snap, other)
    assert zs == pytest.approx(2.3 / 3.0, rel=1e-12)  # (1 / scale) * (avglen / 3) over depth_scale = 1 / scale
    R, t = assets["gt_poses"][0]
    z = _depth_to_camera_axis(other, Snap.scale, Snap.offset, R, t, 0.8, 0.21, -0.4)
    assert z == pytest.approx(0.8 * zs, rel=1e-9)
    # no similarity: one axis stretched
    bad = dict(other, R=Rn @ np.diag([1.0, 1.0, 1.0 + 1e-6, 1.0]))
    with pytest.raises(ValueError):
        RE.z_scale(Snap, bad)


def test_thresholds_are_divided_in_float64_and_rounded_once():
    taus, tq = RE._thresholds(0.2, None, 0.7)
    assert len(taus) == 10 and len(tq) == 11 and tq[-1] == np.inf
    np.testing.assert_allclose(taus, 0.2 * 0.05 * np.arange(1, 11), rtol=1e-15)
    assert tq[:10] == [float(np.float32(t / 0.7)) for t in taus]
    assert RE._thresholds(1.0, [0.1, 0.2], 1.0)[0] == [0.1, 0.2]
    with pytest.raises(ValueError):
        RE._thresholds(1.0, [0.1] * 16, 1.0)
    with pytest.raises(ValueError):
        RE._thresholds(1.0, [], 1.0)


def test_cli_arguments():
    a = RE.build_parser().parse_args(["--poses", "p.pkl", "--object_path", "obj"])
    assert (a.poses, a.object_path, a.obj_aabb, a.diameter, a.min_alpha, a.spp, a.json, a.device) == \
        ("p.pkl", "obj", "", None, 0.5, 8, None, "cuda:0")
    a = RE.build_parser().parse_args(["--poses", "p.pkl", "--object_path", "obj", "--obj_aabb", "[[0,0,0],[1,1,1]]",
                                      "--diameter", "0.3", "--min_alpha", "0.25", "--spp", "2", "--json", "out.json",
                                      "--device", "cuda:1"])
    assert (a.obj_aabb, a.diameter, a.min_alpha, a.spp, a.json, a.device) == \
        ("[[0,0,0],[1,1,1]]", 0.3, 0.25, 2, "out.json", "cuda:1")
    for argv in (["--poses", "p.pkl"], ["--object_path", "obj"]):
        with pytest.raises(SystemExit):
            RE.build_parser().parse_args(argv)
    with pytest.raises(_lib.PxtError):  # before any file is opened
        RE.main(["--poses", "missing.pkl", "--object_path", "missing", "--device", "cpu"])
    from pixtrack_amd.refiner import PoseTrackerRefiner  # (the default min_alpha is the reference points')

    assert RE.DEFAULT_MIN_ALPHA == PoseTrackerRefiner.default_config["reference_points_min_alpha"]


def test_host_tensors_raise_before_any_launch():
    import torch

    img = np.zeros((1, 2, 2, 4), np.float32)
    with pytest.raises(_lib.PxtError):
        RE.depth_agreement(img, img, [1.0], 0.5, "cpu")
    with pytest.raises(_lib.PxtError):
        RE.depth_agreement(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4), [1.0], 0.5, torch.device("cpu"))

    class Bed:
        device = torch.device("cpu")

    eye = np.eye(4)[None]
    with pytest.raises(_lib.PxtError):
        RE.render_pose_errors(Bed(), {}, None, eye, eye, 0.2)
    with pytest.raises(_lib.PxtError):
        RE.evaluate_poses_rendered({}, Bed(), {}, 0.2)
    with pytest.raises(_lib.PxtError):
        RE.evaluate_poses_rendered({}, Bed(), {}, 0.2, device="cpu")
    # the op's own body refuses host memory too (reached directly: the dispatcher has no CPU kernel to offer)
    with pytest.raises(_lib.PxtError):
        ops._depth_agreement(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4), 0.5, [1.0],
                             torch.zeros(1, 24, dtype=torch.int32), torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        torch.ops.pixtrack.depth_agreement(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4), 0.5, [1.0],
                                           torch.zeros(1, 24, dtype=torch.int32), torch.zeros(4096, dtype=torch.uint8))


def test_the_binding_and_the_op_are_there_and_the_abi_is_unchanged():
    import torch

    assert _lib.ABI_VERSION == 13
    L = _lib.lib()
    assert L.pxt_version() == 13 and not L._pxt_missing
    assert {"pxt_depth_agreement", "pxt_depth_agreement_workspace_bytes"} <= set(_lib.PROTOTYPES)
    assert (_lib.PXT_DEPTH_AGREE_RECORD, _lib.PXT_DEPTH_AGREE_MAX_TAUS) == (24, 16) == (RE.RECORD, RE.MAX_TAUS)
    assert "depth_agreement" in ops.op_names()
    s = str(torch.ops.pixtrack.depth_agreement.default._schema)
    assert "float[] tq" in s and "Tensor(a!) records" in s
    # one partial record (24 words) per 1024 pixels and pair
    wb = L.pxt_depth_agreement_workspace_bytes
    assert int(wb(1, 1, 1)) == 96 and int(wb(3, 160, 120)) == 3 * 19 * 96 and int(wb(2, 1025, 1)) == 2 * 2 * 96
    assert int(wb(65535, 1, 1)) == 65535 * 96 and int(wb(1, 1 << 14, 1 << 14)) == (1 << 18) * 96
    for P, W, H in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 14) + 1, 1 << 14), (1, -1, -1)):
        assert int(wb(P, W, H)) < 0, (P, W, H)
