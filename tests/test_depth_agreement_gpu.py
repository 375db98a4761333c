"""pxt_depth_agreement (csrc/pxt_eval_render.hip) / torch.ops.pixtrack.depth_agreement and the mesh-free evaluation on top
of it (pixtrack_amd/render_evaluation.py): P pairs of Depth images compared pixel by pixel in one call.

Oracle: render_evaluation.depth_agreement_reference, a numpy float32 restatement of the per-pixel rules.  Division,
subtraction and comparison are IEEE operations on both sides and the counts are integers, so every word but the float sum
is compared BIT FOR BIT, with no tolerance and no pixel left out.

The float sum (word 4) depends on the order of the additions.  Bar (the project's convention): the
largest relative error, against the float64 sum of the same float32 terms, of a plain float32 pairwise sum (np.sum) over
the very inputs of test 1; the kernel may be 4 x that off.
Measured (seeded inputs below, 10 shapes x 17 pairs): restatement max 1.217e-07 -> bar 4.867e-07; the kernel on an MI355X
9.770e-08.  Both figures are printed before the assertion (pytest -s).

What a synthetic six-frame r9 run scores (160 x 120, diameter 1.81; printed, nothing absolute is asserted): tracked
vsd_mean 0.0076 at every tau, iou_mean 0.992, ar_vsd 1.0; the same poses perturbed by 10 degrees and 5 % of the diameter
vsd_mean 0.43 ... 0.115, iou_mean 0.885, ar_vsd 0.63."""
import ctypes

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, ops
from pixtrack_amd import render_evaluation as RE

pytestmark = pytest.mark.gpu

SHARE = 1024  # pixels of one workgroup (csrc/pxt_eval_render.hip: 256 lanes x 4)
# one pixel, odd sizes, one wave exactly, a partial wave over rows, rows longer than a wavefront's load, many blocks;
# one pixel below / exactly at / one pixel above one workgroup's share; three blocks with a one-pixel tail
SHAPES = ((1, 1), (7, 5), (64, 1), (63, 3), (257, 3), (160, 120), (SHARE - 1, 1), (SHARE, 1), (SHARE + 1, 1),
          (2 * SHARE + 1, 1))
PAIRS = (1, 3, 17)
NTAUS = (1, 10, 16)
PMAX = max(PAIRS)
MIN_ALPHA = 0.5
TQ = [0.25 * (k + 1) for k in range(16)]  # quarter-integers, like most of the dq values: many dq == tq exactly
SENTINEL = -777
EXACT_WORDS = [0, 1, 2, 3, 5, 6, 7] + list(range(8, 24))


def _inputs(W, H, seed):
    """PMAX seeded pairs: two overlapping discs offset from each other; inside a disc alpha is drawn from {0, 0.25, 0.5,
    0.75, 1} and channel 0 from the quarter-integers of [-1, 6] (0 and negatives included), outside both are 0; the two
    middle channels hold noise; one pixel of every pair has an infinite estimated depth."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.45 * max(W, H) + 0.5
    out = []
    for shift in (-0.2, 0.2):
        cx, cy = (W - 1) / 2 + shift * max(W, H), (H - 1) / 2
        disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        img = rng.normal(size=(PMAX, H, W, 4)).astype(np.float32)
        img[..., 3] = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], np.float32), size=(PMAX, H, W)) * disc
        img[..., 0] = rng.integers(-4, 25, size=(PMAX, H, W)).astype(np.float32) * np.float32(0.25) * disc
        out.append(img)
    est, gt = out
    iy, ix = (H - 1) // 2, (W - 1) // 2  # inside both discs
    est[:, iy, ix, 0], est[:, iy, ix, 3] = np.inf, 1.0
    gt[:, iy, ix, 0], gt[:, iy, ix, 3] = 1.0, 1.0
    return est, gt


def _terms(est, gt):
    """The float32 terms of pair sums: dq where both are visible and dq is finite, else 0 ([P, H * W])."""
    with np.errstate(all="ignore"):
        vis = [(a[..., 3] >= np.float32(MIN_ALPHA)) & (a[..., 0] > 0) for a in (est, gt)]
        dq = np.abs(est[..., 0] / est[..., 3] - gt[..., 0] / gt[..., 3])
    keep = vis[0] & vis[1] & np.isfinite(dq)
    return np.where(keep, dq, np.float32(0)).reshape(len(est), -1)


@pytest.fixture(scope="module")
def refs(device):
    """Per shape: the inputs on the host and on the device, the oracle's records and float64 sums for PMAX pairs and 16
    thresholds (a pair's record does not depend on the other pairs; fewer thresholds are a prefix); and the bar."""
    out, worst = {}, 0.0
    for n, (W, H) in enumerate(SHAPES):
        est, gt = _inputs(W, H, 300 + n)
        rec, sums = RE.depth_agreement_reference(est, gt, MIN_ALPHA, TQ)
        terms = _terms(est, gt)
        assert terms.dtype == np.float32 and np.array_equal(terms.astype(np.float64).sum(axis=1), sums)
        pairwise = np.array([np.sum(t) for t in terms], np.float64)  # float32 pairwise sums
        have = sums > 0
        if have.any():
            worst = max(worst, float((np.abs(pairwise[have] - sums[have]) / sums[have]).max()))
        assert (rec[:, 2] >= 1).all()  # (the inf pixel at least)
        out[(W, H)] = dict(est=est, gt=gt, rec=rec, sums=sums, d_est=torch.from_numpy(est).to(device),
                           d_gt=torch.from_numpy(gt).to(device))
    out["restatement"] = worst
    out["bar"] = 4.0 * worst
    print(f"float32 pairwise restatement: max relative error {worst:.3e}; bar {4 * worst:.3e}")
    assert out["bar"] < 1e-5  # a float32 sum of a few thousand terms
    return out


def _run(device, d_est, d_gt, tq, records=None, min_alpha=MIN_ALPHA):
    """One call of the op; -> the records (uint32 [P, 24], host)."""
    P, H, W = (int(x) for x in d_est.shape[:3])
    if records is None:
        records = torch.full((P, 24), SENTINEL, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_depth_agreement_workspace_bytes(P, W, H)), dtype=torch.uint8, device=device)
    ops.ops.depth_agreement(d_est, d_gt, min_alpha, tq, records, ws)
    return records.cpu().numpy().view(np.uint32)


def _want(rec, P, n_taus):
    w = rec[:P].copy()
    w[:, 6] = n_taus
    w[:, 8 + n_taus:] = 0
    return w


# ------------------------------------------------------------------------------------------------ 1. exact records
@pytest.mark.parametrize("n_taus", NTAUS)
@pytest.mark.parametrize("P", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_equal_the_restatement_bit_for_bit(device, refs, shape, P, n_taus):
    r = refs[shape]
    got = _run(device, r["d_est"][:P], r["d_gt"][:P], TQ[:n_taus])
    want = _want(r["rec"], P, n_taus)
    np.testing.assert_array_equal(got[:, EXACT_WORDS], want[:, EXACT_WORDS])
    assert (got[:, 2] <= np.minimum(got[:, 0], got[:, 1])).all()
    assert (np.diff(got[:, 8:8 + n_taus].astype(np.int64), axis=1) >= 0).all()  # nested thresholds
    assert (got[:, 8 + n_taus - 1] < got[:, 2]).all()  # the inf pixel is within none


# ------------------------------------------------------------------------------------------------ 2. the float sum
def test_the_float_sum_stays_within_four_pairwise_errors(device, refs):
    worst = 0.0
    for shape in SHAPES:
        r = refs[shape]
        got = _run(device, r["d_est"], r["d_gt"], TQ)[:, 4].copy().view(np.float32).astype(np.float64)
        have = r["sums"] > 0
        assert (got[~have] == 0.0).all()
        if have.any():
            err = float((np.abs(got[have] - r["sums"][have]) / r["sums"][have]).max())
            print(f"{shape}: kernel sum max relative error {err:.3e}")
            worst = max(worst, err)
    print(f"kernel sum: max relative error {worst:.3e}; float32 pairwise restatement {refs['restatement']:.3e}; "
          f"bar {refs['bar']:.3e}")
    assert worst <= refs["bar"], (worst, refs["bar"])


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("shape", ((160, 120), (2 * SHARE + 1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_record_depends_on_its_own_pair_only(device, refs, shape):
    r = refs[shape]
    base = _run(device, r["d_est"], r["d_gt"], TQ)
    np.testing.assert_array_equal(base[:, EXACT_WORDS], r["rec"][:, EXACT_WORDS])
    perm = np.random.default_rng(9).permutation(PMAX)
    idx = torch.from_numpy(perm).to(device)
    np.testing.assert_array_equal(_run(device, r["d_est"][idx].contiguous(), r["d_gt"][idx].contiguous(), TQ), base[perm])
    for k in range(PMAX):
        np.testing.assert_array_equal(_run(device, r["d_est"][k:k + 1], r["d_gt"][k:k + 1], TQ), base[k:k + 1])
    outs = [torch.full((PMAX, 24), SENTINEL, dtype=torch.int32, device=device) for _ in range(10)]
    ws = torch.empty(int(_lib.lib().pxt_depth_agreement_workspace_bytes(PMAX, *shape)), dtype=torch.uint8, device=device)
    for o in outs:
        ops.ops.depth_agreement(r["d_est"], r["d_gt"], MIN_ALPHA, TQ, o, ws)
    torch.cuda.synchronize(device)
    for o in outs:
        np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), base)
    # one tensor on both sides: every visible pixel agrees with itself (the inf pixel: inf - inf is a NaN)
    same = _run(device, r["d_est"], r["d_est"], TQ)
    assert (same[:, 0] == same[:, 1]).all() and (same[:, 1] == same[:, 2]).all() and (same[:, 2] == same[:, 3]).all()
    assert (same[:, 4:6] == 0).all() and (same[:, 8:] == same[:, 2:3] - 1).all()


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_bad_arguments_are_refused_and_nothing_is_written(device, refs):
    r = refs[(63, 3)]
    L = _lib.lib()
    est, gt = r["d_est"][:3], r["d_gt"][:3]
    rec = torch.full((3, 24), SENTINEL, dtype=torch.int32, device=device)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=device)
    tq = (ctypes.c_float * 17)(*([0.5] * 17))
    s = _lib.stream_ptr(device)
    a = (est.data_ptr(), gt.data_ptr(), 3, 63, 3, MIN_ALPHA, tq, 10, rec.data_ptr(), ws.data_ptr(), s)

    def call(**kw):
        args = list(a)
        for i, val in kw.items():
            args[int(i[1:])] = val
        return L.pxt_depth_agreement(*args)

    cases = (dict(_7=0), dict(_7=17), dict(_2=0), dict(_3=0), dict(_0=est.data_ptr() + 4),  # the issue's five
             dict(_2=65536), dict(_4=0), dict(_3=1 << 15, _4=(1 << 13) + 1), dict(_1=gt.data_ptr() + 8), dict(_0=None),
             dict(_1=None), dict(_6=None), dict(_8=None), dict(_9=None), dict(_8=rec.data_ptr() + 2), dict(_7=-1))
    for kw in cases:
        assert call(**kw) == -1, kw  # PXT_E_ARG
        with pytest.raises(_lib.PxtError):
            _lib.check(call(**kw), "pxt_depth_agreement")
    torch.cuda.synchronize(device)
    assert (rec.cpu() == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(rec.cpu().numpy().view(np.uint32), _run(device, est, gt, [0.5] * 10))
    # through the op
    rec.fill_(SENTINEL)
    bad = (lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, [], rec, ws),
           lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, [0.5] * 17, rec, ws),
           lambda: ops.ops.depth_agreement(est[:0], gt[:0], MIN_ALPHA, TQ, rec[:0], ws),
           lambda: ops.ops.depth_agreement(est, gt[:2], MIN_ALPHA, TQ, rec, ws),
           lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, TQ, rec[:2], ws),
           lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, TQ, rec.float(), ws),
           lambda: ops.ops.depth_agreement(est[..., :3], gt[..., :3], MIN_ALPHA, TQ, rec, ws),
           lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, TQ, rec, ws[:3 * 96 - 1]),
           lambda: ops.ops.depth_agreement(est, gt, MIN_ALPHA, TQ, rec, ws.cpu()))
    for f in bad:
        with pytest.raises(_lib.PxtError):
            f()
    torch.cuda.synchronize(device)
    assert (rec.cpu() == SENTINEL).all()


def test_the_host_wrapper_is_the_raw_op(device, refs):
    r = refs[(257, 3)]
    got = RE.depth_agreement(r["est"], r["gt"], TQ[:10], MIN_ALPHA, device)
    np.testing.assert_array_equal(got, _run(device, r["d_est"], r["d_gt"], TQ[:10]))
    np.testing.assert_array_equal(RE.depth_agreement(r["d_est"][0], r["d_gt"][0], TQ[:10], MIN_ALPHA, device), got[:1])
    fig = RE.frame_figures(got, 1.0)
    ref = RE.frame_figures(_want(r["rec"], PMAX, 10), 1.0, sums=r["sums"])
    np.testing.assert_array_equal(fig["vsd"], ref["vsd"])
    np.testing.assert_array_equal(fig["iou"], ref["iou"])
    np.testing.assert_allclose(fig["mean_abs_dz"], ref["mean_abs_dz"], rtol=refs["bar"])


# ------------------------------------------------------------------------------------------------ 5. real renders
W, H, N = 160, 120, 6


@pytest.fixture(scope="module")
def run(device):
    """Built once: synthetic assets, an r9 tracker over them, its six-frame run with ground truth attached, the query
    camera, the diameter (the diagonal of the SfM points' box) and the Depth renders at the ground-truth poses."""
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    assets = make_tracking_assets(width=W, height=H, n_frames=N)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
    frames = render_query_frames(assets, tr.testbed)
    names = [f"{i:06d}.png" for i in range(N)]
    for name, frame in zip(names, frames):
        tr.run_single_frame((name, frame))
    torch.cuda.synchronize(device)
    T_gt = np.tile(np.eye(4), (N, 1, 1))
    for k, (name, (Rg, tg)) in enumerate(zip(names, assets["gt_poses"])):
        tr.pose_history[name]["gt_pose"] = Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg))
        T_gt[k, :3, :3], T_gt[k, :3, 3] = Rg, tg
    camera = Camera.from_colmap(assets["query_camera"])
    diameter = RE.bounding_box_diagonal(assets["model3d"])
    return dict(assets=assets, tr=tr, names=names, T_gt=T_gt, camera=camera, diameter=diameter,
                gt_images=_renders(tr, camera, T_gt, device))


def _renders(tr, camera, T, device):
    out = torch.empty(len(T), H, W, 4, dtype=torch.float32, device=device)
    for k in range(len(T)):
        RE._render_depth(tr.testbed, tr.nerf2sfm, T[k], camera, 8, out[k])
    return out


def _perturbed(run, rot_deg, trans, seed=21):
    from pixtrack_amd.synthetic import perturb_pose

    rng = np.random.default_rng(seed)
    T = run["T_gt"].copy()
    for k in range(N):
        T[k, :3, :3], T[k, :3, 3] = perturb_pose(T[k, :3, :3], T[k, :3, 3], rng, rot_deg, trans, run["assets"]["center"])
    return T


def test_a_pose_agrees_with_itself_exactly(device, run):
    tr, d = run["tr"], run["diameter"]
    again = _renders(tr, run["camera"], run["T_gt"], device)
    zs = RE.z_scale(tr.testbed, tr.nerf2sfm)
    taus, tq = RE._thresholds(d, None, zs)
    rec = _run(device, again, run["gt_images"], tq)
    print("n_est", rec[:, 0], "of", W * H)
    assert (rec[:, 0] > 0).all() and (rec[:, 0] == rec[:, 1]).all() and (rec[:, 1] == rec[:, 2]).all()
    assert (rec[:, 3] == rec[:, 2]).all() and (rec[:, 8:8 + 11] == rec[:, 2:3]).all()
    assert (rec[:, 4] == 0).all() and (rec[:, 5] == 0).all()  # +0.0, not -0.0
    res = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], run["T_gt"], run["T_gt"].copy(), d)
    assert (res["vsd"] == 0.0).all() and (res["iou"] == 1.0).all() and res["ok"].all() and res["vsd"].shape == (N, 10)
    assert (res["mean_abs_dz"] == 0.0).all() and (res["max_abs_dz"] == 0.0).all()
    np.testing.assert_array_equal(res["n_est"], rec[:, 0])
    np.testing.assert_array_equal(res["taus"], taus)


def test_render_records_equal_the_restatement(device, run):
    tr, d = run["tr"], run["diameter"]
    T_est = _perturbed(run, 3.0, 0.02 * d)
    est = _renders(tr, run["camera"], T_est, device)
    zs = RE.z_scale(tr.testbed, tr.nerf2sfm)
    taus, tq = RE._thresholds(d, None, zs)
    got = _run(device, est, run["gt_images"], tq)
    want, sums = RE.depth_agreement_reference(est.cpu().numpy(), run["gt_images"].cpu().numpy(), MIN_ALPHA, tq)
    np.testing.assert_array_equal(got[:, EXACT_WORDS], want[:, EXACT_WORDS])
    res = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], T_est, run["T_gt"], d)
    fig = RE.frame_figures(got, zs, n_taus=10, finite_slot=10)
    for key in ("vsd", "iou", "n_est", "n_gt", "mean_abs_dz", "max_abs_dz"):
        np.testing.assert_array_equal(res[key], fig[key])
    print("3 deg / 2 % of the diameter: vsd", res["vsd"].mean(axis=0), "iou", res["iou"], "mean |dz|", res["mean_abs_dz"],
          "diameter", d)
    assert (np.diff(res["vsd"], axis=1) <= 0).all()  # non-increasing in tau
    assert (res["iou"] < 1).all() and (res["iou"] > 0).all()
    # a non-finite pose is not rendered: a miss, and only that frame
    bad = T_est.copy()
    bad[2, 0, 3] = np.nan
    res2 = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, [run["camera"]] * N, bad, run["T_gt"], d)
    assert not res2["ok"][2] and (res2["vsd"][2] == 1).all() and res2["iou"][2] == 0
    keep = [0, 1, 3, 4, 5]
    np.testing.assert_array_equal(res2["vsd"][keep], res["vsd"][keep])


def test_a_sideways_shift_by_one_diameter_shows(device, run):
    tr, d = run["tr"], run["diameter"]
    shifted = run["T_gt"].copy()
    shifted[:, 0, 3] += d  # along the camera's x axis
    same = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], run["T_gt"], run["T_gt"], d)
    off = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], run["T_gt"], shifted, d)
    print("shifted by one diameter: iou", off["iou"], "vsd[-1]", off["vsd"][:, -1])
    assert (off["iou"] < same["iou"]).all() and (off["vsd"][:, -1] > same["vsd"][:, -1]).all()
    assert (np.diff(off["vsd"], axis=1) <= 0).all()


def test_a_tracked_run_scores_better_than_its_perturbation(device, run):
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.synthetic import perturb_pose

    tr, d, names = run["tr"], run["diameter"], run["names"]
    res = RE.evaluate_poses_rendered(tr.pose_history, tr.testbed, tr.nerf2sfm, d)
    assert res["n_frames"] == N and res["n_evaluated"] == N and res["n_success"] == N and res["diameter"] == d
    assert len(res["vsd_mean"]) == 10 and len(res["taus"]) == 10 and all(res["frames"][n]["ok"] for n in names)
    rng = np.random.default_rng(22)
    worse = {}
    for n in names:
        R, t = tr.pose_history[n]["T_refined"].numpy()
        Rp, tp = perturb_pose(np.asarray(R, np.float64), np.asarray(t, np.float64), rng, 10.0, 0.05 * d, run["assets"]["center"])
        worse[n] = dict(tr.pose_history[n], T_refined=Pose.from_Rt(torch.from_numpy(Rp), torch.from_numpy(tp)))
    worse[names[3]] = dict(worse[names[3]], success=False)  # and one lost frame
    res_w = RE.evaluate_poses_rendered(worse, tr.testbed, tr.nerf2sfm, d)
    print("tracked:   vsd_mean", res["vsd_mean"], "iou_mean", res["iou_mean"], "mean |dz|", res["mean_abs_dz_mean"],
          "ar_vsd", res["ar_vsd"])
    print("perturbed: vsd_mean", res_w["vsd_mean"], "iou_mean", res_w["iou_mean"], "mean |dz|", res_w["mean_abs_dz_mean"],
          "ar_vsd", res_w["ar_vsd"])
    assert (np.array(res["vsd_mean"]) < np.array(res_w["vsd_mean"])).all()
    assert res_w["n_evaluated"] == N - 1 and res_w["n_success"] == N - 1 and res_w["n_frames"] == N
    lost = res_w["frames"][names[3]]
    assert not lost["ok"] and lost["vsd"] == [1.0] * 10 and lost["iou"] == 0.0
    assert res["ar_vsd"] >= res_w["ar_vsd"]


def test_the_command_line_needs_no_vertex_file(device, run, tmp_path, capsys):
    import json

    from pixtrack_amd.synthetic import write_object_dir
    from pixtrack_amd.utils.io import dump_reference_pickle

    obj = tmp_path / "object"
    write_object_dir(run["assets"], obj)
    dump_reference_pickle(run["tr"].pose_history, str(tmp_path / "poses.pkl"))
    aabb = [[float(x) for x in c] for c in run["assets"]["aabb"]]
    res = RE.main(["--poses", str(tmp_path / "poses.pkl"), "--object_path", str(obj), "--obj_aabb", json.dumps(aabb),
                   "--json", str(tmp_path / "out.json"), "--device", str(device)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(line)
    assert line["n_frames"] == N and line["n_evaluated"] == N and "frames" not in line
    assert line["diameter"] == pytest.approx(run["diameter"], rel=1e-6) and len(line["vsd_mean"]) == 10
    assert 0 <= line["ar_vsd"] <= 1 and 0 < line["iou_mean"] <= 1
    saved = json.loads((tmp_path / "out.json").read_text())
    assert set(saved["frames"]) == set(run["names"]) and saved["n_evaluated"] == res["n_evaluated"]
