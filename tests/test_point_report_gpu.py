"""pxt_lm_point_report (csrc/pxt_lm_report.hip) against the float64 oracle (oracle/lm_oracle.py: residual_jacobian +
make_loss), against the project's own kernels (pxt_lm_information, the LM's log), and against itself (determinism).

Cases and bars
  SCENES below are those of tests/test_pose_uncertainty_gpu.py (same make_lm_scene arguments and seeds, chosen there so
  that no point lies within 1e-3 px of the padded border; the margin is re-checked at every pose evaluated here), at
  level 0 (C = 32: 8-lane groups) and level 2 (C = 128: 32-lane groups), plus "tiny": the first 37 points of the qvga
  scene - less than one workgroup round, a ragged tail.  The initial pose and the LM's refined pose (cropped: the
  initial pose only, as there); the three loss kinds on the first scene.
  `valid` and the reject code must be EQUAL point by point, the integer summary words equal.  Words 3..6 are compared
  over the valid points as |d| / |ref| vector norms, (u, v) as the largest absolute difference in pixels, summary words
  0, 3 and 4 as relative errors of the oracle's sums.  The bar of a quantity is 4x the worst figure the float32 oracle
  shows against the float64 oracle on exactly these cases (`python tests/test_point_report_gpu.py`, no GPU needed; the
  margin the information tests take for a differing operation order), measured:
      uv 4.58e-5 px   cost |r|^2 1.60e-4   rho 1.60e-4   rho' 1.33e-5   w_unc 4.84e-7
      sum rho 1.01e-5   sum rho' w_unc 1.40e-6   sum w_unc 2.19e-7
  (cost and rho: the masked scene at its refined pose, level 0, where the residuals are small differences of nearly equal
  descriptors; sum rho: the 37-point problem at its refined pose.)
  (F32_ORACLE_WORST below).  The inlier threshold of a case is the first of 0.5, 0.5003, 0.5006, ... that no valid
  point's float64 rho' comes within 1e-4 of; the test asserts that distance.
"""
import ctypes as C
import sys
from pathlib import Path

if __name__ == "__main__":  # (run as a script: the repository root is not on the path yet)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import pytest
import torch

import camera_cases as CC
from oracle import lm_oracle as O
from pixtrack_amd import _lib
from pixtrack_amd.geometry import Pose
from pixtrack_amd.ops import ops
from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for
from pixtrack_amd.point_report import decode_points, decode_summary
from pixtrack_amd.synthetic import make_lm_scene

pytestmark = pytest.mark.gpu

# measured on the CPU by this file's __main__ (float32 oracle vs float64 oracle, the worst case per quantity)
F32_ORACLE_WORST = {"uv": 4.58e-5, "cost": 1.60e-4, "rho": 1.60e-4, "robust_weight": 1.33e-5, "confidence": 4.84e-7,
                    "sum_rho": 1.01e-5, "sum_w": 1.40e-6, "sum_conf": 2.19e-7}
BARS = {k: 4 * v for k, v in F32_ORACLE_WORST.items()}
# the k2_limit scene (a camera half as long, distortion factors up to 1.4) exceeds two of them in the float32 oracle
# itself: its own constants, measured the same way (level 0, initial pose)
F32_ORACLE_WORST_K2_LIMIT = {"uv": 7.27e-5, "confidence": 6.09e-7}
BARS_BY_SCENE = {"k2_limit": {**BARS, **{k: 4 * v for k, v in F32_ORACLE_WORST_K2_LIMIT.items()}}}

# name -> make_lm_scene arguments (+ "mask_seed": a point mask keeping ~85 % of the points; "first": only that many
# points of the scene)
SCENES = {
    "qvga": dict(seed=1301, width=320, height=240, n_points=2048),
    "radial": dict(seed=1303, width=320, height=240, n_points=1500, k1=-0.08, sigma_px=2.0),
    "masked": dict(seed=1304, width=320, height=240, n_points=2048, mask_seed=4),
    "cropped": dict(seed=1305, width=320, height=240, n_points=2048, fill=1.5),
    "tiny": dict(seed=1301, width=320, height=240, n_points=2048, first=37),
    # the camera table (tests/camera_cases.py): OPENCV (every record must match with p1, p2 in the projection) and a range
    # limit of the k2 > 0 branch inside an overfilled image, where rep_projectable - a hand copy of project_point's range
    # test - must tell "outside the model's range" (2) from "outside the image" (3) point by point
    "opencv": dict(seed=1303, width=320, height=240, n_points=1500, sigma_px=2.0, **CC.SCENE_KW["opencv"]),
    "k2_limit": dict(seed=1305, width=320, height=240, n_points=2048, **CC.SCENE_KW["k2_limit"]),
}
# scene -> at least this many points with reject code 2 that lie in front of the camera and project inside the image, and
# at least this many with code 3
BOTH_REJECTS = {"k2_limit": (20, 40)}
LEAVES_THE_VIEW = {"cropped": (0.255, 0.43)}  # scene -> the share of points with reject code 3 lies in this range (26.1 % at
# level 0, 42.5 % at level 2 in the float64 oracle)
LOSSES = {"squared": (0, 2.0, 1.0), "huber": (1, 0.0, 0.1), "barron": (2, 0.0, 0.1)}
LEVELS = (0, 2)
PAD = 1
ORACLE_POSES = {"cropped": ("init",), "k2_limit": ("init",)}  # (where the LM's refined pose puts that scene's border points is the device's business)
CASES = [(s, l, p, "barron") for s in SCENES for l in LEVELS for p in ORACLE_POSES.get(s, ("init", "refined"))] + \
        [("qvga", l, "init", k) for l in LEVELS for k in ("squared", "huber")]


def build_scene(name):
    kw = dict(SCENES[name])
    mask_seed, first = kw.pop("mask_seed", None), kw.pop("first", None)
    sc = make_lm_scene(**kw)
    mask = None
    if mask_seed is not None:
        mask = (np.random.default_rng(mask_seed).uniform(size=sc.p3d.shape[0]) > 0.15).astype(np.uint8)
    return sc, mask, first


def pack_level(scene, level, first=None):
    fq = scene.feats_query[level]
    Cc = fq.shape[0] - 1
    cs = cstride_for(Cc)
    h, w = fq.shape[1:]
    fmap = torch.zeros(h, w, cs)
    fmap[..., :Cc] = O.l2_normalize(fq[:-1], dim=0).permute(1, 2, 0)
    fmap[..., Cc] = fq[-1]
    fr = scene.feats_ref[level]
    fref = torch.zeros(fr.shape[0], cs)
    fref[:, :Cc] = O.l2_normalize(fr[:, :-1], dim=1)
    fref[:, Cc] = fr[:, -1]
    return fmap, fref[:first].contiguous(), Cc, scene.camera.scale(scene.scales[level])


def oracle_points(fmap, fref, Cc, cam, p3d, pose12, loss, mask, dtype, pad=PAD):
    """The report's per-point words and sums from the oracle in `dtype`, plus the border margin of the nearest point."""
    kind, alpha, scale = loss
    name = {0: "squared", 1: "huber", 2: "barron"}[kind]
    loss_fn = O.make_loss(name) if kind == 0 else O.make_loss(name, alpha, scale)
    chw = fmap[..., :Cc + 1].permute(2, 0, 1).contiguous().to(dtype)
    fr = fref.to(dtype)
    cam_t = cam._data.to(dtype)
    pose = torch.as_tensor(np.asarray(pose12, np.float64)).to(dtype)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    pts = torch.as_tensor(np.asarray(p3d)).to(dtype)
    res, valid, w_unc, _J = O.residual_jacobian(R, t, cam_t, pts, fr[:, :Cc], chw[:Cc], fr[:, Cc:Cc + 1], chw[Cc:Cc + 1], pad)
    kept = torch.ones_like(valid) if mask is None else torch.as_tensor(np.asarray(mask)).bool()
    in_window = valid  # visible (in front, inside the distortion range, inside the image) & mask_in_image
    valid = valid & kept
    cost = (res ** 2).sum(-1)
    rho, wl = loss_fn(cost)
    pc = O.pose_transform(R, t, pts)
    p2d, _ = O.world2image(cam_t, pc)
    in_front = pc[..., -1] > O.CAM_EPS
    _, in_range = O._undistort(pc[..., :-1] / pc[..., -1:].clamp(min=O.CAM_EPS), cam_t[6:])
    # the split of the oracle's validity: mask, then `visible` without its image test, then the (padded) image
    reject = torch.where(~kept, 1, torch.where(~(in_front & in_range), 2, torch.where(~in_window, 3, 0)))
    h, w = chw.shape[1:]
    lim = torch.tensor([w - pad - 1, h - pad - 1], dtype=dtype)
    margin = torch.minimum((p2d - pad).abs().min(-1).values, (lim - p2d).abs().min(-1).values)
    v = valid.to(dtype)
    return {"valid": valid.numpy(), "reject": reject.numpy().astype(np.uint8), "in_front": in_front.numpy(),
            "uv": p2d.double().numpy(), "cost": cost.double().numpy(), "rho": rho.double().numpy(),
            "robust_weight": (wl * torch.ones_like(cost)).double().numpy(), "confidence": w_unc.double().numpy(),
            "sum_rho": float((v * rho).sum()), "sum_w": float((v * wl * w_unc).sum()), "sum_conf": float((v * w_unc).sum()),
            "margin": float(margin.min()), "r2_margin": float(CC.r2_margin(cam_t[6:], pc.double().numpy()).min())}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def compare(got, want):
    """-> {quantity: error} of a report-like dict against the float64 oracle, over the oracle's valid points."""
    v = want["valid"]
    out = {"uv": float(np.abs(got["uv"][v] - want["uv"][v]).max())}
    for k in ("cost", "rho", "robust_weight", "confidence"):
        out[k] = rel(got[k][v], want[k][v])
    for k in ("sum_rho", "sum_w", "sum_conf"):
        out[k] = rel(got[k], want[k])
    return out


def pick_inlier_weight(robust_weight64, valid):
    """The first of 0.5, 0.5003, ... that no valid point's float64 rho' lies within 1e-4 of."""
    w = np.asarray(robust_weight64)[valid]
    for step in range(200):
        thr = 0.5 + 3e-4 * step
        if w.size == 0 or np.abs(w - thr).min() > 1e-4:
            return float(np.float32(thr))
    raise AssertionError("no inlier threshold with a 1e-4 margin")


def report_dict(points, summary):
    d = decode_points(points)
    s = np.asarray(summary, np.float64)
    return {"valid": d["valid"], "reject": d["reject"], "uv": d["p2d"].astype(np.float64), "cost": d["cost"].astype(np.float64),
            "rho": d["rho"].astype(np.float64), "robust_weight": d["robust_weight"].astype(np.float64),
            "confidence": d["confidence"].astype(np.float64), "sum_rho": s[0], "sum_w": s[3], "sum_conf": s[4]}


# ------------------------------------------------------------------------------------------------ device helpers
class Dev:
    def __init__(self, device):
        self.device = device
        self.ws, self.info_ws = {}, None
        self.lm_ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)

    def workspace(self, K):
        K = max(1, min(K, _lib.PXT_LM_REPORT_MAX_PROBLEMS))  # (the out-of-range cases bring a valid workspace)
        if K not in self.ws:
            self.ws[K] = torch.zeros(int(_lib.lib().pxt_lm_point_report_workspace_bytes(K)), dtype=torch.uint8,
                                     device=self.device)
        return self.ws[K]


def to_dev(device, fmap, fref, Cc, cam, p3d, mask):
    return {"fmap": fmap.to(device).contiguous(), "fref": fref.to(device).contiguous(), "C": Cc, "cam": cam,
            "p3d": torch.as_tensor(np.asarray(p3d)).float().to(device).contiguous(),
            "mask": None if mask is None else torch.as_tensor(mask).to(device)}


def _cams(problems):
    cams, ndist = [], []
    for p in problems:
        cams += [float(x) for x in p["cam"].as10().tolist()]
        ndist.append(int(p["cam"]._data.shape[-1] - 6))
    return cams, ndist


SENTINEL = -7.0


def report(dv, problems, poses, loss=LOSSES["barron"], inlier=0.5, want_points=True, summaries=None, points=None,
           is_record=False, min_valid=10, pad=PAD, workspace=None):
    """One launch -> (points tensors (None where not asked), summaries); both prefilled with SENTINEL."""
    K = len(problems)
    dev = dv.device
    if summaries is None:
        summaries = [torch.full((16,), SENTINEL, device=dev) for _ in range(K)]
    want = want_points if isinstance(want_points, (list, tuple)) else [want_points] * K
    if points is None:
        points = [torch.full((int(p["p3d"].shape[0]), 8), SENTINEL, device=dev) if w else None for p, w in zip(problems, want)]
    cams, ndist = _cams(problems)
    pose_t = [q if torch.is_tensor(q) else torch.as_tensor(np.asarray(q, np.float32)).to(dev) for q in poses]
    inl = list(inlier) if isinstance(inlier, (list, tuple)) else [float(inlier)] * K
    ops.lm_point_report([p["p3d"] for p in problems], [p["mask"] for p in problems], [p["fmap"] for p in problems],
                        [p["fref"] for p in problems], [p["C"] for p in problems], cams, ndist, pose_t, is_record, pad,
                        loss[0], loss[1], loss[2], min_valid, inl, points, summaries,
                        dv.workspace(K) if workspace is None else workspace)
    return points, summaries


def information(dv, problem, pose, loss):
    if dv.info_ws is None:
        dv.info_ws = torch.zeros(int(_lib.lib().pxt_lm_information_workspace_bytes(1)), dtype=torch.uint8, device=dv.device)
    rec = torch.zeros(48, device=dv.device)
    cams, ndist = _cams([problem])
    ops.lm_information([problem["p3d"]], [problem["mask"]], [problem["fmap"]], [problem["fref"]], [problem["C"]], cams, ndist,
                       [torch.as_tensor(np.asarray(pose, np.float32)).to(dv.device)], False, PAD, loss[0], loss[1], loss[2], 10,
                       [rec], dv.info_ws)
    return rec.cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def dv(device):
    return Dev(device)


@pytest.fixture(scope="module")
def scenes(device, dv):
    """Per scene: levels 0..2 on the host and the device, the initial pose and the LM kernel's refined pose."""
    out = {}
    for name in SCENES:
        sc, mask, first = build_scene(name)
        p3d = sc.p3d[:first]
        levels = [pack_level(sc, l, first) for l in range(3)]
        devl = [to_dev(device, *lv, p3d, mask) for lv in levels]
        init = np.concatenate([sc.R_init.reshape(-1), sc.t_init])
        opt = PixTrackOptimizer(dict(num_iters=100, pad=PAD))
        lam = torch.full((6,), 1e-2)
        packs = [LevelPack(devl[l]["fmap"], devl[l]["fref"], devl[l]["C"], levels[l][3], lam) for l in (2, 1, 0)]
        res = PixTrackOptimizer.refine_levels(devl[0]["p3d"], packs, Pose(torch.from_numpy(init).float()), opt.native_conf(),
                                              dv.lm_ws, mask=devl[0]["mask"]).result()
        assert not res.failed
        out[name] = {"p3d": p3d, "mask": mask, "levels": levels, "dev": devl, "init": init.astype(np.float32),
                     "refined": res.T.as12().numpy().astype(np.float32), "packs": packs}
    return out


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("scene,level,which,loss", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_report_matches_the_float64_oracle(dv, scenes, scene, level, which, loss):
    S = scenes[scene]
    fmap, fref, Cc, cam = S["levels"][level]
    pose = S[which]
    want = oracle_points(fmap, fref, Cc, cam, S["p3d"], pose, LOSSES[loss], S["mask"], torch.float64)
    assert want["margin"] > 1e-3, f"a point sits within 1e-3 px of the border ({want['margin']}): the seed is unfair"
    assert want["r2_margin"] > CC.R2_REL_MARGIN, f"a point sits at the range limit ({want['r2_margin']}): the seed is unfair"
    inlier = pick_inlier_weight(want["robust_weight"], want["valid"])
    assert np.abs(want["robust_weight"][want["valid"]] - inlier).min() > 1e-4
    N = S["p3d"].shape[0]
    n_valid = int(want["valid"].sum())
    assert n_valid >= (20 if scene == "tiny" else 500)
    if scene in LEAVES_THE_VIEW:
        lo, hi = LEAVES_THE_VIEW[scene]
        assert lo * N < int((want["reject"] == 3).sum()) < hi * N
    if scene in BOTH_REJECTS:
        n2, n3 = BOTH_REJECTS[scene]
        w_, h_ = fmap.shape[1], fmap.shape[0]
        in_image = (want["uv"] >= 0).all(1) & (want["uv"][:, 0] <= w_ - 1) & (want["uv"][:, 1] <= h_ - 1)
        beyond = want["in_front"] & (want["reject"] == 2)  # in front of the camera and outside the model's range
        print(scene, level, "code 2 in front", int(beyond.sum()), "of them inside the image", int((beyond & in_image).sum()),
              "code 3", int((want["reject"] == 3).sum()))
        assert int((beyond & in_image).sum()) >= n2 and int((want["reject"] == 3).sum()) >= n3
    pts, summ = report(dv, [S["dev"][level]], [pose], LOSSES[loss], inlier)
    pts, summ = pts[0].cpu().numpy(), summ[0].cpu().numpy()
    got = report_dict(pts, summ)
    errs = compare(got, want)
    print(scene, level, which, loss, "n_valid", int(summ[1]), n_valid, "inliers", int(summ[2]), "thr", inlier,
          {k: f"{v:.2e}" for k, v in errs.items()})
    assert summ[15] == 1.0 and np.all(summ[8:15] == 0.0)
    np.testing.assert_array_equal(got["valid"], want["valid"])
    np.testing.assert_array_equal(got["reject"], want["reject"])
    # invalid points: zeros in words 3..6; (u, v) is NaN exactly for the points behind the camera
    assert np.all(pts[~want["valid"], 3:7] == 0.0)
    np.testing.assert_array_equal(np.isnan(pts[:, 1:3]).any(1), ~want["in_front"])
    assert set(np.unique(pts[:, 0])) <= {0.0, 1.0}
    # the integer summary words
    assert int(summ[1]) == n_valid
    assert int(summ[2]) == int((want["robust_weight"][want["valid"]] >= inlier).sum())
    for code in (1, 2, 3):
        assert int(summ[4 + code]) == int((want["reject"] == code).sum()), code
    assert int(summ[1] + summ[5] + summ[6] + summ[7]) == N
    bars = BARS_BY_SCENE.get(scene, BARS)
    for k, v in errs.items():
        assert v <= bars[k], (k, v, bars[k])
    d = decode_summary(summ)
    assert d["n_valid_points"] == n_valid and d["inlier_ratio"] == summ[2] / summ[1]


def test_reject_code_two_behind_the_camera_and_outside_the_distortion_range(dv, scenes):
    """The scenes above keep every point in front of the camera: reject code 2 and the NaN (u, v) get a pose of their own
    (the camera turned half way round: every point behind it) and a camera whose distortion model has a limited range."""
    S = scenes["qvga"]
    fmap, fref, Cc, cam = S["levels"][0]
    flip = np.diag([-1.0, 1.0, -1.0])  # half a turn about the camera's y axis
    pose = np.concatenate([(flip @ S["init"][:9].reshape(3, 3).astype(np.float64)).reshape(-1),
                           flip @ S["init"][9:].astype(np.float64)]).astype(np.float32)
    want = oracle_points(fmap, fref, Cc, cam, S["p3d"], pose, LOSSES["barron"], None, torch.float64)
    assert not want["in_front"].any()
    pts, summ = report(dv, [S["dev"][0]], [pose])
    pts, summ = pts[0].cpu().numpy(), summ[0].cpu().numpy()
    N = S["p3d"].shape[0]
    assert summ[15] == -2.0 and summ[1] == 0 and summ[6] == N and summ[0] == 0
    assert np.isnan(pts[:, 1:3]).all() and np.all(pts[:, 7] == 2.0) and np.all(pts[:, [0, 3, 4, 5, 6]] == 0.0)
    assert decode_summary(summ)["inlier_ratio"] is None
    # k1 > 0: the model is monotone only for r^2 < 1 / (3 k1); with k1 = 40 that radius lies inside the image
    from pixtrack_amd.geometry import Camera

    data = cam._data.clone().double()
    cam2 = Camera(torch.cat([data[:6], torch.tensor([40.0, 0.0], dtype=data.dtype)]).to(cam._data.dtype))
    want = oracle_points(fmap, fref, Cc, cam2, S["p3d"], S["init"], LOSSES["barron"], None, torch.float64)
    n2 = int((want["reject"] == 2).sum())
    assert 0 < n2 < N and want["in_front"].all()
    pc = O.pose_transform(torch.from_numpy(S["init"][:9].reshape(3, 3)).double(), torch.from_numpy(S["init"][9:]).double(),
                          torch.from_numpy(np.asarray(S["p3d"])).double())
    r2 = ((pc[:, :2] / pc[:, 2:]) ** 2).sum(-1).numpy()
    assert np.abs(r2 - 1.0 / 120.0).min() > 1e-7  # (no point within float32's reach of the model's limit)
    pts, summ = report(dv, [dict(S["dev"][0], cam=cam2)], [S["init"]])
    pts, summ = pts[0].cpu().numpy(), summ[0].cpu().numpy()
    assert int(summ[6]) == n2
    np.testing.assert_array_equal((pts[:, 7] == 2.0), want["reject"] == 2)
    assert not np.isnan(pts[:, 1:3]).any()


# ------------------------------------------------------------------------------------------------ 2. the project's kernels
@pytest.mark.parametrize("scene", list(SCENES))
def test_report_agrees_with_the_information_record_and_the_lm_log(dv, scenes, scene):
    S = scenes[scene]
    opt = PixTrackOptimizer(dict(num_iters=1, pad=PAD))
    conf = opt.native_conf()
    loss = (conf.loss, conf.loss_alpha, conf.loss_scale)
    lam = torch.full((6,), 1e-2)
    for level in LEVELS:
        d = S["dev"][level]
        for which in ("init", "refined"):
            pose = S[which]
            pts, summ = report(dv, [d], [pose], loss)
            pts, summ = pts[0].cpu().numpy().astype(np.float64), summ[0].cpu().numpy().astype(np.float64)
            rec = information(dv, d, pose, loss)
            pack = LevelPack(d["fmap"], d["fref"], d["C"], d["cam"], lam)
            res = PixTrackOptimizer.refine_levels(d["p3d"], [pack], Pose(torch.from_numpy(pose)), conf, dv.lm_ws,
                                                  mask=d["mask"]).result()
            k0, k1 = float(res.log[0, 0, 0]), float(res.log[0, 0, 1])
            print(scene, level, which, "n_valid", summ[1], rec[1], k1, "sum rho", summ[0], rec[0], "mean", summ[0] / summ[1], k0)
            assert summ[1] == rec[1] == k1 == pts[:, 0].sum()
            assert abs(summ[0] - rec[0]) <= BARS["sum_rho"] * abs(rec[0])
            assert abs(summ[0] / summ[1] - k0) <= BARS["sum_rho"] * abs(k0)
            assert abs(pts[:, 4].sum() - summ[0]) <= BARS["sum_rho"] * abs(summ[0])


# ------------------------------------------------------------------------------------------------ 3. determinism
def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def test_bit_identical_across_launches_batches_streams_and_neighbours(dv, scenes, device):
    names = ["qvga", "radial", "masked", "cropped", "tiny"]
    probs = [scenes[n]["dev"][0 if i % 2 == 0 else 2] for i, n in enumerate(names)]
    poses = [scenes[n]["init" if i < 3 else ("init" if n == "cropped" else "refined")] for i, n in enumerate(names)]
    solo = [report(dv, [p], [q]) for p, q in zip(probs, poses)]
    solo = [(_bits(p[0]), _bits(s[0])) for p, s in solo]
    for (p, s) in solo:
        assert s[15].view(torch.float32) in (1.0, -2.0) and not bool((p.view(torch.float32)[:, 0] == SENTINEL).any())
    # the same launch again
    for (p, s), prob, pose in zip(solo, probs, poses):
        p2, s2 = report(dv, [prob], [pose])
        assert torch.equal(_bits(p2[0]), p) and torch.equal(_bits(s2[0]), s)
    # inside a batch of 5 (parameter records from the workspace, not the kernel arguments), in shuffled order
    perm = [3, 0, 4, 2, 1]
    pb, sb = report(dv, [probs[i] for i in perm], [poses[i] for i in perm])
    for j, i in enumerate(perm):
        assert torch.equal(_bits(pb[j]), solo[i][0]) and torch.equal(_bits(sb[j]), solo[i][1]), i
    # a batch of 2 (kernel arguments), the neighbour without a points buffer
    pb, sb = report(dv, [probs[1], probs[0]], [poses[1], poses[0]], want_points=[False, True])
    assert pb[0] is None
    assert torch.equal(_bits(sb[0]), solo[1][1]) and torch.equal(_bits(sb[1]), solo[0][1]) and torch.equal(_bits(pb[1]), solo[0][0])
    pb, sb = report(dv, [probs[i] for i in perm], [poses[i] for i in perm], want_points=[True, False, True, False, False])
    for j, i in enumerate(perm):
        assert torch.equal(_bits(sb[j]), solo[i][1])
        assert pb[j] is None or torch.equal(_bits(pb[j]), solo[i][0])
    # on another stream
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        pb, sb = report(dv, [probs[2], probs[4], probs[1]], [poses[2], poses[4], poses[1]])
    side.synchronize()
    for j, i in enumerate((2, 4, 1)):
        assert torch.equal(_bits(pb[j]), solo[i][0]) and torch.equal(_bits(sb[j]), solo[i][1])


# ------------------------------------------------------------------------------------------------ 4. pose from the LM record
def test_pose_read_from_the_lm_record_on_the_device(dv, scenes, device):
    S = scenes["qvga"]
    d = S["dev"][0]
    opt = PixTrackOptimizer(dict(num_iters=100, pad=PAD))
    conf = opt.native_conf()
    loss = (conf.loss, conf.loss_alpha, conf.loss_scale)
    pending = PixTrackOptimizer.refine_levels(d["p3d"], S["packs"], Pose(torch.from_numpy(S["init"])), conf, dv.lm_ws, mask=None)
    summ = torch.zeros(16).pin_memory()
    pts, _ = report(dv, [d], [pending.buf], loss, summaries=[summ], is_record=True)
    res = pending.result()  # (no synchronisation between the two launches)
    torch.cuda.synchronize(device)
    assert summ[15] == 1.0 and not res.failed
    again_p, again_s = report(dv, [d], [res.T.as12().numpy()], loss)
    assert torch.equal(_bits(again_p[0]), _bits(pts[0]))
    assert torch.equal(_bits(again_s[0]), summ.view(torch.int32))
    # the optimizer-level entry: the same bits through PixTrackOptimizer.point_report_levels
    pending = PixTrackOptimizer.refine_levels(d["p3d"], S["packs"], Pose(torch.from_numpy(S["init"])), conf, dv.lm_ws, mask=None)
    handle = PixTrackOptimizer.point_report_levels([{"p3d": d["p3d"], "mask": None, "pack": S["packs"][-1], "pose": pending,
                                                     "points": True}], conf, dv.workspace(1), pool_key="test")
    pending.result()
    out = handle.result()[0]
    np.testing.assert_array_equal(out.astype(np.float32).view(np.uint32), summ.numpy().view(np.uint32))
    assert torch.equal(_bits(handle.points[0]), _bits(pts[0]))
    # a refinement that reports `failed` (a point mask keeping fewer than min_valid points): skipped, nothing else written
    few = torch.zeros(d["p3d"].shape[0], dtype=torch.uint8, device=device)
    few[:5] = 1
    pending = PixTrackOptimizer.refine_levels(d["p3d"], S["packs"], Pose(torch.from_numpy(S["init"])), conf, dv.lm_ws, mask=few)
    summ2 = torch.full((16,), 123.0).pin_memory()
    summ2[15] = 0.0
    pts2, _ = report(dv, [dict(d, mask=few)], [pending.buf], loss, summaries=[summ2], is_record=True)
    res = pending.result()
    torch.cuda.synchronize(device)
    assert res.failed
    assert summ2[15] == -1.0 and bool((summ2[:15] == 123.0).all())
    assert bool((pts2[0] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_invalid_arguments_raise(dv, scenes, device):
    S = scenes["qvga"]
    d = S["dev"][2]
    pose = torch.from_numpy(S["init"]).to(device)
    with pytest.raises(_lib.PxtError):  # no problem
        ops.lm_point_report([], [], [], [], [], [], [], [], False, 1, 2, 0.0, 0.1, 10, [], [], [], dv.workspace(1))
    with pytest.raises(_lib.PxtError):  # too many problems
        report(dv, [d] * 65, [pose] * 65, want_points=False)
    with pytest.raises(_lib.PxtError):  # a host-memory map
        report(dv, [dict(d, fmap=d["fmap"].cpu())], [pose])
    with pytest.raises(_lib.PxtError):  # a points tensor of the wrong shape
        report(dv, [d], [pose], points=[torch.zeros(d["p3d"].shape[0], 7, device=device)])
    with pytest.raises(_lib.PxtError):  # a workspace that is too small
        report(dv, [d] * 5, [pose] * 5, want_points=False, workspace=dv.workspace(1))
    L = _lib.lib()
    q = (_lib.LmReportProblem * 2)()
    out = torch.zeros(2, 16, device=device)
    pts = torch.zeros(2, d["p3d"].shape[0], 8, device=device)
    for k in range(2):
        q[k].p3d, q[k].point_mask, q[k].n_points = d["p3d"].data_ptr(), None, d["p3d"].shape[0]
        h, w, cs = d["fmap"].shape
        q[k].level.fmap, q[k].level.fref = d["fmap"].data_ptr(), d["fref"].data_ptr()
        q[k].level.h, q[k].level.w, q[k].level.C, q[k].level.cstride = h, w, d["C"], cs
        q[k].level.cam[:] = [float(x) for x in d["cam"].as10().tolist()]
        q[k].level.ndist = int(d["cam"]._data.shape[-1] - 6)
        q[k].pose, q[k].pose_is_lm_record, q[k].inlier_weight = pose.data_ptr(), 0, 0.5
        q[k].points, q[k].summary = pts[k].data_ptr(), out[k].data_ptr()
    conf = _lib.LmConf()
    conf.pad, conf.loss, conf.loss_scale, conf.min_valid = 1, 2, 0.1, 10
    ws = dv.workspace(2)
    s = _lib.stream_ptr(device)

    def call(K=2, c=conf, w=ws):
        return L.pxt_lm_point_report(q, K, C.byref(c) if c is not None else None, w.data_ptr() if w is not None else None, s)

    assert call() == 0
    assert call(K=0) == -1 and call(K=-2) == -1 and call(K=_lib.PXT_LM_REPORT_MAX_PROBLEMS + 1) == -1
    assert call(c=None) == -1 and call(w=None) == -1
    keep = q[1].summary
    q[1].summary = None  # a null summary
    assert call() == -1
    q[1].summary = q[0].summary  # two problems, one summary
    assert call() == -1
    q[1].summary = keep
    q[1].points = q[0].points  # two problems, one points buffer
    assert call() == -1
    q[1].points = pts[1].data_ptr() + 4  # misaligned points
    assert call() == -1
    q[1].points = None  # summary only: fine
    assert call() == 0
    q[1].pose = pose.data_ptr() + 4  # misaligned pose
    assert call() == -1
    q[1].pose = pose.data_ptr()
    q[1].level.cstride = cs + 2  # misaligned cstride
    assert call() == -1
    q[1].level.cstride = cs
    assert call() == 0
    assert int(L.pxt_lm_point_report_workspace_bytes(0)) < 0 and int(L.pxt_lm_point_report_workspace_bytes(65)) < 0
    torch.cuda.synchronize(device)
    assert bool((out[:, 15] == 1.0).all())


# ------------------------------------------------------------------------------------------------ CPU calibration
if __name__ == "__main__":
    # float32 oracle vs float64 oracle on the cases above (the refined pose: the float32 oracle's own refinement), and
    # the validity / reject-code agreement of the seeds.  No GPU.
    worst = {}
    for name in SCENES:
        sc, mask, first = build_scene(name)
        p3d = sc.p3d[:first]
        levels = [pack_level(sc, l, first) for l in range(3)]
        conf = O.LMConf(num_iters=100, pad=PAD)
        fq = [torch.cat([lv[0][..., :lv[2]], lv[0][..., lv[2]:lv[2] + 1]], -1).permute(2, 0, 1) for lv in levels]
        fr = [lv[1][:, :lv[2] + 1] for lv in levels]
        ret = O.refine_pose_using_features(fq, sc.scales, sc.camera._data, torch.from_numpy(sc.R_init), torch.from_numpy(sc.t_init),
                                           fr, torch.from_numpy(p3d), [torch.full((6,), 1e-2)] * 3, conf,
                                           mask=None if mask is None else torch.from_numpy(mask).bool())
        assert ret["success"]
        poses = {"init": np.concatenate([sc.R_init.reshape(-1), sc.t_init]).astype(np.float32),
                 "refined": np.concatenate([ret["R"].numpy().reshape(-1), ret["t"].numpy()]).astype(np.float32)}
        for level in LEVELS:
            fmap, fref, Cc, cam = levels[level]
            for which, pose in poses.items():
                if which not in ORACLE_POSES.get(name, ("init", "refined")):
                    continue
                for lname in (LOSSES if (name == "qvga" and which == "init") else ("barron",)):
                    a = oracle_points(fmap, fref, Cc, cam, p3d, pose, LOSSES[lname], mask, torch.float32)
                    b = oracle_points(fmap, fref, Cc, cam, p3d, pose, LOSSES[lname], mask, torch.float64)
                    errs = compare(a, b)
                    same = bool((a["valid"] == b["valid"]).all() and (a["reject"] == b["reject"]).all())
                    thr = pick_inlier_weight(b["robust_weight"], b["valid"])
                    for k, v in errs.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    print(f"{name:7s} L{level} {which:7s} {lname:7s} n {int(a['valid'].sum()):5d}/{int(b['valid'].sum()):5d} "
                          f"codes {np.bincount(b['reject'], minlength=4).tolist()} same {same} margin {b['margin']:.4f} "
                          f"r2 margin {b['r2_margin']:.1e} thr {thr:.4f} "
                          + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print("worst float32-vs-float64 figures:", {k: f"{v:.2e}" for k, v in worst.items()})
