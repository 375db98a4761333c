"""Every logged iteration of the persistent LM kernel (csrc/pxt_lm.hip) against a float64 replay of that one step.

tests/test_lm_gpu.py compares the FINAL pose with the oracle; LM corrects itself, so a step that is a few per cent wrong in
direction or length still contracts to the same fixed point.  Here nothing accumulates: the kernel logs, per iteration,
the mean cost, n_valid, dR, dt, |g|, the Cholesky flag and the pose after the step (LMResult.log[level, it]); each logged
step is replayed in float64 (oracle/lm_oracle.py: lm_step) from the pose the DEVICE started it at - the previous logged
pose, the previous level's last pose, or T_init in float32 - on the float32 inputs the kernel was given, widened.

What is compared, per logged iteration (replay())
  n_valid exactly; the mean cost relatively; |g| (see below); the Cholesky flag; the step d = (t' - Rd t, log_SO3(Rd))
  with Rd = R' R^T formed in float64 from the two logged float32 poses: |d_gpu - d_64| <= REL_STEP |d_64| + ABS; the
  logged dt against |d_64[:3]|; the logged dR through its cosine (a float32 acosf resolves no angle below 0.02 deg; the
  cosine does); the stop rule, exactly, in float32 on the kernel's own logged numbers; iteration counts and the final
  pose bits.  n_valid must be decidable: every replayed pose must keep every point at least 1e-3 px from the padded
  border ("unfair seed" otherwise).  No iteration is skipped.

Cases (CASES, BATCH)
  * each pyramid level alone from the perturbed pose, the stop thresholds 0 and num_iters = 6: six real steps, at least
    three of them of 1e-3 or more (asserted on the CPU and on the device), over the accumulation variants (point counts
    at, below and above every threshold of lm_refine_problem with 8 workgroups, each also with lm_path = 2), grids of 1,
    3, 8, 17 and 128 workgroups, 10 / 63 / 65 points, point masks, the three losses, k1 = -0.05, pads 0 and 1, the three
    lambda sets of CONSTS and one more, HEAVY.  The CONSTS sets damp with lambda = 2e-5 ... 9e-4: the step is the
    Gauss-Newton step to within float32 noise (a damping 5 % off moves it by 5e-5 of its length at most), and the 80x60
    level contracts 3e-1, 5e-3, 4e-4: two steps of 1e-3 or more, not three.  HEAVY (lambda = 0.014 ... 7) makes the
    damping shape the step and gives six steps between 1e-2 and 1e-3; every case on the 80x60 level uses it;
  * 1 and 9 points and a mask leaving 9: the masked identity step (failed, pose bits unchanged, iters [1, 0, 0]);
  * three-level runs with the default thresholds, pose carried from level to level, natural stops: one single launch and
    one refine_levels_batch of three unlike problems;
  * an object that overfills the image (fill = 1.5, pad 0): valid points whose 12-texel footprint reads zero-padded
    texels, ONE step per level at the initial pose (where a device trajectory puts border points the CPU cannot decide);
  * the camera table of tests/camera_cases.py: OPENCV (ndist 4: p1, p2 in the point and in the four distortion terms of
    the Jacobian) on every accumulation variant, the general path and lm_path = 2; PINHOLE (ndist 0) over three levels;
    and the k2 > 0 range limit inside an overfilled image, one step per level, both paths, 8 and 128 workgroups: the
    points inside the image and beyond the range (31 to 49 per level) must drop out of n_valid exactly.  The float32
    oracle stays below every constant of this file on them (__main__ asserts it; the worst new relative step is 1.1e-4,
    opencv-v2-n100 at its 1.2e-3 step, against 2.85e-4), so the constants stand as they were.  No replayed pose may hold a point nearer than relative 1e-5 (in
    r^2) to the range limit (FAIR_R2_MARGIN), as none may sit within 1e-3 px of the padded border.

Bars (measured by this file's __main__ on the CPU: the float32 oracle against the float64 oracle over the same cases, on
the float64 trajectory rounded to float32 after every step; the bar is 4x the worst value - another summation order
across lanes and workgroups - as in test_pose_uncertainty_gpu.py)
  worst relative error of the mean cost F32_COST; of the step where |d| >= 1e-3 F32_STEP_REL (that is where it is
  largest: 2.85e-4 at a step of 1.3e-3, 1.3e-4 at the steps of 0.3); worst absolute step error where |d| < 1e-3
  F32_STEP_ABS.  The relative error of a small step grows as it shrinks (g is a sum of cancelling terms), hence the two
  terms: REL_STEP alone bounds every float32-oracle step of 1e-3 or more with the factor 4, ABS_STEP alone every
  smaller one, and the device is given their sum.
  |g|: where |d| >= 1e-3 its relative error is at most F32_GNORM; over all steps it reaches 0.3 (the last steps of a
  converged level, |g| 1e-7 of its first value), which as a bar would hold nothing.  What the float32 error of g scales
  with is the size of the terms that cancel in it: every step's |g| is therefore also held to
  REL_GTERMS |sum_i |w_i J_i^T r_i||, F32_GTERMS being the worst such ratio of the float32 oracle.
  ABS also carries the rounding of the two float32 poses the device step is read back from: twelve entries, each off by
  at most 2^-24 of its magnitude.  |dR|_F <= 2^-24 |R|_F = sqrt(3) 2^-24 for either pose, so |d(Rd)|_F <= 2 sqrt(3) 2^-24
  and the rotation vector, vee(Rd - Rd^T) / 2 to first order, moves by at most |d(Rd)|_F / sqrt(2) = sqrt(6) 2^-24; the
  translation t' - Rd t moves by at most 2^-24 |t'| + |d(Rd)| |t| + 2^-24 |t| <= (2 + 2 sqrt(3)) 2^-24 |t|:
  pose_rounding(|t|) = 2^-24 sqrt(6 + (2 + 2 sqrt(3))^2 |t|^2), 3.6e-7 at |t| = 1.
  The cosine of dR: the kernel's (tr Rd - 1) / 2 carries three diagonal roundings (2^-25 each), two additions (2^-24,
  2^-23) and is halved: 1.125 * 2^-23; COS_ABS = 4 * 2^-24 covers it and acosf's own ulp, plus the step's own bar
  |w| (REL_STEP |w| + ABS) since d cos = -sin |w| d|w|.
"""
import functools
import math
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
from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for
from pixtrack_amd.synthetic import make_lm_scene

pytestmark = pytest.mark.gpu

# measured on the CPU by this file's __main__ (float32 oracle vs float64 oracle, worst over every step of every case)
F32_COST = 5.6e-6  # mean cost, relative (measured 5.52e-6: v3-n200, squared loss)
F32_GTERMS = 4.0e-5  # |g| against the norm of sum_i |w_i J_i^T r_i|, every step (3.94e-5: batch-2, the last step of level 0)
F32_GNORM = 1.75e-4  # |g|, relative, where |d| >= BIG_STEP (1.72e-4: n10)
F32_STEP_REL = 2.9e-4  # the step, relative, where |d| >= BIG_STEP (2.85e-4: v2-n128-edge, the 1.3e-3 step)
F32_STEP_ABS = 4.5e-7  # the step, absolute, where |d| < BIG_STEP (4.42e-7: v2-n128-edge, the 5e-7 step)
REL_COST, REL_GNORM, REL_STEP, ABS_STEP = 4 * F32_COST, 4 * F32_GNORM, 4 * F32_STEP_REL, 4 * F32_STEP_ABS
REL_GTERMS = 4 * F32_GTERMS
COS_ABS = 4 * 2.0 ** -24
BIG_STEP = 1e-3  # a step at or above this length is held by the relative term
FAIR_MARGIN = 1e-3  # px: no point of a replayed pose may sit nearer to the padded border
FAIR_R2_MARGIN = CC.R2_REL_MARGIN  # ... nor nearer (relative, in r^2) to the range limit of its distortion model


def pose_rounding(t_norm):
    return 2.0 ** -24 * math.sqrt(6.0 + (2.0 + 2.0 * math.sqrt(3.0)) ** 2 * t_norm ** 2)


CONSTS = [[-2.0] * 6, [-1.5, -2.5, -2.0, -1.8, -2.2, -2.0], [-2.0, -2.0, -1.0, -3.0, -2.0, -1.5]]  # per level, as test_lm_gpu
# lambda = 0.32, 0.014, 7.0, 0.048, 2.1, 0.32: a damping that shapes the step (the CONSTS sets give 2e-5 ... 9e-4, which
# moves a step by less than float32 noise) and slows the contraction, so that a level takes six steps of 1e-3 or more
HEAVY = [0.0, -0.5, 0.5, -0.3, 0.3, 0.0]
LOSSES = {"squared": ("squared_loss", ("squared", 0.0, 1.0)), "huber": ("scaled_huber(0.1)", ("huber", 0.0, 0.1)),
          "barron": ("scaled_barron(0, 0.1)", ("barron", 0.0, 0.1))}
SIZE = dict(width=320, height=240, n_points=2048)
SCENES = {
    "A": dict(seed=1001, sigma_px=2.0),
    "B": dict(seed=1002, sigma_px=2.0, k1=-0.05),
    # the object overfills the image: valid points read zero-padded texels at pad 0 (test_pose_uncertainty_gpu's "cropped")
    "E": dict(seed=1305, fill=1.5),
    "F": dict(seed=1305, fill=1.5, k1=-0.08),
    # the camera table (tests/camera_cases.py): ndist 4 (tangential terms in the point and its Jacobian), ndist 0, and
    # a range limit inside an overfilled image (k2 > 0 branch)
    "opencv": dict(seed=1401, sigma_px=2.0, **CC.SCENE_KW["opencv"]),
    "pinhole": dict(seed=1402, sigma_px=2.0, **CC.SCENE_KW["pinhole"]),
    "k2_limit": dict(seed=1305, **CC.SCENE_KW["k2_limit"]),
}
LEVEL_C = {0: 32, 1: 128, 2: 128}
ZERO_STOPS = dict(grad_stop_criteria=0.0, dt_stop_criteria=0.0, dR_stop_criteria=0.0)


def lm_variant(C, n, G, path):
    """lm_refine_problem's choice (csrc/pxt_lm.hip): 512 threads = 8 waves per workgroup, two 32-lane groups per wave."""
    groups32 = G * 8 * 2
    groups16, groups8 = 2 * groups32, 4 * groups32
    if path == 2:
        return 0
    if C == 32 and n <= groups8:
        return 1
    if C == 128 and n <= groups32:
        return 2
    if C == 128 and n <= groups16:
        return 3
    if C == 128 and n <= groups8:
        return 4
    return 0


def general_rounds(C, n, G):
    """Rounds of lm_accumulate's point loop and whether the last one is ragged."""
    per_round = G * 8 * (8 if C <= 32 else 2)
    return -(-n // per_round), n % per_round != 0


def _case(name, scene, levels, n, G, variants, path=0, pad=1, loss="barron", mask=None, iters=6, natural=False, kind="traj",
          lam="level"):
    return dict(name=name, scene=scene, levels=list(levels), n=n, G=G, variants=list(variants), path=path, pad=pad,
                loss=loss, mask=mask, iters=iters, natural=natural, kind=kind, lam=lam)


def _traj(name, scene, level, n, G, variant, **kw):
    return _case(name, scene, [level], n, G, [variant], **kw)


KEEP85 = ("keep", 4)  # a point mask keeping ~85 %
CASES = [
    # ---- accumulation variants at 8 workgroups (thresholds 128 / 256 / 512 groups), each also on the general path
    _traj("v2-n100", "A", 1, 100, 8, 2, lam="heavy"),
    _traj("v3-n200", "B", 2, 200, 8, 3, pad=0, loss="squared"),
    _traj("v4-n400", "A", 1, 400, 8, 4, pad=0, loss="huber", lam="heavy"),
    _traj("gen32-n600", "B", 1, 600, 8, 0, lam="heavy"),  # five rounds, the last ragged
    _traj("v1-n400", "A", 0, 400, 8, 1, loss="squared", lam="heavy"),
    _traj("gen8-n600", "A", 0, 600, 8, 0, pad=0),  # two rounds, the last ragged
    _traj("v2-n100-path2", "A", 1, 100, 8, 0, path=2, lam="heavy"),
    _traj("v3-n200-path2", "B", 2, 200, 8, 0, path=2, pad=0, loss="squared"),
    _traj("v4-n400-path2", "A", 1, 400, 8, 0, path=2, pad=0, loss="huber", lam="heavy"),
    _traj("gen32-n600-path2", "B", 1, 600, 8, 0, path=2, lam="heavy"),
    _traj("v1-n400-path2", "A", 0, 400, 8, 0, path=2, loss="squared", lam="heavy"),
    _traj("gen8-n600-path2", "A", 0, 600, 8, 0, path=2, pad=0),
    # the point counts on either side of a threshold
    _traj("v2-n128-edge", "A", 2, 128, 8, 2, pad=0),
    _traj("v3-n129-edge", "B", 1, 129, 8, 3, loss="huber", lam="heavy"),
    _traj("v4-n257-edge", "B", 2, 257, 8, 4, loss="squared", lam="heavy"),
    _traj("v4-n512-edge", "A", 2, 512, 8, 4, loss="huber"),
    _traj("v1-n512-edge", "B", 0, 512, 8, 1, loss="huber", lam="heavy"),
    _traj("gen32-n513-edge", "A", 1, 513, 8, 0, pad=0, lam="heavy"),
    # ---- grids: 1, 3, 17, 128 workgroups (17 and 128: a second trip of the 16-strided workgroup fold; 17 a partial,
    # 128 a double trip of the granule sweep)
    _traj("g1-gen32", "A", 1, 2048, 1, 0, lam="heavy"),
    _traj("g3-gen8", "A", 0, 2048, 3, 0, pad=0, loss="huber"),
    _traj("g3-v3", "A", 1, 90, 3, 3, lam="heavy"),
    _traj("g17-v4", "A", 2, 1000, 17, 4),
    _traj("g17-v1", "B", 0, 777, 17, 1, pad=0, lam="heavy"),
    _traj("g128-v2", "B", 1, 2048, 128, 2, loss="squared", lam="heavy"),
    _traj("g128-v1", "A", 0, 2048, 128, 1, lam="heavy"),
    _traj("g128-gen32", "A", 1, 2048, 128, 0, path=2, lam="heavy"),
    # ---- few points (min_valid = 10): 10 takes real steps
    _traj("n10", "A", 1, 10, 8, 2, lam="heavy"),
    _traj("n63", "B", 0, 63, 8, 1, lam="heavy"),
    _traj("n65", "A", 2, 65, 8, 2, pad=0),
    # ---- point masks
    _traj("mask85-v2", "B", 1, 2048, 128, 2, mask=KEEP85, lam="heavy"),
    _traj("mask85-gen8", "A", 0, 1500, 8, 0, mask=KEEP85),
    _traj("mask-leaves-10", "A", 1, 300, 8, 4, mask=("exact", 10), lam="heavy"),
    # ---- the masked identity step: fewer than min_valid valid points (default thresholds, three levels)
    _case("n1-fails", "A", [2, 1, 0], 1, 8, [2, 2, 1], iters=30, natural=True, kind="failed"),
    _case("n9-fails", "B", [2, 1, 0], 9, 8, [2, 2, 1], iters=30, natural=True, kind="failed"),
    _case("mask-leaves-9", "A", [2, 1, 0], 300, 8, [4, 4, 1], mask=("exact", 9), iters=30, natural=True, kind="failed"),
    # ---- the default thresholds, pose carried over three levels, natural stops (n_workgroups 0: the library's 128)
    _case("three-levels-n777", "B", [2, 1, 0], 777, 0, [2, 2, 1], iters=30, natural=True, kind="natural"),
    # ---- the camera table: OPENCV (p1, p2 in the point and in Jd00 / Jd01 / Jd10 / Jd11) on every accumulation variant,
    # the general path and lm_path = 2; PINHOLE over three levels
    _traj("opencv-v2-n100", "opencv", 2, 100, 8, 2),
    _traj("opencv-v3-n200", "opencv", 1, 200, 8, 3, lam="heavy"),
    _traj("opencv-v1-n400", "opencv", 0, 400, 8, 1, loss="squared", lam="heavy"),
    _traj("opencv-gen32-n600", "opencv", 1, 600, 8, 0, pad=0, lam="heavy"),
    _traj("opencv-v3-n200-path2", "opencv", 1, 200, 8, 0, path=2, lam="heavy"),
    _case("pinhole-three-levels-n777", "pinhole", [2, 1, 0], 777, 0, [2, 2, 1], iters=30, natural=True, kind="natural"),
]
# ---- border reads: one step per level at the initial pose, pad 0, both paths, two grids
for _scene, _runs in (("E", [(0, 128), (2, 128), (0, 8), (2, 8)]), ("F", [(0, 128), (2, 8)])):
    for _level in (0, 1, 2):
        for _path, _G in _runs:
            CASES.append(_case(f"border-{_scene}-L{_level}-path{_path}-g{_G}", _scene, [_level], 2048, _G,
                               [lm_variant(LEVEL_C[_level], 2048, _G, _path)], path=_path, pad=0, iters=1, natural=True,
                               kind="border"))
# ---- the k2 > 0 range limit inside the image: points beyond it must drop out of n_valid exactly (one step, pad 0)
for _level in (0, 1, 2):
    for _path, _G in [(0, 128), (2, 128), (0, 8), (2, 8)]:
        CASES.append(_case(f"border-k2_limit-L{_level}-path{_path}-g{_G}", "k2_limit", [_level], 2048, _G,
                           [lm_variant(LEVEL_C[_level], 2048, _G, _path)], path=_path, pad=0, iters=1, natural=True,
                           kind="border"))
# ---- one refine_levels_batch of three unlike problems (8 workgroups each, default thresholds)
BATCH = [
    _case("batch-0", "B", [2, 1, 0], 500, 8, [4, 4, 1], iters=30, natural=True, kind="natural"),
    _case("batch-1", "A", [1, 0], 1200, 8, [0, 0], mask=KEEP85, iters=30, natural=True, kind="natural"),
    _case("batch-2", "A", [2, 0], 64, 8, [2, 1], iters=30, natural=True, kind="natural"),
]


# ------------------------------------------------------------------------------------------------ host inputs
@functools.lru_cache(maxsize=None)
def scene(name):
    return make_lm_scene(**SIZE, **SCENES[name])


@functools.lru_cache(maxsize=None)
def packed_level(name, level):
    """What the refiner's fast path builds, on the host in float32: normalised HWC query map + normalised references,
    the level's camera and its ten floats, the level's lambdas."""
    sc = scene(name)
    fq = sc.feats_query[level]
    Cc = fq.shape[0] - 1
    cs = cstride_for(Cc)
    h, w = fq.shape[1:]
    fmap = torch.zeros(h, w, cs)
    fmap[..., :Cc] = O.l2_normalize(fq[:-1], dim=0).permute(1, 2, 0)
    fmap[..., Cc] = fq[-1]
    fr = sc.feats_ref[level]
    fref = torch.zeros(fr.shape[0], cs)
    fref[:, :Cc] = O.l2_normalize(fr[:, :-1], dim=1)
    fref[:, Cc] = fr[:, -1]
    cam = sc.camera.scale(sc.scales[level])
    ndist = int(cam._data.shape[-1] - 6)
    return dict(level=level, fmap=fmap, fref=fref, C=Cc, cam=cam, cam10=cam.as10(), ndist=ndist,
                chw={torch.float32: fmap[..., :Cc + 1].permute(2, 0, 1).contiguous(),
                     torch.float64: fmap[..., :Cc + 1].permute(2, 0, 1).contiguous().double()})


def point_mask(spec, n):
    if spec is None:
        return None
    if spec[0] == "keep":
        return np.random.default_rng(spec[1]).uniform(size=n) > 0.15
    m = np.zeros(n, bool)
    m[np.round(np.linspace(0, n - 1, spec[1])).astype(int)] = True
    assert int(m.sum()) == spec[1]
    return m


def host_problem(case):
    """The float32 numbers one launch is given: the first n points of the scene, their mask, T_init, the levels."""
    sc = scene(case["scene"])
    n = case["n"]
    T0 = np.concatenate([sc.R_init.reshape(-1), sc.t_init]).astype(np.float32)
    mask = point_mask(case["mask"], n)
    kind, alpha, scale = LOSSES[case["loss"]][1]
    return dict(case=case, n=n, p3d=torch.from_numpy(sc.p3d[:n]).float(), mask=None if mask is None else torch.from_numpy(mask),
                T0=T0,
                levels=[dict(packed_level(case["scene"], l), lam=O.damping_lambda(torch.as_tensor(
                    HEAVY if case["lam"] == "heavy" else CONSTS[l], dtype=torch.float32))) for l in case["levels"]],
                conf=O.LMConf(num_iters=case["iters"], pad=case["pad"], loss=kind, loss_alpha=alpha, loss_scale=scale,
                              min_valid=10))


def optimizer_conf(case):
    d = dict(num_iters=case["iters"], pad=case["pad"], loss_fn=LOSSES[case["loss"]][0], min_valid=10,
             n_workgroups=case["G"], lm_path=case["path"])
    if not case["natural"]:
        d.update(ZERO_STOPS)
    return d


# ------------------------------------------------------------------------------------------------ one oracle step
def oracle_step(hp, lv, T12, dtype, failed=False):
    """One LM step at the float32 pose T12 in `dtype`, plus what decides fairness: the smallest distance of any point to
    the padded border and the number of valid points whose 12-texel footprint reads outside the map."""
    n, Cc, pad = hp["n"], lv["C"], hp["conf"].pad
    T = torch.from_numpy(np.asarray(T12, np.float32).copy()).to(dtype)
    R, t = T[:9].reshape(3, 3), T[9:]
    cam = lv["cam10"][:6 + lv["ndist"]].to(dtype)
    chw = lv["chw"][dtype]
    fr = lv["fref"][:n].to(dtype)
    p3d = hp["p3d"].to(dtype)
    delta, g, H, n_valid, cost = O.lm_step(R, t, cam, p3d, fr[:, :Cc], chw[:Cc], fr[:, Cc:Cc + 1], chw[Cc:Cc + 1],
                                           lv["lam"].to(dtype), hp["conf"], mask=hp["mask"], failed=failed)
    p2d, visible = O.world2image(cam, O.pose_transform(R, t, p3d))
    h, w = chw.shape[1:]
    lim = torch.tensor([w - pad - 1, h - pad - 1], dtype=dtype)
    margin = float(torch.minimum((p2d - pad).abs().min(-1).values, (lim - p2d).abs().min(-1).values).min())
    valid = visible & O.mask_in_image(p2d, w, h, pad)
    p_cam = O.pose_transform(R, t, p3d).double().numpy()
    r2_margin = float(CC.r2_margin(cam[6:], p_cam).min())
    in_img = torch.all((p2d >= 0) & (p2d <= cam[:2] - 1), -1) & torch.from_numpy(p_cam[:, 2] > O.CAM_EPS)
    beyond_range = int((in_img & ~visible).sum())  # inside the image, in front of the camera, outside the model's range
    if hp["mask"] is not None:
        valid = valid & hp["mask"]
    assert int(valid.sum()) == n_valid
    # |sum_i |w_i J_i^T r_i||: what the float32 error of g scales with (g itself is a sum of cancelling terms)
    res, _, w_unc, J = O.residual_jacobian(R, t, cam, p3d, fr[:, :Cc], chw[:Cc], fr[:, Cc:Cc + 1], chw[Cc:Cc + 1], pad)
    kind, alpha, scale = hp["conf"].loss, hp["conf"].loss_alpha, hp["conf"].loss_scale
    _, w_loss = O.make_loss(kind, alpha, scale)((res ** 2).sum(-1))
    weights = w_loss * valid.to(dtype) * w_unc
    g_terms = float((weights[:, None] * torch.einsum("ndi,nd->ni", J, res).abs()).sum(0).norm())
    i0 = torch.floor(p2d).long()
    outside = (i0[:, 0] - 1 < 0) | (i0[:, 0] + 2 > w - 1) | (i0[:, 1] - 1 < 0) | (i0[:, 1] + 2 > h - 1)
    return dict(delta=delta.double().numpy(), g=g.double().numpy(), H=H.double().numpy(), n_valid=n_valid, cost=cost,
                failed=failed or n_valid < hp["conf"].min_valid, margin=margin, readers=int((valid & outside).sum()),
                t_norm=float(t.double().norm()), g_terms=g_terms, r2_margin=r2_margin, beyond_range=beyond_range)


def compose64(delta, T12):
    """(so3exp(dw), dt) @ T in float64 -> 12 float64."""
    T = torch.from_numpy(np.asarray(T12, np.float64))
    d = torch.from_numpy(np.asarray(delta, np.float64))
    R, t = O.pose_compose(O.so3exp(d[3:]), d[:3], T[:9].reshape(3, 3), T[9:])
    return np.concatenate([R.reshape(-1).numpy(), t.numpy()])


def so3_log(Rm):
    v = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    s = float(np.linalg.norm(v))
    return v if s < 1e-12 else v * (math.atan2(s, (np.trace(Rm) - 1.0) / 2.0) / s)


def step_between(T_prev, T_next):
    """The step the device took, from two logged float32 poses, in float64."""
    a, b = np.asarray(T_prev, np.float64), np.asarray(T_next, np.float64)
    Rd = b[:9].reshape(3, 3) @ a[:9].reshape(3, 3).T
    return np.concatenate([b[9:] - Rd @ a[9:], so3_log(Rd)])


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------ the replay
def replay(hp, res, native_conf):
    """Every logged iteration of `res` against one float64 step from the pose the device started it at.
    -> one record per iteration (for the printout); asserts everything the module docstring lists."""
    case = hp["case"]
    log = res.log.numpy()
    num_iters = case["iters"]
    f32 = np.float32
    dt_stop, dR_stop, grad_stop = f32(native_conf.dt_stop), f32(native_conf.dR_stop), f32(native_conf.grad_stop)
    assert res.total_iters == sum(res.iters), (res.total_iters, res.iters)
    T_prev = hp["T0"]
    failed = False
    out = []
    for li, lv in enumerate(hp["levels"]):
        n_it = res.iters[li]
        if failed:
            assert n_it == 0, res.iters  # the levels after a failure never start
            continue
        assert 1 <= n_it <= num_iters, res.iters
        for it in range(n_it):
            row = log[li, it]
            T_next = row[8:20]
            want = oracle_step(hp, lv, T_prev, torch.float64, failed)
            where = (case["name"], lv["level"], it)
            assert want["margin"] >= FAIR_MARGIN, f"unfair seed: a point {want['margin']:.2e} px from the border at {where}"
            assert want["r2_margin"] >= FAIR_R2_MARGIN, f"unfair seed: a point {want['r2_margin']:.2e} from the range limit at {where}"
            assert float(row[1]) == want["n_valid"], (where, float(row[1]), want["n_valid"])
            assert row[5] == 0.0, (where, "Cholesky failed")
            d64 = want["delta"]
            d_gpu = step_between(T_prev, T_next)
            rec = dict(where=where, d=float(np.linalg.norm(d64)), step_err=float(np.linalg.norm(d_gpu - d64)),
                       cost=float("nan"), gnorm=float("nan"))
            if want["n_valid"] > 0:
                rec["cost"] = rel(float(row[0]), want["cost"])
                assert rec["cost"] <= REL_COST, (where, "cost", float(row[0]), want["cost"])
                gn64 = float(np.linalg.norm(want["g"]))
                rec["gnorm"] = rel(float(row[4]), gn64)
                assert abs(float(row[4]) - gn64) <= REL_GTERMS * want["g_terms"], (where, "|g|", float(row[4]), gn64)
                if rec["d"] >= BIG_STEP or want["failed"]:
                    assert rec["gnorm"] <= REL_GNORM, (where, "|g|, relative", float(row[4]), gn64)
            failed = want["failed"]
            if failed:  # the masked identity step
                assert np.array_equal(T_next.view(np.uint32), np.asarray(T_prev, f32).view(np.uint32)), where
                assert row[2] == 0.0 and row[3] == 0.0, (where, row[2], row[3])
            else:
                bar = REL_STEP * rec["d"] + ABS_STEP + pose_rounding(want["t_norm"] + rec["d"])
                assert rec["step_err"] <= bar, (where, "step", d_gpu, d64, rec["step_err"], bar)
                dt64 = float(np.linalg.norm(d64[:3]))
                assert abs(float(row[3]) - dt64) <= REL_STEP * rec["d"] + ABS_STEP, (where, "dt", float(row[3]), dt64)
                w64 = float(np.linalg.norm(d64[3:]))
                cos_gpu = math.cos(float(row[2]) * math.pi / 180.0)
                cos_bar = COS_ABS + w64 * (REL_STEP * rec["d"] + ABS_STEP)
                assert abs(cos_gpu - math.cos(w64)) <= cos_bar, (where, "dR", float(row[2]), math.degrees(w64))
            # the stop rule, in float32, on the kernel's own numbers
            stop = bool((row[3] < dt_stop and row[2] < dR_stop) or row[4] < grad_stop)
            if it < n_it - 1:
                assert not stop and not failed, (where, "went on after its stop rule held", row[2:5])
            elif n_it < num_iters:
                assert stop, (where, "stopped before its stop rule held", row[2:5])
            out.append(rec)
            T_prev = T_next
    assert res.failed == failed
    assert np.array_equal(res.T.as12().numpy().view(np.uint32), np.asarray(T_prev, f32).view(np.uint32))
    return out


def show(records):
    for r in records:
        print("%-28s L%d it %d  |d| %.3e  step err %.2e  cost %.2e  |g| %.2e" % (*r["where"], r["d"], r["step_err"],
                                                                               r["cost"], r["gnorm"]))


# ------------------------------------------------------------------------------------------------ the device side
class Dev:
    def __init__(self, device):
        self.device = device
        self.levels = {}
        self.ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)

    def level(self, name, level):
        key = (name, level)
        if key not in self.levels:
            lv = packed_level(name, level)
            self.levels[key] = (lv["fmap"].to(self.device).contiguous(), lv["fref"].to(self.device).contiguous())
        return self.levels[key]

    def problem(self, hp):
        """-> (p3d, mask, packs, T_init) on the device for one host problem."""
        case, n = hp["case"], hp["n"]
        packs = []
        for lv in hp["levels"]:
            fmap, fref = self.level(case["scene"], lv["level"])
            packs.append(LevelPack(fmap, fref[:n], lv["C"], lv["cam"], lv["lam"]))
        mask = None if hp["mask"] is None else hp["mask"].to(torch.uint8).to(self.device)
        return hp["p3d"].to(self.device).contiguous(), mask, packs, Pose(torch.from_numpy(hp["T0"].copy()))


@pytest.fixture(scope="module")
def dv(device):
    return Dev(device)


def check_variants(case):
    G = case["G"] or 128
    got = [lm_variant(LEVEL_C[l], case["n"], G, case["path"]) for l in case["levels"]]
    assert got == case["variants"], (case["name"], got, case["variants"])


def check_shape_of_result(case, res):
    if case["kind"] == "traj":
        assert not res.failed and res.iters == [6], res.iters  # thresholds 0: exactly six steps
    elif case["kind"] == "failed":
        assert res.failed and res.iters == [1, 0, 0], res.iters
    elif case["kind"] == "border":
        assert not res.failed and res.iters == [1], res.iters
    else:
        assert not res.failed and all(1 <= n < case["iters"] for n in res.iters), res.iters  # natural stops


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_logged_step_matches_a_float64_replay(dv, case):
    check_variants(case)
    hp = host_problem(case)
    p3d, mask, packs, T_init = dv.problem(hp)
    conf = PixTrackOptimizer(optimizer_conf(case)).native_conf()
    res = PixTrackOptimizer.refine_levels(p3d, packs, T_init, conf, dv.ws, mask=mask).result()
    records = replay(hp, res, conf)
    show(records)
    check_shape_of_result(case, res)
    if case["kind"] == "traj":
        assert sum(r["d"] >= BIG_STEP for r in records) >= 3, "the relative bar must bite on at least three steps"


def test_every_problem_of_a_batched_launch_matches_its_replay(dv, device):
    n_ws = int(_lib.lib().pxt_lm_workspace_bytes())
    conf = PixTrackOptimizer(optimizer_conf(BATCH[0])).native_conf()
    hps, probs = [], []
    for case in BATCH:
        check_variants(case)
        hp = host_problem(case)
        p3d, mask, packs, T_init = dv.problem(hp)

        class Ref:
            pass

        ref = Ref()
        ref.p3d, ref.valid = p3d, mask
        hps.append(hp)
        probs.append({"ref": ref, "packs": packs, "T_init": T_init, "camera": None,
                      "workspace": torch.zeros(n_ws, dtype=torch.uint8, device=device)})
    bws = torch.zeros(int(_lib.lib().pxt_lm_batch_workspace_bytes(len(BATCH))), dtype=torch.uint8, device=device)
    handles = PixTrackOptimizer.refine_levels_batch(probs, conf, bws)
    for hp, h in zip(hps, handles):
        res = h.result()
        show(replay(hp, res, conf))
        check_shape_of_result(hp["case"], res)


# ------------------------------------------------------------------------------------------------ CPU calibration
def simulate(hp):
    """The case on the CPU alone: the float64 oracle's trajectory, rounded to float32 after every step; at every pose
    of it the float32 oracle against the float64 oracle.  -> one record per step."""
    case, conf = hp["case"], hp["conf"]
    oc = PixTrackOptimizer(optimizer_conf(case)).conf
    T = hp["T0"]
    failed = False
    out = []
    for lv in hp["levels"]:
        if failed:
            break
        for it in range(case["iters"]):
            a = oracle_step(hp, lv, T, torch.float32, failed)
            b = oracle_step(hp, lv, T, torch.float64, failed)
            d = float(np.linalg.norm(b["delta"]))
            rec = dict(level=lv["level"], it=it, d=d, margin=b["margin"], r2_margin=b["r2_margin"],
                       beyond_range=b["beyond_range"], readers=b["readers"], n_valid=b["n_valid"],
                       same_validity=a["n_valid"] == b["n_valid"], failed=b["failed"],
                       step_err=float(np.linalg.norm(a["delta"] - b["delta"])), cost=float("nan"), gnorm=float("nan"),
                       gterms=float("nan"))
            if b["n_valid"] > 0:
                rec["cost"] = rel(a["cost"], b["cost"])
                gn32, gn64 = float(np.linalg.norm(a["g"])), float(np.linalg.norm(b["g"]))
                rec["gnorm"] = abs(gn32 - gn64) / gn64
                rec["gterms"] = abs(gn32 - gn64) / b["g_terms"]
            out.append(rec)
            failed = b["failed"]
            T = compose64(b["delta"], T).astype(np.float32)
            dR = math.degrees(float(np.linalg.norm(b["delta"][3:])))
            dt = float(np.linalg.norm(b["delta"][:3]))
            gn = float(np.linalg.norm(b["g"]))
            if failed or (dt < oc.dt_stop_criteria and dR < oc.dR_stop_criteria) or gn < oc.grad_stop_criteria:
                break
    return out


if __name__ == "__main__":
    # No GPU.  The float32 oracle against the float64 oracle over CASES and BATCH, the fairness margins, the
    # border-reader counts, the steps at or above BIG_STEP per case - and every condition the cases must meet.
    import time

    t0 = time.time()
    for name in SCENES:
        sc = scene(name)
        for level in range(3):
            cq = float(sc.feats_query[level][-1].median())
            cr = float(sc.feats_ref[level][:, -1].median())
            print(f"scene {name} level {level}: median confidence query {cq:.3f} reference {cr:.3f}")
            assert cq > 1e-3 and cr > 1e-3, "a numerically dead level"
    seen = set()
    worst = dict(cost=0.0, gnorm=0.0, gterms=0.0, step_rel=0.0, step_abs=0.0)
    t_max = 0.0
    for case in CASES + BATCH:
        check_variants(case)
        for l, v in zip(case["levels"], case["variants"]):
            seen.add((LEVEL_C[l], v) if v else (LEVEL_C[l], 0) + general_rounds(LEVEL_C[l], case["n"], case["G"] or 128))
        assert case["n"] <= 2048
        hp = host_problem(case)
        recs = simulate(hp)
        big = sum(r["d"] >= BIG_STEP for r in recs)
        iters = [sum(r["level"] == l for r in recs) for l in case["levels"]]
        margin = min(r["margin"] for r in recs)
        for r in recs:
            assert r["same_validity"] and r["margin"] >= FAIR_MARGIN and r["r2_margin"] >= FAIR_R2_MARGIN, \
                ("unfair seed", case["name"], r)
            big_step = r["d"] >= BIG_STEP or r["failed"]  # (a masked step: |g| is that of the pose the level started at)
            if r["n_valid"] > 0:
                worst["cost"] = max(worst["cost"], r["cost"])
                worst["gterms"] = max(worst["gterms"], r["gterms"])
                if big_step:
                    worst["gnorm"] = max(worst["gnorm"], r["gnorm"])
            if not r["failed"]:
                if big_step:
                    worst["step_rel"] = max(worst["step_rel"], r["step_err"] / r["d"])
                else:
                    worst["step_abs"] = max(worst["step_abs"], r["step_err"])
        t_max = max(t_max, float(np.linalg.norm(hp["T0"][9:])))
        print(f"{case['name']:28s} iters {iters} steps>={BIG_STEP:g}: {big}  margin {margin:.3f} px  readers "
              f"{[r['readers'] for r in recs if r['it'] == 0]}  n_valid {recs[0]['n_valid']}  |d| "
              + " ".join(f"{r['d']:.1e}" for r in recs) + "  step err " + " ".join(f"{r['step_err']:.1e}" for r in recs)
              + "  |g| err " + " ".join(f"{r['gnorm']:.1e}" for r in recs))
        if case["kind"] == "traj":
            assert iters == [6] and not recs[-1]["failed"] and big >= 3, (case["name"], iters, big)
        elif case["kind"] == "failed":
            assert iters == [1, 0, 0] and recs[0]["failed"] and recs[0]["n_valid"] < 10, (case["name"], iters)
        elif case["kind"] == "border":
            assert iters == [1] and recs[0]["readers"] > 0 and not recs[0]["failed"], (case["name"], recs[0])
            if case["scene"] == "k2_limit":  # in-image points beyond the range exist: n_valid is exact only if they drop out
                print(f"{'':28s} {recs[0]['beyond_range']} points inside the image and beyond the range")
                assert recs[0]["beyond_range"] >= 20, (case["name"], recs[0])
        else:
            assert not recs[-1]["failed"] and all(1 <= n < case["iters"] for n in iters), (case["name"], iters)
    # every row of the accumulation matrix is populated
    for need in [(32, 1), (128, 2), (128, 3), (128, 4), (128, 0, 5, True), (32, 0, 2, True)]:
        assert need in seen, (need, sorted(seen, key=str))
    print("worst float32-vs-float64: relative cost %.3e, |g| over the sum of its terms' magnitudes %.3e; where |d| >= %g: "
          "relative |g| %.3e, relative step %.3e; where |d| < %g: absolute step %.3e"
          % (worst["cost"], worst["gterms"], BIG_STEP, worst["gnorm"], worst["step_rel"], BIG_STEP, worst["step_abs"]))
    print("constants in this file: F32_COST %.3e F32_GTERMS %.3e F32_GNORM %.3e F32_STEP_REL %.3e F32_STEP_ABS %.3e"
          % (F32_COST, F32_GTERMS, F32_GNORM, F32_STEP_REL, F32_STEP_ABS))
    print("pose rounding at the largest |t| = %.3f: %.3e; COS_ABS %.3e" % (t_max, pose_rounding(t_max), COS_ABS))
    for k, c in (("cost", F32_COST), ("gterms", F32_GTERMS), ("gnorm", F32_GNORM), ("step_rel", F32_STEP_REL),
                 ("step_abs", F32_STEP_ABS)):
        assert worst[k] <= c <= 1.1 * worst[k] + 1e-12, (k, worst[k], c, "the constants are stale: measure again")
    print("%.0f s" % (time.time() - t0))
