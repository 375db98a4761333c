"""pxt_depth_refine (csrc/pxt_depth_refine.hip) / torch.ops.pixtrack.depth_refine against a float64 replay of every
logged iteration, from the pose the device started that iteration at, on the float32 inputs widened
(pixtrack_amd/depth_refinement.py: depth_step_reference, solve6_reference, apply_delta_reference).

Per iteration: n_valid exactly, the mean cost, |g|, the step (the pose after it, dR, dt), the LU flag, the stop rule on
the kernel's own logged numbers; then the final record.  The reject codes are compared exactly for every point the
replay finds at least 1e-3 px from the padded border, 1e-4 (relative) from the edge and residual gates and 1e-4 px
from a texel boundary; the other, fragile points take the kernel's code in the replay, and may be at most 2 % of a
case's points at any step.

Bars (the project's method, tests/test_lm_steps_gpu.py): this file's __main__ runs the float32 statement of the kernel
through the same replay on the CPU, over every case; the worst deviations stand below as named constants with the
measured figure beside them, and the device gets 4 x that - the factor covers another summation order across lanes
and waves and the kernel's fused multiply-adds.  No bar comes from the kernel's own output.

The cases are the smallest that can still go wrong: the point counts at which the dealing of points to 1024 threads,
64-lane waves and min_valid = 10 changes (1, 9, 10, 63, 64, 65, 1023, 1024, 1025, 4096), an image whose uint16 rows are
no 4-byte multiples (161 x 119), a point mask, the three losses, k1 = -0.05, pads 0 and 2, no prior, a full positive
definite one and an indefinite one (which sends the solve to its LU fallback), damping that shapes the step, and a run
that stops by the default thresholds.  The points of those cases lie on the object in the middle of the image, so two
more, ``border_pad0`` and ``border_pad2``, carry what the gates are for: points on the background plane in the 3.5 px
band along all four borders (inside and outside the padded window; with pad 0 their footprints reach past every side
of the image), points behind the camera, and single texels zeroed under the footprints of object points.  The host
test's hand-placed points run through the kernel as well, at both pads, against the codes written down by hand.
__main__ requires every reject code 1..6 to occur among the cases.
Two cases carry the distortion of a camera of tests/camera_cases.py: ``opencv`` (ndist 4: the tangential terms of the
Jacobian the step is built from) and ``k2_limit``, with twenty points beyond the model's range (reject code 2) and
twenty inside it but outside the image (code 3) - dr_projectable restates project_point's range test by hand.  The
float32 statement stays below every constant above on both.
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
from pixtrack_amd import _lib
from pixtrack_amd import depth_refinement as DR
from pixtrack_amd.depth_scene import CAM10, SCALE, make_scene, pose12, rodrigues
from test_depth_refine_host import GATE_CODES_PAD0, GATE_CODES_PAD2, GATE_CONF, gate_counts, hand_placed_points

pytestmark = pytest.mark.gpu

# measured on the CPU by this file's __main__ (the float32 statement through the float64 replay; worst step of every case)
COST_REL_F32 = 7.4e-4    # mean cost, relative: r = F - p.z cancels seven digits near convergence (7.37e-04, case n10)
G_REL_F32 = 6.7e-9       # |g| against the rounding scale of its terms, sum w (|F| + |p.z|) |J| (6.67e-09, case n10)
POSE_ABS_F32 = 1.1e-6    # the pose after the step, largest entry (1.06e-06, case n63)
DR_DEG_F32 = 1.9e-2      # dR of the step, degrees: acos near 1 resolves 0.02 deg in float32 (1.90e-02, case natural_stop)
DT_ABS_F32 = 7.6e-8      # dt of the step (7.54e-08, case indefinite_prior)
UPDATE_ABS_F32 = 1.9e-6  # the accumulated update a (1.86e-06, case n63)
FACTOR = 4
MAX_FRAGILE = 0.02


def f32(x):
    return float(np.float32(x))


def conf_f32(conf):
    """The conf as the kernel receives it: every float rounded to float32."""
    d = dict(conf.__dict__)
    for k in ("loss_alpha", "loss_scale", "max_residual", "max_edge", "grad_stop", "dt_stop", "dR_stop"):
        d[k] = f32(d[k])
    d["lambda_"] = tuple(f32(x) for x in d["lambda_"])
    return DR.DepthRefineConf(**d)


BASE = DR.DepthRefineConf(num_iters=3, pad=2, loss=1, loss_scale=0.004, lambda_=(1e-2,) * 6, max_residual=0.02,
                          max_edge=0.01, grad_stop=0.0, dt_stop=0.0, dR_stop=0.0, min_valid=10, relative=False)
_A = np.random.default_rng(3).normal(size=(6, 6))
FULL_PRIOR = (_A @ _A.T) * np.outer([30, 30, 30, 1, 1, 1], [30, 30, 30, 1, 1, 1]) * 0.05
INDEFINITE_PRIOR = np.diag([0, 0, 0, 0, 0, -2e3])

# name -> (n_points, options)
CASES = {f"n{n}": (n, {}) for n in (1, 9, 10, 63, 64, 65, 1023, 1024, 1025, 4096)}
CASES.update({
    "odd_image": (600, dict(size=(161, 119))),
    "masked": (600, dict(mask=True)),
    "squared": (600, dict(conf=dict(loss=0))),
    "barron": (600, dict(conf=dict(loss=2, loss_alpha=0.0))),
    "radial": (600, dict(k1=-0.05)),
    "pad0": (600, dict(conf=dict(pad=0))),
    "full_prior": (600, dict(prior=FULL_PRIOR)),
    "indefinite_prior": (600, dict(prior=INDEFINITE_PRIOR)),
    "heavy_damping": (600, dict(conf=dict(lambda_=(10.0,) * 6, num_iters=5))),
    "natural_stop": (600, dict(conf="default", rot_deg=0.3, trans=0.001)),
    "border_pad0": (600, dict(conf=dict(pad=0), border=True)),
    "border_pad2": (600, dict(border=True)),
    # the distortion of two cameras of tests/camera_cases.py on this scene's camera: OPENCV (p1, p2 in the point and in
    # the four Jd terms the step is built from) and the k2 > 0 range limit, with points placed on either side of it -
    # dr_projectable is a hand copy of project_point's range test and must tell code 2 from code 3
    "opencv": (600, dict(dist=CC.CAMERAS["opencv"]["params"][4:])),
    "k2_limit": (600, dict(dist=CC.CAMERAS["k2_limit"]["params"][3:], range_band=True)),
})
N_BAND, N_BEHIND, N_HOLES = 80, 10, 8
N_RANGE = 40  # half beyond the range limit (code 2), half inside it and outside the image (code 3)

_SCENES = {}


def scene_for(size):
    if size not in _SCENES:
        _SCENES[size] = make_scene(size[0], size[1], n_per=40000, seed=11)
    return _SCENES[size]


_BUILT = {}


def border_extras(sc, size, good, rng):
    """-> (points [N_BAND + N_BEHIND, 3], sensor): points on the background plane from 1.5 px outside to 3.5 px inside
    the four borders and points behind the camera, placed at the ground-truth pose; the scene's sensor image with one texel
    zeroed somewhere in the 4 x 4 surroundings of N_HOLES of the ``good`` points."""
    Wd, Hd = size
    fx, fy, cx, cy = sc["cam10"][2:6]
    side = rng.integers(0, 4, N_BAND)
    band = rng.uniform(-1.5, 3.5, N_BAND)  # (negative: outside the image)
    u = np.select([side == 0, side == 1], [band, Wd - 1 - band], rng.uniform(0, Wd - 1, N_BAND))
    v = np.select([side == 2, side == 3], [band, Hd - 1 - band], rng.uniform(0, Hd - 1, N_BAND))
    u = np.concatenate([u, rng.uniform(20, Wd - 20, N_BEHIND)])
    v = np.concatenate([v, rng.uniform(20, Hd - 20, N_BEHIND)])
    z = np.concatenate([np.full(N_BAND, 0.45), np.full(N_BEHIND, -0.1)])  # (the scene's plane; behind the camera)
    p = np.stack([z * (u - cx) / fx, z * (v - cy) / fy, z], 1)
    extras = (p - sc["t"]) @ sc["R"]
    sensor = sc["sensor"].copy()
    q = good[:N_HOLES] @ sc["R"].T + sc["t"]
    x0 = np.floor(fx * q[:, 0] / q[:, 2] + cx).astype(int) + rng.integers(-1, 3, N_HOLES)
    y0 = np.floor(fy * q[:, 1] / q[:, 2] + cy).astype(int) + rng.integers(-1, 3, N_HOLES)
    sensor[y0, x0] = 0
    return extras, sensor


def range_extras(sc, dist, rng):
    """-> points [N_RANGE, 3] in front of the camera at the ground-truth pose: the first half at r^2 = 1.05 .. 1.5 x the
    model's range limit, the second at 0.8 .. 0.95 x (where the distorted point lies 150 px from the principal point:
    outside the 160 x 120 image in every direction)."""
    lim = CC.r2_limit(dist)
    r = np.sqrt(lim * np.concatenate([rng.uniform(1.05, 1.5, N_RANGE // 2), rng.uniform(0.8, 0.95, N_RANGE - N_RANGE // 2)]))
    phi = rng.uniform(0, 2 * np.pi, N_RANGE)
    p = 0.45 * np.stack([r * np.cos(phi), r * np.sin(phi), np.ones(N_RANGE)], 1)
    return (p - sc["t"]) @ sc["R"]


def build_case(name):
    """The float32 inputs of a case (and the conf as the kernel receives it)."""
    if name in _BUILT:
        return _BUILT[name]
    n, opt = CASES[name]
    size = opt.get("size", (160, 120))
    sc = scene_for(size)
    rng = np.random.default_rng(sum(map(ord, name)))
    n_bad = 0 if n <= 10 else int(round(0.15 * n))
    n_extra = N_BAND + N_BEHIND if opt.get("border") else (N_RANGE if opt.get("range_band") else 0)
    good = sc["points"][rng.permutation(len(sc["points"]))[:n - n_bad - n_extra]]
    bad = sc["all_points"][rng.permutation(len(sc["all_points"]))[:n_bad]]
    sensor = sc["sensor"]
    if opt.get("border"):
        extras, sensor = border_extras(sc, size, good, rng)
        bad = np.concatenate([bad, extras])
    elif opt.get("range_band"):
        bad = np.concatenate([bad, range_extras(sc, opt["dist"], rng)])
    pts = np.concatenate([good, bad])[rng.permutation(n)].astype(np.float32)
    assert len(pts) == n
    rot, trans = (0.2, 0.0005) if n <= 10 else (opt.get("rot_deg", 0.5), opt.get("trans", 0.002))
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dv = rng.normal(size=3)
    dv /= np.linalg.norm(dv)
    T0 = pose12(rodrigues(np.radians(rot) * ax) @ sc["R"], sc["t"] + trans * dv).astype(np.float32)
    cam10 = sc["cam10"].astype(np.float32)
    ndist = 0
    if "k1" in opt:
        cam10[6] = opt["k1"]
        ndist = 2
    if "dist" in opt:
        ndist = len(opt["dist"])
        cam10[6:6 + ndist] = opt["dist"]
    conf = opt.get("conf", {})
    if conf == "default":  # the package's defaults at the point set's extent; room for the stop rule to act
        conf = DR.DepthRefineConf(num_iters=32).resolve(DR.points_extent(sc["points"]))
    else:
        conf = DR.DepthRefineConf(**{**BASE.__dict__, **conf})
    mask = (rng.uniform(size=n) > 0.2).astype(np.uint8) if opt.get("mask") else None
    case = {"name": name, "points": pts, "mask": mask, "sensor": sensor, "scale": np.float32(SCALE), "cam10": cam10,
            "ndist": ndist, "T0": T0, "conf": conf_f32(conf), "prior": DR.prior_upper(opt.get("prior")).astype(np.float32)}
    _BUILT[name] = case
    return case


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30) if float(a) != float(b) else 0.0


def replay(case, out):
    """Holds a run - record [32], log [iterations, 20] and codes [iterations + 1, N], float32 as the kernel wrote them -
    to the float64 replay; raises on what must be exact, returns the worst deviations of what is rounded."""
    conf = case["conf"]
    w = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731  (float32 inputs widened)
    P = DR._prior_matrix(w(case["prior"]), np.float64)
    rec, log, codes = w(out["record"]), w(out["log"]), np.asarray(out["codes"])
    iters = int(rec[13])
    assert rec[13] == iters and 0 <= iters <= conf.num_iters and len(log) >= iters and len(codes) >= iters + 1
    dev = {"cost": 0.0, "g": 0.0, "pose": 0.0, "dR": 0.0, "dt": 0.0, "update": 0.0, "fragile": 0.0}
    T = w(case["T0"])
    a = np.zeros(6)
    stop = False

    def step(pose, used=None):
        return DR.depth_step_reference(w(case["points"]), case["mask"], case["sensor"], float(case["scale"]),
                                       w(case["cam10"]), case["ndist"], pose, conf, np.float64, codes=used)

    for i in range(iters + 1):
        st = step(T)
        frag = DR.fragile_points(st)
        dev["fragile"] = max(dev["fragile"], float(frag.mean()))
        assert frag.mean() <= MAX_FRAGILE, (case["name"], i, frag.mean())
        kc = codes[i]
        wrong = np.flatnonzero(~frag & (kc != st["codes"]))
        assert len(wrong) == 0, (case["name"], i, wrong[:8], kc[wrong[:8]], st["codes"][wrong[:8]])
        st = step(T, np.where(frag, kc, st["codes"]).astype(np.uint8))
        n_valid = st["n_valid"]
        mean = st["cost"] / max(n_valid, 1)
        fail = n_valid < conf.min_valid
        if i == iters:  # the evaluation without an update: the kernel was right to end here, and its record says why
            assert fail or stop or i == conf.num_iters, (case["name"], i)
            assert rec[17] == n_valid and rec[12] == float(fail) and rec[31] == (-2.0 if fail else 1.0)
            assert rec[18:24].tolist() == st["counts"].tolist()
            assert rec[18:24].tolist() == [int((kc == c).sum()) for c in range(1, 7)]
            dev["cost"] = max(dev["cost"], rel(rec[16], mean))
            break
        assert not fail and not stop, (case["name"], i, n_valid, stop)  # the kernel went on: it had to
        line = log[i]
        assert line[1] == n_valid and line[6] == 0 and line[7] == 0
        dev["cost"] = max(dev["cost"], rel(line[0], mean))
        g = st["g"] + P @ a
        Hm = st["H"] + P
        v = st["used"] == 0
        # r = F - p.z is rounded at the size of F and p.z, not at its own (near convergence seven digits cancel): the
        # sum g = sum w r J carries errors of the size of sum w (|F| + |p.z|) |J| eps, whatever r is
        g_scale = np.linalg.norm(((st["w"][v] * (np.abs(st["F"][v]) + np.abs(st["p"][v, 2])))[:, None]
                                  * np.abs(st["J"][v])).sum(0) + np.abs(P) @ np.abs(a))
        dev["g"] = max(dev["g"], abs(line[4] - np.linalg.norm(g)) / max(g_scale, 1e-30))
        delta, lu = DR.solve6_reference(g, Hm, conf.lambda_)
        assert line[5] == float(lu), (case["name"], i)
        Tn, dR, dtr = DR.apply_delta_reference(delta, T)
        dev["pose"] = max(dev["pose"], float(np.abs(line[8:20] - Tn).max()))
        dev["dR"] = max(dev["dR"], abs(line[2] - dR))
        dev["dt"] = max(dev["dt"], abs(line[3] - dtr))
        # the stop rule on the kernel's own numbers, in its arithmetic
        l32 = out["log"][i].astype(np.float32)
        stop = bool((l32[3] < np.float32(conf.dt_stop) and l32[2] < np.float32(conf.dR_stop))
                    or l32[4] < np.float32(conf.grad_stop))
        a = a + delta
        T = line[8:20].copy()  # the pose the device starts the next evaluation at
    r32 = np.asarray(out["record"], dtype=np.float32)
    last = np.asarray(out["log"][iters - 1][8:20] if iters else case["T0"], dtype=np.float32)
    np.testing.assert_array_equal(r32[:12].view(np.uint32), last.view(np.uint32))
    first = np.asarray(out["log"][0][:2] if iters else r32[16:18], dtype=np.float32)
    np.testing.assert_array_equal(r32[14:16].view(np.uint32), first.view(np.uint32))
    dev["update"] = float(np.abs(rec[24:30] - a).max())
    assert rec[30] == 0
    return dev, iters


def check(dev):
    assert dev["cost"] <= FACTOR * COST_REL_F32, dev
    assert dev["g"] <= FACTOR * G_REL_F32, dev
    assert dev["pose"] <= FACTOR * POSE_ABS_F32, dev
    assert dev["dR"] <= FACTOR * DR_DEG_F32, dev
    assert dev["dt"] <= FACTOR * DT_ABS_F32, dev
    assert dev["update"] <= FACTOR * UPDATE_ABS_F32, dev


# ------------------------------------------------------------------------------------------------ device helpers
def problem(case, device, pose=None):
    sensor = torch.from_numpy(np.ascontiguousarray(case["sensor"]).view(np.int16)).to(device)
    return dict(points=torch.from_numpy(case["points"]).to(device),
                mask=None if case["mask"] is None else torch.from_numpy(case["mask"]).to(device), sensor=sensor,
                sensor_scale=float(case["scale"]), camera=(case["cam10"], case["ndist"]),
                pose=case["T0"] if pose is None else pose, prior=case["prior"])


def run_gpu(cases, device, conf=None):
    """One launch for the cases (sharing ``conf``, default the first one's) -> one dict(record, log, codes) per case."""
    conf = conf or cases[0]["conf"]
    h = DR.depth_refine_batch([problem(c, device) for c in cases], conf, want_log=True, want_codes=True)
    recs = h.result()
    torch.cuda.synchronize(device)
    return [{"record": h.recs[k].numpy().copy(), "log": h.logs[k].cpu().numpy(), "codes": h.codes[k].cpu().numpy()}
            for k in range(len(cases))], recs


@pytest.mark.parametrize("name", list(CASES))
def test_every_iteration_against_the_float64_replay(device, name):
    case = build_case(name)
    out = run_gpu([case], device)[0][0]
    dev, iters = replay(case, out)
    print(name, "iterations", iters, "status", out["record"][31], {k: f"{v:.2e}" for k, v in dev.items()})
    check(dev)
    n = CASES[name][0]
    if n < 10:
        assert out["record"][31] == -2.0 and iters == 0  # fewer points than min_valid: failed at the first evaluation
    if name == "indefinite_prior":
        assert out["log"][:iters, 5].any()  # the LU fallback ran
    if name == "natural_stop":
        assert 0 < iters < case["conf"].num_iters  # stopped by the default thresholds
    if name.startswith("border"):  # the gates these cases are for acted on the device, at every evaluation
        for row in out["codes"][:iters + 1]:
            assert {2, 3, 4} <= set(row.tolist()), np.bincount(row, minlength=7)
    if name == "k2_limit":  # beyond the range: code 2, all of them and no other point; inside it and off the image: code 3
        assert iters >= 1
        for row in out["codes"][:iters + 1]:
            assert int((row == 2).sum()) == N_RANGE // 2 and int((row == 3).sum()) >= N_RANGE // 2, np.bincount(row, minlength=7)
    # rows the run did not reach stay as the caller left them
    assert not out["log"][iters:].any() and not out["codes"][iters + 1:].any()


def gate_case(pad):
    """The host test's hand-placed points (tests/test_depth_refine_host.py) as a case: one evaluation at the
    ground-truth pose."""
    if "gates" not in _SCENES:
        _SCENES["gates"] = make_scene()
    sc = _SCENES["gates"]
    pts, mask, sensor = hand_placed_points(sc)
    conf = DR.DepthRefineConf(**{**GATE_CONF.__dict__, "pad": pad})
    return {"name": f"gates_pad{pad}", "points": pts.astype(np.float32), "mask": mask, "sensor": sensor,
            "scale": np.float32(SCALE), "cam10": CAM10.astype(np.float32), "ndist": 0, "T0": sc["T"].astype(np.float32),
            "conf": conf_f32(conf), "prior": np.zeros(21, np.float32)}


@pytest.mark.parametrize("pad,expected", [(2, GATE_CODES_PAD2), (0, GATE_CODES_PAD0)])
def test_hand_placed_gate_points_on_the_device(device, pad, expected):
    """Every reject code, decided by the kernel on points placed by hand with fat margins: masked, behind the camera,
    outside the padded window, over a hole, ONE tap of the twelve over a hole, a hole beside the cross, across the
    silhouette, in front of the surface - and, with pad 0, footprints that reach past column W, row H, column -1 and
    row -1, whose taps count as raw 0."""
    case = gate_case(pad)
    out = run_gpu([case], device)[0][0]
    rec = out["record"]
    print("pad", pad, "codes", out["codes"][0].tolist(), "counts", rec[18:24].tolist())
    assert out["codes"][0].tolist() == expected
    assert rec[18:24].tolist() == gate_counts(expected)
    assert rec[15] == rec[17] == expected.count(0) and rec[13] == 0 and rec[12] == 0 and rec[31] == 1.0
    dev, iters = replay(case, out)  # (the record against the replay; the cost of two points sets no bar)
    assert iters == 0 and dev["fragile"] == 0


def test_a_problem_depends_on_itself_alone(device):
    cases = [build_case("n1025"), build_case("odd_image"), build_case("full_prior")]
    conf = cases[0]["conf"]
    alone = [run_gpu([c], device, conf)[0][0] for c in cases]
    again = [run_gpu([c], device, conf)[0][0] for c in cases]
    batch = run_gpu(cases, device, conf)[0]  # three unlike problems: parameter records through the workspace
    rolled = run_gpu(cases[1:] + cases[:1], device, conf)[0]  # every problem at every one of the three positions
    rolled = rolled[-1:] + rolled[:-1]
    rolled2 = run_gpu(cases[2:] + cases[:2], device, conf)[0]
    rolled2 = rolled2[-2:] + rolled2[:-2]
    # batches of two: the largest whose parameter records still travel as kernel arguments
    pairs = [run_gpu([cases[k], cases[(k + 1) % 3]], device, conf)[0] for k in range(3)]
    for k in range(3):
        assert alone[k]["record"][31] == 1.0
        for other in (again[k], batch[k], rolled[k], rolled2[k], pairs[k][0], pairs[(k + 2) % 3][1]):
            for key in ("record", "log", "codes"):
                a, b = alone[k][key], other[key]
                np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                              b.view(np.uint32) if b.dtype == np.float32 else b)


def call_op(device, case, pose, is_record, rec, log, codes, conf=None):
    from pixtrack_amd.ops import ops

    conf = conf or case["conf"]
    p = problem(case, device)
    ws = torch.zeros(int(_lib.lib().pxt_depth_refine_workspace_bytes(1)), dtype=torch.uint8, device=device)
    ops.depth_refine([p["points"]], [p["mask"]], [p["sensor"]], [p["sensor_scale"]], [float(x) for x in case["cam10"]],
                     [case["ndist"]], [pose], is_record, [float(x) for x in case["prior"]], conf.num_iters, conf.pad,
                     conf.loss, conf.loss_alpha, conf.loss_scale, list(conf.lambda_), conf.max_residual, conf.max_edge,
                     conf.grad_stop, conf.dt_stop, conf.dR_stop, conf.min_valid, [rec], [log], [codes], ws)
    return p, ws


def test_chained_behind_the_lm_on_the_device(device):
    """Queued behind a real pxt_lm_refine with pose_is_lm_record = 1: the bits of a call given that pose as 12 floats;
    behind a failed LM record only word 31 is written."""
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer
    from test_pose_uncertainty_gpu import PAD, build_scene, pack_level, to_dev

    sc, _ = build_scene("qvga")
    levels = [pack_level(sc, l) for l in range(3)]
    devl = [to_dev(device, *lv, sc.p3d, None) for lv in levels]
    init = np.concatenate([sc.R_init.reshape(-1), sc.t_init]).astype(np.float32)
    opt = PixTrackOptimizer(dict(num_iters=100, pad=PAD))
    conf_lm = opt.native_conf()
    lam = torch.full((6,), 1e-2)
    packs = [LevelPack(devl[l]["fmap"], devl[l]["fref"], devl[l]["C"], levels[l][3], lam) for l in (2, 1, 0)]
    lm_ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)

    # the depth problem: the LM scene's points and camera over a plane at the points' median depth
    p3d = np.asarray(sc.p3d, dtype=np.float32)[:2048]
    cam = levels[0][3]
    cam10 = cam.as10().numpy().astype(np.float32)
    Wd, Hd = int(cam10[0]), int(cam10[1])
    R0, t0 = init[:9].reshape(3, 3).astype(np.float64), init[9:].astype(np.float64)
    z = np.median((p3d.astype(np.float64) @ R0.T + t0)[:, 2])
    scale = np.float32(z / 3000.0)
    ext = DR.points_extent(p3d)
    # (a point cloud over a flat depth image is no pose problem: heavy damping keeps the three steps small)
    conf = conf_f32(DR.DepthRefineConf(num_iters=3, pad=2, loss=1, loss_scale=0.5 * ext, max_residual=2 * ext,
                                       max_edge=ext, lambda_=(1e3,) * 6, grad_stop=0.0, dt_stop=0.0, dR_stop=0.0,
                                       relative=False))
    case = {"name": "chained", "points": p3d, "mask": None, "sensor": np.full((Hd, Wd), 3000, np.uint16), "scale": scale,
            "cam10": cam10, "ndist": int(cam._data.shape[-1] - 6), "conf": conf, "prior": np.zeros(21, np.float32), "T0": init}
    N = len(p3d)

    def buffers(fill):
        rec = torch.full((32,), fill).pin_memory()
        return rec, torch.full((3, 20), fill, device=device), torch.full((4, N), 77, dtype=torch.uint8, device=device)

    pending = PixTrackOptimizer.refine_levels(devl[0]["p3d"], packs, Pose(torch.from_numpy(init)), conf_lm, lm_ws, mask=None)
    rec, log, codes = buffers(0.0)
    keep = call_op(device, case, pending.buf, True, rec, log, codes)  # (no synchronisation between the two launches)
    res = pending.result()
    torch.cuda.synchronize(device)
    assert not res.failed and rec[31] == 1.0 and rec[15] > 100
    T_lm = res.T.as12().numpy().astype(np.float32)
    pose = torch.zeros(16).pin_memory()
    pose[:12] = torch.from_numpy(T_lm)
    rec2, log2, codes2 = buffers(0.0)
    keep2 = call_op(device, case, pose, False, rec2, log2, codes2)
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(rec.numpy().view(np.uint32), rec2.numpy().view(np.uint32))
    np.testing.assert_array_equal(log.cpu().numpy().view(np.uint32), log2.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(codes.cpu().numpy(), codes2.cpu().numpy())

    # a refinement that reports `failed` (a point mask keeping fewer than min_valid points): skipped
    few = torch.zeros(devl[0]["p3d"].shape[0], dtype=torch.uint8, device=device)
    few[:5] = 1
    pending = PixTrackOptimizer.refine_levels(devl[0]["p3d"], packs, Pose(torch.from_numpy(init)), conf_lm, lm_ws, mask=few)
    rec3, log3, codes3 = buffers(123.0)
    keep3 = call_op(device, case, pending.buf, True, rec3, log3, codes3)
    res = pending.result()
    torch.cuda.synchronize(device)
    assert res.failed
    r3 = rec3.numpy()
    assert r3[31] == -1.0 and np.all(r3[:31] == 123.0)
    assert bool((log3 == 123.0).all()) and bool((codes3 == 77).all())
    assert DR.decode_record(r3)["status"] == -1.0 and not DR.accept(DR.decode_record(r3), True)
    del keep, keep2, keep3


def test_argument_errors_launch_and_write_nothing(device):
    L = _lib.lib()
    case = build_case("n64")
    p = problem(case, device)
    N = 64
    out = torch.full((40,), 55.0, device=device)
    log = torch.full((3, 20), 55.0, device=device)
    codes = torch.full((4, N), 55, dtype=torch.uint8, device=device)
    pose = torch.zeros(20, device=device)
    pose[:12] = torch.from_numpy(case["T0"]).to(device)
    ws = torch.zeros(int(L.pxt_depth_refine_workspace_bytes(_lib.PXT_DEPTH_MAX_PROBLEMS)), dtype=torch.uint8, device=device)
    stream = int(torch.cuda.current_stream(device).cuda_stream)

    def fresh():
        q = _lib.DepthProblem()
        q.p3d, q.point_mask, q.n_points = p["points"].data_ptr(), None, N
        q.sensor, q.width, q.height, q.sensor_scale = p["sensor"].data_ptr(), 160, 120, float(case["scale"])
        q.cam[:] = [float(x) for x in case["cam10"]]
        q.ndist, q.pose, q.pose_is_lm_record = 0, pose.data_ptr(), 0
        q.out, q.log, q.codes = out.data_ptr(), log.data_ptr(), codes.data_ptr()
        c = _lib.DepthConf()
        c.num_iters, c.pad, c.loss, c.loss_scale, c.min_valid = 3, 2, 1, 0.004, 10
        c.lambda_[:] = [1e-2] * 6
        c.max_residual, c.max_edge = 0.02, 0.01
        return q, c

    def call(q, c, K=1, workspace=None, probs=None):
        arr = probs if probs is not None else (_lib.DepthProblem * max(K, 1))(*([q] * max(K, 1)))
        return L.pxt_depth_refine(arr, K, C.byref(c), ws.data_ptr() if workspace is None else workspace, stream)

    def bad(**kw):
        q, c = fresh()
        for k, v in kw.items():
            setattr(c if hasattr(c, k) else q, k, v)
        return call(q, c)

    E = -1  # PXT_E_ARG
    assert bad(n_points=0) == E and bad(n_points=_lib.PXT_DEPTH_MAX_POINTS + 1) == E
    assert bad(num_iters=-1) == E and bad(num_iters=_lib.PXT_DEPTH_MAX_ITERS + 1) == E
    assert bad(width=3) == E and bad(height=3) == E
    assert bad(width=1 << 15, height=(1 << 15) + 1) == E  # more than 2^30 pixels (checked before anything is read)
    assert bad(log=log.data_ptr() + 2) == E
    assert bad(pad=-1) == E and bad(loss=3) == E and bad(loss=-1) == E and bad(min_valid=-1) == E and bad(ndist=1) == E
    assert bad(p3d=None) == E and bad(sensor=None) == E and bad(pose=None) == E and bad(out=None) == E
    assert bad(p3d=p["points"].data_ptr() + 4) == E and bad(pose=pose.data_ptr() + 4) == E
    assert bad(out=out.data_ptr() + 4) == E and bad(sensor=p["sensor"].data_ptr() + 1) == E
    q, c = fresh()
    assert call(q, c, K=0) == E and call(q, c, K=_lib.PXT_DEPTH_MAX_PROBLEMS + 1,
                                          probs=(_lib.DepthProblem * 17)(*([q] * 17))) == E
    assert call(q, c, workspace=0) == E and call(q, c, workspace=ws.data_ptr() + 4) == E
    assert call(q, c, K=2) == E  # two problems writing one record
    assert L.pxt_depth_refine(None, 1, C.byref(c), ws.data_ptr(), stream) == E
    assert L.pxt_depth_refine((_lib.DepthProblem * 1)(q), 1, None, ws.data_ptr(), stream) == E
    assert int(L.pxt_depth_refine_workspace_bytes(0)) == E and int(L.pxt_depth_refine_workspace_bytes(17)) == E
    torch.cuda.synchronize(device)
    assert bool((out == 55.0).all()) and bool((log == 55.0).all()) and bool((codes == 55).all())
    # and the same problem, untouched, runs
    assert call(q, c) == 0
    torch.cuda.synchronize(device)
    assert float(out[31]) == 1.0 and bool((out[32:] == 55.0).all())


if __name__ == "__main__":
    worst = {}
    seen = np.zeros(7, dtype=np.int64)
    for pad, expected in ((2, GATE_CODES_PAD2), (0, GATE_CODES_PAD0)):
        case = gate_case(pad)
        ref = DR.depth_refine_reference(case["points"], case["mask"], case["sensor"], case["scale"], case["cam10"], 0,
                                        case["T0"], case["conf"], dtype=np.float32)
        assert ref["codes"][0].tolist() == expected, (pad, ref["codes"][0].tolist())
        dev, _ = replay(case, {"record": ref["record"], "log": ref["log"], "codes": ref["codes"]})
        print(case["name"], " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for name in CASES:
        case = build_case(name)
        ref = DR.depth_refine_reference(case["points"], case["mask"], case["sensor"], case["scale"], case["cam10"],
                                        case["ndist"], case["T0"], case["conf"], prior=case["prior"], dtype=np.float32)
        n = ref["iterations"]
        out = {"record": ref["record"].astype(np.float32), "log": ref["log"].astype(np.float32), "codes": ref["codes"]}
        dev, iters = replay(case, out)
        # the float64 reference's own trajectory: its fragile share
        r64 = DR.depth_refine_reference(case["points"].astype(np.float64), case["mask"], case["sensor"], float(case["scale"]),
                                        case["cam10"].astype(np.float64), case["ndist"], case["T0"].astype(np.float64),
                                        case["conf"], prior=case["prior"].astype(np.float64))
        frag64 = max(float(DR.fragile_points(s).mean()) for s in r64["steps"])
        assert frag64 <= MAX_FRAGILE, (name, frag64)
        hist = np.bincount(ref["codes"].reshape(-1), minlength=7)
        seen += hist
        if name.startswith("border"):
            assert all({2, 3, 4} <= set(row.tolist()) for row in ref["codes"]), (name, hist)
        if name == "k2_limit":
            assert iters >= 1 and all(int((row == 2).sum()) == N_RANGE // 2 and int((row == 3).sum()) >= N_RANGE // 2
                                      for row in ref["codes"][:iters + 1]), (name, hist)
        print(f"{name:18s} N {len(case['points']):5d} iters {iters:2d} status {out['record'][31]:+.0f} n_valid "
              f"{int(out['record'][15]):5d} -> {int(out['record'][17]):5d} LU {int(out['log'][:n, 5].sum())} fragile64 {frag64:.4f} "
              + " ".join(f"{k} {v:.2e}" for k, v in dev.items()) + f" codes {hist.tolist()}")
        for k, v in dev.items():
            if v >= worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, name)
    print("worst:", {k: (f"{v:.2e}", n) for k, (v, n) in worst.items()})
    print("codes 0..6 over all cases:", seen.tolist())
    assert (seen[1:] > 0).all(), seen  # every reject code occurs in some case
