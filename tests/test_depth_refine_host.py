"""The sensor-depth refinement's numpy statement (pixtrack_amd/depth_refinement.py: the oracle of the GPU tests) on an
analytic scene, without a GPU: convergence from perturbed poses, every reject code on hand-placed points, the Jacobian
against finite differences, the failure and evaluate-only cases, and the ctypes mirrors of the two new structs.

The scene (pixtrack_amd/depth_scene.py): two ellipsoids (semi-axes (0.05, 0.02, 0.02) at the origin, (0.015, 0.04,
0.015) at (0.02, 0.01, 0)) in front of a plane at z = 0.45, seen by a 160 x 120 camera; the depth is ray-cast per pixel
and rounded to counts of 1e-4.
`python tests/test_depth_refine_host.py` prints the figures the bars below were taken from.
"""
import ctypes
import subprocess
import sys
import textwrap
from pathlib import Path

if __name__ == "__main__":  # (run as a script: the repository root is not on the path yet)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import pytest

from pixtrack_amd import depth_refinement as DR
from pixtrack_amd.depth_scene import CAM10, H, PLANE_Z, SCALE, W, make_scene, pose12, rodrigues

ROOT = Path(__file__).resolve().parent.parent

CONF = DR.DepthRefineConf(num_iters=10, pad=2, loss=1, loss_scale=0.004, lambda_=(1e-2,) * 6, max_residual=0.02,
                          max_edge=0.01, grad_stop=0.0, dt_stop=0.0, dR_stop=0.0, min_valid=10, relative=False)
SEEDS = tuple(range(8))

# float64 reference, 8 seeds, 1 deg / 4 mm perturbations, 10 iterations (measured by __main__ below; the bars are twice
# the worst seed):
ROT_ERR_DEG = 2 * 0.3104          # measured worst 0.3104 deg (from 1 deg)
TRANS_ERR = 2 * 8.46e-05          # measured worst 0.0846 mm (from 4 mm)
# with the prior diag(0, 0, 0, 50, 50, 50):
PRIOR_ROT_MOVE_DEG = 2 * 0.0032   # the rotation's distance from its START: measured worst 0.0032 deg
PRIOR_TRANS_ERR = 2 * 2.914e-04   # measured worst 0.2914 mm (from 4 mm)


def rot_deg(Ra, Rb):
    c = (np.trace(Ra @ Rb.T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


@pytest.fixture(scope="module")
def scene():
    return make_scene()


def perturbed(scene, seed, deg=1.0, trans=0.004):
    rng = np.random.default_rng(100 + seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dv = rng.normal(size=3)
    dv /= np.linalg.norm(dv)
    Rp = rodrigues(np.radians(deg) * ax)
    return pose12(Rp @ scene["R"], scene["t"] + trans * dv)  # (rotated about the object's origin)


def convergence_figures(scene, prior=None):
    out = []
    for seed in SEEDS:
        T0 = perturbed(scene, seed)
        res = DR.depth_refine_reference(scene["points"], None, scene["sensor"], SCALE, CAM10, 0, T0, CONF, prior=prior)
        T = res["T"]
        out.append({"rot": rot_deg(T[:9].reshape(3, 3), scene["R"]), "trans": float(np.linalg.norm(T[9:] - scene["t"])),
                    "rot_move": rot_deg(T[:9].reshape(3, 3), T0[:9].reshape(3, 3)),
                    "trans0": float(np.linalg.norm(T0[9:] - scene["t"])), "res": res})
    return out


def test_scene_keeps_the_expected_share_of_points(scene):
    assert 300 <= len(scene["points"]) <= 900, len(scene["points"])  # "about 480 of 6000"
    assert scene["sensor"].min() > 0  # the plane: every pixel has a measurement


def test_converges_from_perturbed_poses(scene):
    figs = convergence_figures(scene)
    for f in figs:
        res = f["res"]
        assert not res["failed"] and res["iterations"] == 10 and res["record"][31] == 1.0
        assert res["record"][16] <= res["record"][14]
        assert f["rot"] <= ROT_ERR_DEG and f["trans"] <= TRANS_ERR, (f["rot"], f["trans"])


def test_rotation_prior_holds_the_rotation_and_still_fixes_the_translation(scene):
    figs = convergence_figures(scene, prior=np.diag([0, 0, 0, 50.0, 50.0, 50.0]))
    for f in figs:
        assert f["rot_move"] <= PRIOR_ROT_MOVE_DEG, f["rot_move"]
        assert f["trans0"] > 3e-3 and f["trans"] <= PRIOR_TRANS_ERR, (f["trans0"], f["trans"])


def test_float32_statement_follows_the_float64_one(scene):
    T0 = perturbed(scene, 0)
    a = DR.depth_refine_reference(scene["points"], None, scene["sensor"], SCALE, CAM10, 0, T0, CONF, dtype=np.float64)
    b = DR.depth_refine_reference(scene["points"].astype(np.float32), None, scene["sensor"], np.float32(SCALE),
                                  CAM10.astype(np.float32), 0, T0.astype(np.float32), CONF, dtype=np.float32)
    assert b["record"].dtype == np.float32 and b["iterations"] == a["iterations"]
    assert np.abs(a["T"] - b["T"]).max() < 1e-4


def back_project(scene, u, v, z):
    fx, fy, cx, cy = CAM10[2:6]
    p = np.array([z * (u - cx) / fx, z * (v - cy) / fy, z])
    return scene["R"].T @ (p - scene["t"])


def find_surface_pixel(scene, flat=True):
    """(x, y) of an object pixel whose 6 x 6 surroundings are smooth (flat) - or, not flat, whose right neighbour is the
    background."""
    d = scene["depth"]
    for y in range(10, H - 10):
        for x in range(10, W - 10):
            win = d[y - 2:y + 4, x - 2:x + 4]
            if flat and d[y, x] < 0.4 and win.max() - win.min() < 0.004:
                return x, y
            if not flat and d[y, x] < 0.4 and d[y, x + 1] > 0.4 and d[y + 1, x] < 0.4 and d[y + 1, x + 1] > 0.4:
                return x, y
    raise AssertionError("no such pixel")


GATE_CODES_PAD2 = [0, 1, 2, 3, 4, 3, 5, 6, 4, 0, 3, 3]
GATE_CODES_PAD0 = [0, 1, 2, 0, 4, 4, 5, 6, 4, 0, 4, 4]  # (the border points lie on the plane: valid once inside)
GATE_CONF = DR.DepthRefineConf(num_iters=0, pad=2, loss=1, loss_scale=0.004, max_residual=0.02, max_edge=0.01,
                               min_valid=1, relative=False)


def hand_placed_points(scene):
    """-> (points [12, 3], mask, sensor): one point or more per reject code at the ground-truth pose, with fat margins;
    the expected codes are GATE_CODES_PAD2 / GATE_CODES_PAD0 under GATE_CONF."""
    sensor = scene["sensor"].copy()
    d = scene["depth"]

    def smooth(x, y):
        return d[y, x] < 0.4 and np.ptp(d[y - 2:y + 4, x - 2:x + 4]) < 0.004

    x0, y0 = find_surface_pixel(scene)
    xe, ye = find_surface_pixel(scene, flat=False)
    # a second smooth pixel, far from the first, takes the hole
    xh, yh = next((x, y) for y in range(H - 11, 10, -1) for x in range(W - 11, 10, -1)
                  if smooth(x, y) and abs(x - x0) + abs(y - y0) > 12)
    sensor[yh - 3:yh + 5, xh - 3:xh + 5] = 0
    # two more, far from both: one texel of the cross's outermost tap (row 1, column 3) punched under the first, the
    # 4 x 4 block's corner (row 0, column 0), which the cross does not read, under the second
    far = [(x0, y0), (xh, yh)]
    for _ in range(2):
        far.append(next((x, y) for y in range(10, H - 10) for x in range(10, W - 10)
                        if smooth(x, y) and all(max(abs(x - a), abs(y - b)) > 8 for a, b in far)))
    (xp, yp), (xc, yc) = far[2:]
    sensor[yp, xp + 2] = 0
    sensor[yc - 1, xc - 1] = 0

    def on_surface(x, y, dz=0.0):
        u, v = x + 0.4, y + 0.3
        ax, ay = 0.4, 0.3
        z = ((1 - ax) * (1 - ay) * d[y, x] + ax * (1 - ay) * d[y, x + 1] + (1 - ax) * ay * d[y + 1, x]
             + ax * ay * d[y + 1, x + 1])
        return back_project(scene, u, v, z + dz)

    pts = np.array([
        on_surface(x0, y0),                       # 0 valid
        on_surface(x0, y0),                       # 1 masked out
        back_project(scene, 80.0, 60.0, -0.1),    # 2 behind the camera
        back_project(scene, 1.3, 60.3, PLANE_Z),  # 3 inside the image, outside the padded window
        on_surface(xh, yh),                       # 4 over the hole
        back_project(scene, W - 1.5, 30.4, PLANE_Z),  # 3 with pad 2; with pad 0 its tap column W lies outside: 4
        back_project(scene, xe + 0.5, ye + 0.5, d[ye, xe]),  # 5 across the silhouette
        on_surface(x0, y0, dz=-0.05),             # 6 0.05 in front of the surface
        on_surface(xp, yp),                       # 4 one tap of twelve over a hole
        on_surface(xc, yc),                       # 0 a hole beside the cross
        back_project(scene, 0.6, 0.4, PLANE_Z),   # 3 with pad 2; with pad 0 tap column -1 and row -1 lie outside: 4
        back_project(scene, W - 1.4, H - 1.3, PLANE_Z),  # 3 with pad 2; with pad 0 tap column W and row H lie outside: 4
    ])
    mask = np.array([1, 0] + [1] * 10, dtype=np.uint8)
    return pts, mask, sensor


def gate_counts(codes):
    return [codes.count(c) for c in range(1, 7)]


def test_every_reject_code_on_hand_placed_points(scene):
    pts, mask, sensor = hand_placed_points(scene)
    conf = GATE_CONF
    assert set(GATE_CODES_PAD2) == set(range(7))
    for dtype in (np.float64, np.float32):
        st = DR.depth_step_reference(pts, mask, sensor, SCALE, CAM10, 0, scene["T"], conf, dtype=dtype)
        assert st["codes"].tolist() == GATE_CODES_PAD2
        assert st["counts"].tolist() == gate_counts(GATE_CODES_PAD2) == [1, 1, 4, 2, 1, 1] and st["n_valid"] == 2
        assert not DR.fragile_points(st).any()  # fat margins
        st0 = DR.depth_step_reference(pts, mask, sensor, SCALE, CAM10, 0, scene["T"], DR.DepthRefineConf(
            **{**conf.__dict__, "pad": 0}), dtype=dtype)
        assert st0["codes"].tolist() == GATE_CODES_PAD0
        assert not DR.fragile_points(st0).any()
    res = DR.depth_refine_reference(pts, mask, sensor, SCALE, CAM10, 0, scene["T"], conf)
    assert res["record"][18:24].tolist() == [1, 1, 4, 2, 1, 1] and res["record"][15] == 2 and res["record"][31] == 1.0
    assert res["codes"].shape == (1, 12)


def test_jacobian_against_finite_differences(scene):
    pts = scene["points"][:64]
    T = scene["T"]
    st = DR.depth_step_reference(pts, None, scene["sensor"], SCALE, CAM10, 0, T, CONF)
    assert (st["codes"] == 0).all()
    eps = 1e-6
    for k in range(6):
        delta = np.zeros(6)
        delta[k] = eps
        Tp, _, _ = DR.apply_delta_reference(delta, T)
        Tm, _, _ = DR.apply_delta_reference(-delta, T)
        sp = DR.depth_step_reference(pts, None, scene["sensor"], SCALE, CAM10, 0, Tp, CONF)
        sm = DR.depth_step_reference(pts, None, scene["sensor"], SCALE, CAM10, 0, Tm, CONF)
        dz = (sp["p"][:, 2] - sm["p"][:, 2]) / (2 * eps)
        du = (sp["u"] - sm["u"]) / (2 * eps)
        dv = (sp["v"] - sm["v"]) / (2 * eps)
        assert np.abs(dz - st["Jz"][:, k]).max() < 1e-8
        assert np.abs(du - st["J0"][:, k]).max() < 1e-5 * max(1.0, np.abs(st["J0"][:, k]).max())
        assert np.abs(dv - st["J1"][:, k]).max() < 1e-5 * max(1.0, np.abs(st["J1"][:, k]).max())
    assert np.allclose(st["J"], st["gx"][:, None] * st["J0"] + st["gy"][:, None] * st["J1"] - st["Jz"], rtol=0, atol=1e-15)

    # gx, gy: central differences of the bilinear depth, one pixel to either side
    a = scene["sensor"].astype(np.float64) * SCALE

    def bil(u, v):
        x, y = np.floor(u).astype(int), np.floor(v).astype(int)
        ax, ay = u - x, v - y
        return (1 - ax) * (1 - ay) * a[y, x] + ax * (1 - ay) * a[y, x + 1] + (1 - ax) * ay * a[y + 1, x] + ax * ay * a[y + 1, x + 1]

    u, v = st["u"], st["v"]
    assert np.abs(st["F"] - bil(u, v)).max() < 1e-14
    assert np.abs(st["gx"] - 0.5 * (bil(u + 1, v) - bil(u - 1, v))).max() < 1e-14
    assert np.abs(st["gy"] - 0.5 * (bil(u, v + 1) - bil(u, v - 1))).max() < 1e-14
    assert np.abs(st["r"] - (st["F"] - st["p"][:, 2])).max() == 0


def test_too_few_valid_points_fail_and_leave_the_pose(scene):
    T0 = perturbed(scene, 1)
    conf = DR.DepthRefineConf(**{**CONF.__dict__, "min_valid": len(scene["points"]) + 1})
    res = DR.depth_refine_reference(scene["points"], None, scene["sensor"], SCALE, CAM10, 0, T0, conf)
    rec = res["record"]
    assert res["failed"] and rec[12] == 1.0 and rec[13] == 0 and rec[31] == -2.0
    assert (rec[:12] == T0).all() and (rec[24:30] == 0).all()
    assert len(res["log"]) == 0 and res["codes"].shape[0] == 1
    assert not DR.accept(DR.decode_record(rec), True)


def test_zero_iterations_only_evaluate(scene):
    T0 = perturbed(scene, 2)
    conf = DR.DepthRefineConf(**{**CONF.__dict__, "num_iters": 0})
    res = DR.depth_refine_reference(scene["points"], None, scene["sensor"], SCALE, CAM10, 0, T0, conf)
    rec = res["record"]
    assert not res["failed"] and rec[13] == 0 and rec[31] == 1.0 and (rec[:12] == T0).all()
    assert rec[14] == rec[16] > 0 and rec[15] == rec[17] > 0
    st = DR.depth_step_reference(scene["points"], None, scene["sensor"], SCALE, CAM10, 0, T0, conf)
    assert rec[14] == st["cost"] / st["n_valid"] and rec[18:24].tolist() == st["counts"].tolist()


def test_defaults_are_fractions_of_the_extent():
    c = DR.DepthRefineConf()
    assert (c.loss, c.loss_scale, c.max_residual, c.max_edge, c.num_iters, c.min_valid, c.pad) == (1, 0.02, 0.1, 0.05, 10, 10, 2)
    assert c.lambda_ == (1e-2,) * 6 and c.relative
    a = DR.DepthRefineConf.from_sfm_scale(2.0)
    assert not a.relative and (a.loss_scale, a.max_residual, a.max_edge) == (0.04, 0.2, 0.1)
    assert a.resolve(5.0) is a
    with pytest.raises(ValueError):
        DR.depth_step_reference(np.zeros((1, 3)), None, np.ones((4, 4), np.uint16), 1.0, CAM10, 0, np.zeros(12), c)
    assert DR.points_extent(np.array([[0, 0, 0], [1, 2, 2.0]])) == 3.0
    assert DR.prior_upper((2.0, 3.0)).tolist() == DR.prior_upper(np.diag([2, 2, 2, 3, 3, 3.0])).tolist()


def test_cli_option_reads_the_sensor_files_and_refuses_a_directory_without_them(tmp_path, caplog):
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import build_parser, depth_option_from_args

    parser = build_parser()
    assert depth_option_from_args(parser.parse_args([])) is None
    with pytest.raises(ValueError):
        depth_option_from_args(parser.parse_args(["--depth_refine"]))
    image = np.arange(12, dtype=np.uint16).reshape(3, 4)
    np.save(tmp_path / "000001-depth.npy", image)
    argv = ["--depth_refine", "--sensor_depth_dir", str(tmp_path), "--sensor_depth_scale", "1e-4",
            "--sensor_depth_template", "{stem}.npy", "--sensor_depth_sub", "color", "depth", "--depth_prior", "0", "50"]
    opt = depth_option_from_args(parser.parse_args(argv))
    assert opt.sensor_depth_scale == 1e-4 and opt.prior == (0.0, 50.0) and opt.conf == DR.DepthRefineConf()
    # no file found yet: a wrong directory, template or substitution is an error, not a run that does nothing
    with pytest.raises(FileNotFoundError):
        opt.lookup("000002-color.png")
    got = opt.lookup("000001-color.png")
    assert got.dtype == np.uint16 and (got == image).all()
    # once files were found, a frame without one is logged and keeps the LM's pose
    with caplog.at_level("WARNING"):
        assert opt.lookup("000002-color.png") is None
    assert "000002-depth.npy" in caplog.text


def test_binding_and_op_are_registered():
    from pixtrack_amd import _build, _lib, ops

    assert (_build.CSRC / "pxt_depth_refine.hip").exists()
    assert "pxt_depth_refine" in _lib.PROTOTYPES and "pxt_depth_refine_workspace_bytes" in _lib.PROTOTYPES
    assert "depth_refine" in ops.op_names()
    assert (_lib.PXT_DEPTH_RECORD, _lib.PXT_DEPTH_LOG_STRIDE) == (DR.RECORD, DR.LOG_STRIDE)
    assert (_lib.PXT_DEPTH_MAX_POINTS, _lib.PXT_DEPTH_MAX_ITERS, _lib.PXT_DEPTH_MAX_PROBLEMS) == (
        DR.MAX_POINTS, DR.MAX_ITERS, DR.MAX_PROBLEMS)
    L = _lib.lib()
    assert int(L.pxt_depth_refine_workspace_bytes(1)) > 0 and int(L.pxt_depth_refine_workspace_bytes(17)) < 0


def test_struct_layouts_match_header_sizes(tmp_path):
    from pixtrack_amd import _lib

    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include "pixtrack_hip.h"
        int main(void) {
          printf("%zu %zu %d %d %d %d %d\\n", sizeof(pxt_depth_conf), sizeof(pxt_depth_problem), PXT_DEPTH_MAX_POINTS,
                 PXT_DEPTH_MAX_ITERS, PXT_DEPTH_MAX_PROBLEMS, PXT_DEPTH_RECORD, PXT_DEPTH_LOG_STRIDE);
          return 0;
        }
        """
    )
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    assert [ctypes.sizeof(_lib.DepthConf), ctypes.sizeof(_lib.DepthProblem)] == out[:2]
    assert out[2:] == [_lib.PXT_DEPTH_MAX_POINTS, _lib.PXT_DEPTH_MAX_ITERS, _lib.PXT_DEPTH_MAX_PROBLEMS,
                       _lib.PXT_DEPTH_RECORD, _lib.PXT_DEPTH_LOG_STRIDE]


if __name__ == "__main__":
    sc = make_scene()
    print("points kept:", len(sc["points"]), "of", len(sc["all_points"]))
    for name, prior in (("no prior", None), ("rotation prior 50", np.diag([0, 0, 0, 50.0, 50.0, 50.0]))):
        figs = convergence_figures(sc, prior)
        print(name, "worst rot %.4f deg, trans %.4f mm, rot move %.4f deg; start trans %.2f mm" % (
            max(f["rot"] for f in figs), 1e3 * max(f["trans"] for f in figs), max(f["rot_move"] for f in figs),
            1e3 * max(f["trans0"] for f in figs)))
        for f in figs:
            print("   rot %.4f trans %.4f mm move %.4f cost %.3e -> %.3e" % (
                f["rot"], 1e3 * f["trans"], f["rot_move"], f["res"]["record"][14], f["res"]["record"][16]))
