"""The host side of the sensor-depth VSD (pixtrack_amd/sensor_evaluation.py): the numpy restatement of pxt_sensor_vsd's
per-pixel rules against an independent float64 transcription of BOP's ``vsd`` (Hodan et al., ECCV 2018 / BOP 2019:
``estimate_visib_mask_gt`` / ``_est`` in bop19 mode, step cost), a hand-checked occlusion scene, the camera's part (ray
factors, sensor alignment), the depth image reader, the figures' conventions and the command line's parser.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import sensor_evaluation as SE
from pixtrack_amd.geometry import Camera

ROOT = Path(__file__).resolve().parent.parent
MIN_ALPHA = 0.5


# --------------------------------------------------------------------------------- BOP's vsd, transcribed in float64
def _bop_visib_mask(d_test, d_model, delta):
    """bop19: a model pixel is visible when it is not behind the measured surface by more than delta, or when the
    sensor measured nothing there."""
    d_diff = d_model - d_test
    return ((d_diff <= delta) | (d_test == 0)) & (d_model > 0)


def _bop_vsd(dist_est, dist_gt, dist_test, delta, taus):
    """-> (errors per tau, |visib_gt|, |visib_est|, |inter|, |union|); the distance images hold 0 off the object."""
    visib_gt = _bop_visib_mask(dist_test, dist_gt, delta)
    visib_est = _bop_visib_mask(dist_test, dist_est, delta) | (visib_gt & (dist_est > 0))
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    n_union = int(union.sum())
    comp = n_union - int(inter.sum())
    dists = np.abs(dist_gt[inter] - dist_est[inter])
    if n_union == 0:
        errors = [1.0] * len(taus)
    else:
        errors = [(int((dists >= tau).sum()) + comp) / float(n_union) for tau in taus]
    return errors, int(visib_gt.sum()), int(visib_est.sum()), int(inter.sum()), n_union


def _seeded(W, H, P, seed):
    """Two offset discs; alpha from {0, 1/4, 1/2, 3/4, 1}, channel 0 and the sensor counts quarter-integers."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.45 * max(W, H) + 0.5
    out = []
    for off in (-0.2, 0.2):
        disc = (xx - ((W - 1) / 2 + off * max(W, H))) ** 2 + (yy - (H - 1) / 2) ** 2 <= r * r
        img = rng.normal(size=(P, H, W, 4)).astype(np.float32)
        img[..., 3] = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], np.float32), size=(P, H, W)) * disc
        img[..., 0] = rng.integers(-4, 25, size=(P, H, W)).astype(np.float32) * np.float32(0.25) * disc
        out.append(img)
    sensor = rng.integers(0, 25, size=(P, H, W)).astype(np.uint16)  # raw counts; sensor_q = 1/4 makes quarter-integers
    sensor[rng.random((P, H, W)) < 0.15] = 0
    ray = (1.0 + 0.25 * rng.integers(0, 5, size=(H, W))).astype(np.float32)
    return out[0], out[1], sensor, ray


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (-3, 2)])
@pytest.mark.parametrize("with_ray", [False, True])
def test_the_restatement_is_bops_vsd(shift, with_ray):
    W, H, P = 37, 23, 4
    est, gt, sensor, ray = _seeded(W, H, P, 5)
    ray = ray if with_ray else None
    delta, taus = 0.25 + 0.125, [0.25 * k + 0.125 for k in range(10)]  # offset by an eighth: nothing is borderline
    rec, sums = SE.sensor_vsd_reference(est, gt, sensor, ray, shift, MIN_ALPHA, 0.25, delta, taus)
    fig = SE.sensor_frame_figures(rec, 1.0, sums=sums)
    r64 = np.ones((H, W)) if ray is None else ray.astype(np.float64)
    raw = SE.shifted_sensor(sensor, shift)
    assert (raw == 0).any() and (raw != 0).any()
    for p in range(P):
        dist = []
        for img in (est[p].astype(np.float64), gt[p].astype(np.float64)):
            with np.errstate(all="ignore"):
                on = (img[..., 3] >= MIN_ALPHA) & (img[..., 0] > 0)
                dist.append(np.where(on, img[..., 0] / np.where(on, img[..., 3], 1.0) * r64, 0.0))
        dist_test = raw[p].astype(np.float64) * 0.25 * r64
        errors, n_gt, n_est, n_inter, n_union = _bop_vsd(dist[0], dist[1], dist_test, delta, taus)
        assert (int(rec[p, 0]), int(rec[p, 1]), int(rec[p, 2]), int(rec[p, 3])) == (n_est, n_gt, n_inter, n_union)
        assert n_inter > 20 and n_union > n_inter
        np.testing.assert_array_equal(fig["vsd"][p], np.asarray(errors))
        assert rec[p, 6] == 10 and rec[p, 7] == 1 and (rec[p, 11:16] == 0).all() and (rec[p, 26:] == 0).all()
        assert rec[p, 10] == (raw[p] != 0).sum()


def test_a_hand_checked_occlusion_scene():
    W = H = 32
    yy, xx = np.mgrid[0:H, 0:W]
    disc_g = (xx - 13) ** 2 + (yy - 16) ** 2 <= 64
    disc_e = (xx - 18) ** 2 + (yy - 16) ** 2 <= 64
    slab, row = xx < 10, yy == 16
    assert (disc_g & slab & ~row).sum() > 0 and (disc_g & disc_e).sum() > 0 and (disc_e & ~disc_g).sum() > 0
    gt, est = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    gt[disc_g, 0], gt[disc_g, 3] = 2.0, 1.0
    est[disc_e, 0], est[disc_e, 3] = 2.5, 1.0     # deeper than the ground truth (and the sensor) by 0.5 > delta
    counts = np.full((H, W), 1000, np.uint16)     # far background at 10.0
    counts[disc_g] = 200                          # the object where the sensor sees it: 2.0
    counts[slab] = 100                            # the occluder at 1.0
    counts[row] = 0                               # a row without a measurement
    delta, taus = 0.1, [0.25, 0.75]
    rec, _ = SE.sensor_vsd_reference(est, gt, counts, None, (0, 0), MIN_ALPHA, 0.01, delta, taus)
    fig = SE.sensor_frame_figures(rec, 1.0)
    # pixels behind the slab leave vis_g, raw == 0 pixels count as visible (behind the slab too)
    vis_g = disc_g & (~slab | row)
    assert rec[0, 9] == disc_g.sum() and rec[0, 1] == vis_g.sum() < disc_g.sum()
    assert (disc_g & slab & row).sum() > 0
    # an estimate deeper than the sensor by more than delta is still visible through vis_g && sil(e); off the ground
    # truth it is in front of the background, or on the row without a measurement
    vis_e = disc_e & (vis_g | ~slab | row)
    assert rec[0, 8] == disc_e.sum() and rec[0, 0] == vis_e.sum()
    assert (vis_g & disc_e).sum() > 0 and rec[0, 2] == (vis_g & vis_e).sum() == (vis_g & disc_e).sum()
    assert rec[0, 3] == (vis_g | vis_e).sum()
    # visib_fract is the counted ratio
    assert fig["visib_fract"][0] == vis_g.sum() / disc_g.sum() and 0 < fig["visib_fract"][0] < 1
    # |dd| = 0.5 on the intersection: beyond tau 0.25, within 0.75
    n_inter, n_union = int(rec[0, 2]), int(rec[0, 3])
    assert rec[0, 16] == 0 and rec[0, 17] == n_inter
    np.testing.assert_array_equal(fig["vsd"][0], [1.0, (n_union - n_inter) / n_union])
    assert rec[0, 5] == np.float32(0.5).view(np.uint32) and fig["max_abs_dd"][0] == 0.5
    # without the occluder every ground-truth pixel is visible
    rec2, _ = SE.sensor_vsd_reference(est, gt, np.where(slab & ~disc_g, 1000, np.where(disc_g, 200, counts)).astype(np.uint16),
                                      None, (0, 0), MIN_ALPHA, 0.01, delta, taus)
    assert SE.sensor_frame_figures(rec2, 1.0)["visib_fract"][0] == 1.0


def test_a_shift_that_leaves_the_image_reads_nothing():
    est, gt, sensor, ray = _seeded(9, 4, 2, 8)
    rec, _ = SE.sensor_vsd_reference(est, gt, sensor, ray, (9, 0), MIN_ALPHA, 0.25, 0.375, [0.5])
    assert (rec[:, 10] == 0).all() and (rec[:, 0] == rec[:, 8]).all() and (rec[:, 1] == rec[:, 9]).all()
    np.testing.assert_array_equal(SE.shifted_sensor(sensor, (1, -1))[:, 1:, :-1], sensor[:, :-1, 1:])
    assert (SE.shifted_sensor(sensor, (1, -1))[:, 0] == 0).all() and (SE.shifted_sensor(sensor, (1, -1))[:, :, -1] == 0).all()


# ------------------------------------------------------------------------------------------------------ the camera
def _camera(W, H, fx, fy, cx, cy):
    return Camera.from_colmap(dict(model="PINHOLE", width=W, height=H, params=[fx, fy, cx, cy]))


def test_ray_factors():
    cam = _camera(33, 21, 40.0, 40.0, 16.5, 10.5)
    r = SE.ray_factors(cam)
    assert r.dtype == np.float32 and r.shape == (21, 33)
    assert r[10, 16] == 1.0  # the centre pixel of an odd-sized image looks along the axis
    np.testing.assert_array_equal(r, r[::-1])
    np.testing.assert_array_equal(r, r[:, ::-1])
    f = float(cam.f[0])
    yy, xx = np.mgrid[0:21, 0:33].astype(np.float64)
    want = np.sqrt(1.0 + ((xx + 0.5 - 16.5) / f) ** 2 + ((yy + 0.5 - 10.5) / f) ** 2).astype(np.float32)
    np.testing.assert_array_equal(r, want)
    assert r.max() == r[0, 0] > 1.0
    # the principal point and fy play no part: the renderer ignores them
    np.testing.assert_array_equal(SE.ray_factors(_camera(33, 21, 40.0, 55.0, 3.0, 4.0)), r)


def test_sensor_alignment():
    assert SE.sensor_alignment(_camera(640, 480, 600.0, 600.0, 320.0, 240.0)) == (0, 0, 0.0)
    ycb = _camera(640, 480, 1066.778, 1067.487, 312.99, 241.31)
    sx, sy, res = SE.sensor_alignment(ycb)
    assert (sx, sy) == (round(312.99 - 320), round(241.31 - 240)) == (-7, 1)
    assert res == pytest.approx(0.31 + abs(1067.487 / 1066.778 - 1) * 240, abs=1e-3) and res < 1
    assert SE.check_alignment(ycb) == (sx, sy, res)
    off = _camera(640, 480, 600.0, 606.0, 320.0, 240.0)  # 1 % of 240 px = 2.4 px at the border
    assert SE.sensor_alignment(off)[2] == pytest.approx(2.4, abs=1e-3)
    with pytest.raises(ValueError):
        SE.check_alignment(off)
    assert SE.check_alignment(off, allow_misaligned=True)[2] == pytest.approx(2.4, abs=1e-3)


# ------------------------------------------------------------------------------------------------------ files
def test_read_sensor_depth(tmp_path):
    from PIL import Image

    a = (np.arange(7 * 5, dtype=np.uint32).reshape(5, 7) * 1871 % 65536).astype(np.uint16)
    a[0, 0], a[4, 6] = 0, 65535
    Image.fromarray(a).save(tmp_path / "d.png")
    np.save(tmp_path / "d.npy", a)
    for name in ("d.png", "d.npy"):
        got = SE.read_sensor_depth(tmp_path / name, size=(7, 5))
        assert got.dtype == np.uint16
        np.testing.assert_array_equal(got, a)
        with pytest.raises(ValueError):
            SE.read_sensor_depth(tmp_path / name, size=(5, 7))
    Image.fromarray((a >> 8).astype(np.uint8)).save(tmp_path / "u8.png")
    np.save(tmp_path / "u8.npy", (a >> 8).astype(np.uint8))
    np.save(tmp_path / "f.npy", a.astype(np.float32))
    Image.fromarray(a.astype(np.float32)).save(tmp_path / "f.tiff")
    for name in ("u8.png", "u8.npy", "f.npy", "f.tiff"):
        with pytest.raises(ValueError):
            SE.read_sensor_depth(tmp_path / name)


# ------------------------------------------------------------------------------------------------------ figures
def test_figures_and_summary_conventions():
    rec = np.zeros((4, SE.RECORD), np.uint32)
    rec[:, 6], rec[:, 7] = 2, 1
    rec[1, [0, 1, 2, 3, 8, 9]] = [6, 8, 4, 10, 6, 16]   # half the silhouette visible
    rec[1, 16:18] = [1, 3]
    rec[2, [0, 1, 2, 3, 8, 9]] = [5, 1, 1, 5, 5, 20]    # a twentieth visible
    rec[2, 16:18] = [1, 1]
    rec[3, [0, 3, 8]] = [7, 7, 7]                       # the ground truth is nowhere: vsd 1, visib_fract 0
    fig = SE.sensor_frame_figures(rec, 2.0)
    np.testing.assert_array_equal(fig["vsd"], [[1, 1], [0.9, 0.7], [0.8, 0.8], [1, 1]])
    np.testing.assert_array_equal(fig["visib_fract"], [0, 0.5, 0.05, 0])
    assert fig["ok"].all() and list(fig["n_vis_gt"]) == [0, 8, 1, 0] and list(fig["n_sil_gt"]) == [0, 16, 20, 0]
    # frame 2 is below the cut and leaves the recall; frame 0 is a lost frame whose visibility is unknown: a miss
    vsd = np.array([[1.0, 1.0], [0.04, 0.04], [0.04, 0.04], [0.04, 0.04]])
    vf = np.array([0.0, 0.5, 0.05, 0.9])
    s = SE.summarize_sensor(vsd, vf, [False, True, True, True], [False, True, True, True], 0.1)
    assert s["n_below_visibility"] == 1 and s["ar_vsd_sensor"] == pytest.approx(2 / 3)
    assert s["visib_fract_mean"] == pytest.approx((0.5 + 0.05 + 0.9) / 3) and s["vsd_sensor_mean"] == [0.04, 0.04]
    # a lost frame above the cut is a miss, one below it is left out
    s = SE.summarize_sensor(vsd, [0.05, 0.5, 0.5, 0.9], [False, True, True, True], [True] * 4, 0.1)
    assert s["n_below_visibility"] == 1 and s["ar_vsd_sensor"] == 1.0
    s = SE.summarize_sensor(vsd, [0.5, 0.5, 0.5, 0.9], [False, True, True, True], [True] * 4, 0.1)
    assert s["n_below_visibility"] == 0 and s["ar_vsd_sensor"] == 0.75


# ------------------------------------------------------------------------------------------------------ command line
def test_the_parser_and_the_file_names(capsys):
    ap = SE.build_parser()
    base = ["--poses", "p.pkl", "--object_path", "obj", "--sensor_depth_dir", "D"]
    with pytest.raises(SystemExit):
        ap.parse_args(base)
    capsys.readouterr()
    args = ap.parse_args(base + ["--sensor_depth_scale", "0.0001"])
    assert args.sensor_depth_scale == 1e-4 and args.delta == 0.015 and args.min_visib_fract == 0.1
    assert args.sensor_depth_template == "{stem}.png" and args.sensor_depth_sub is None and not args.allow_misaligned
    assert not args.bop and args.spp == 8  # render_evaluation's arguments are all there
    args = ap.parse_args(base + ["--sensor_depth_scale", "1", "--sensor_depth_sub", "color", "depth", "--bop",
                                 "--allow_misaligned", "--sensor_depth_template", "{stem}.npy"])
    assert args.sensor_depth_sub == ["color", "depth"] and args.bop and args.allow_misaligned
    assert SE.sensor_file_name("000001-color.png", args.sensor_depth_template, args.sensor_depth_sub) == "000001-depth.npy"
    assert SE.sensor_file_name("seq/000007.jpg") == "000007.png"
    assert SE.sensor_file_name("000007.jpg", "depth_{name}") == "depth_000007.jpg"


def test_the_header_declares_both_symbols():
    text = (ROOT / "include" / "pixtrack_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("pxt_sensor_vsd_workspace_bytes", "pxt_sensor_vsd"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
    from pixtrack_amd import _lib

    assert "pxt_sensor_vsd" in _lib.PROTOTYPES and "pxt_sensor_vsd_workspace_bytes" in _lib.PROTOTYPES
    assert re.search(r"#define\s+PXT_SENSOR_VSD_RECORD\s+32\b", text) and _lib.PXT_SENSOR_VSD_RECORD == SE.RECORD == 32
    assert _lib.ABI_VERSION == 13  # added entry points keep the version
