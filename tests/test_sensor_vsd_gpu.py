"""pxt_sensor_vsd (csrc/pxt_eval_vsd.hip) / torch.ops.pixtrack.sensor_vsd and the sensor-depth evaluation on top of it
(pixtrack_amd/sensor_evaluation.py): P pairs of Depth images compared with each other and with the frames' sensor depth
images in one call - BOP's occlusion-aware VSD and the visible fraction.

Oracle: sensor_evaluation.sensor_vsd_reference, a numpy float32 restatement of the per-pixel rules (itself held to a
float64 transcription of BOP's vsd in tests/test_sensor_vsd_host.py).  Division, multiplication, subtraction and
comparison are single IEEE operations on both sides and the counts are integers, so every word but the float sum is
compared BIT FOR BIT, with no tolerance and no pixel left out.

The float sum (word 4) depends on the order of the additions.  Bar (the project's convention): the
largest relative error, against the float64 sum of the same float32 terms, of a plain float32 pairwise sum (np.sum) over
the very inputs of test 1; the kernel may be 4 x that off.
Measured (seeded inputs below, 9 shapes x 17 pairs x 2 ray planes x 4 shifts): restatement max 1.115e-07 -> bar 4.461e-07;
the kernel on an MI355X 1.298e-07.  Both figures are printed before the assertion (pytest -s).

What six synthetic 160 x 120 frames score behind a slab over the object's left third (printed, nothing absolute is
asserted): visib_fract 0.696 ... 0.699; estimates 3 degrees / 2 % of the diameter off: vsd 0.065 at the smallest tau and
0.059 from the second on."""
import ctypes

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, ops
from pixtrack_amd import render_evaluation as RE
from pixtrack_amd import sensor_evaluation as SE

pytestmark = pytest.mark.gpu

SHARE = 1024  # pixels of one workgroup (csrc/pxt_eval_vsd.hip: 256 lanes x 4)
# one pixel, odd sizes, one wave exactly, a partial wave over rows, rows longer than a wavefront's load, many blocks;
# one pixel below / one above one workgroup's share; three blocks with a one-pixel tail
SHAPES = ((1, 1), (7, 5), (64, 1), (63, 3), (257, 3), (160, 120), (SHARE - 1, 1), (SHARE + 1, 1), (2 * SHARE + 1, 1))
PAIRS = (1, 3, 17)
NTAUS = (1, 10, 16)
PMAX = max(PAIRS)
MIN_ALPHA = 0.5
SENSOR_Q = 0.25   # a raw count is a quarter: quarter-integer sensor depths
DELTA_Q = 0.25    # like most d - d_s: many equal it exactly
TQ = [0.25 * (k + 1) for k in range(16)]  # quarter-integers, like most of the dd values: many dd == tq exactly
SENTINEL = -777
GUARD = 4099      # odd: the sensor array behind it is 2-byte aligned and no more
GUARD_VALUE = 0x5A5A
REC = 32
EXACT_WORDS = [0, 1, 2, 3] + list(range(5, 32))


def _shifts(W):
    return ((0, 0), (1, 0), (-3, 2), (W, 0))  # the last one puts every sensor pixel outside the image


def _inputs(W, H, seed):
    """PMAX seeded pairs: two overlapping discs offset from each other; inside a disc alpha is drawn from {0, 0.25, 0.5,
    0.75, 1} and channel 0 from the quarter-integers of [-1, 6] (0 and negatives included), outside both are 0; the two
    middle channels hold noise; raw sensor counts from 0 ... 24 (a seventh of them forced to 0: no measurement); a ray
    plane of quarter-integers in [1, 2]; one pixel of every pair has an infinite estimated depth, one a NaN alpha."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.45 * max(W, H) + 0.5
    out = []
    for off in (-0.2, 0.2):
        cx, cy = (W - 1) / 2 + off * max(W, H), (H - 1) / 2
        disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        img = rng.normal(size=(PMAX, H, W, 4)).astype(np.float32)
        img[..., 3] = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], np.float32), size=(PMAX, H, W)) * disc
        img[..., 0] = rng.integers(-4, 25, size=(PMAX, H, W)).astype(np.float32) * np.float32(0.25) * disc
        out.append(img)
    est, gt = out
    sensor = rng.integers(0, 25, size=(PMAX, H, W)).astype(np.uint16)
    sensor[rng.random((PMAX, H, W)) < 1 / 7] = 0
    ray = (1.0 + 0.25 * rng.integers(0, 5, size=(H, W))).astype(np.float32)
    iy, ix = (H - 1) // 2, (W - 1) // 2  # inside both discs
    est[:, iy, ix, 0], est[:, iy, ix, 3] = np.inf, 1.0
    # a ground truth nearer than any measured count can hide: visible whatever the shift brings there, and the estimate
    # through it, so the inf pixel is an `inter` pixel of every case
    gt[:, iy, ix, 0], gt[:, iy, ix, 3] = 0.25, 1.0
    if W * H > 1:
        jy, jx = divmod((iy * W + ix + 1) % (W * H), W)
        est[:, jy, jx, 3] = np.nan
    return est, gt, sensor, ray


def _terms(est, gt, sensor, ray, shift):
    """The float32 terms of pair sums: dd on the `inter` pixels where it is finite, else 0 ([P, H * W])."""
    P, H, W = sensor.shape
    r = np.ones((H, W), np.float32) if ray is None else ray
    raw = SE.shifted_sensor(sensor, shift)
    ma, sq, dq = np.float32(MIN_ALPHA), np.float32(SENSOR_Q), np.float32(DELTA_Q)
    with np.errstate(all="ignore"):
        sil = [(a[..., 3] >= ma) & (a[..., 0] > 0) for a in (est, gt)]
        d_e, d_g = (est[..., 0] / est[..., 3]) * r, (gt[..., 0] / gt[..., 3]) * r
        d_s = (raw.astype(np.float32) * sq) * r
        vis_g = sil[1] & (((d_g - d_s) <= dq) | (raw == 0))
        vis_e = sil[0] & (((d_e - d_s) <= dq) | (raw == 0) | vis_g)
        dd = np.abs(d_e - d_g)
    keep = vis_g & vis_e & np.isfinite(dd)
    return np.where(keep, dd, np.float32(0)).reshape(P, -1)


def _guarded(sensor, device):
    """The sensor counts on the device, allocated exactly between two guard arrays -> (whole buffer, the sensor view)."""
    n = sensor.size
    whole = torch.full((GUARD + n + GUARD,), GUARD_VALUE, dtype=torch.int16, device=device)
    view = whole[GUARD:GUARD + n].view(*sensor.shape)
    view.copy_(torch.from_numpy(sensor.view(np.int16)).to(device))
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    return whole, view


def _guards_untouched(whole):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == GUARD_VALUE).all() and (h[-GUARD:] == GUARD_VALUE).all())


@pytest.fixture(scope="module")
def refs(device):
    """Per shape: the inputs on the host and on the device (the sensor array between its guards), the oracle's records
    and float64 sums of PMAX pairs and 16 thresholds for every (ray, shift) (a pair's record does not depend on the other
    pairs; fewer thresholds are a prefix); and the bar."""
    out, worst = {}, 0.0
    for n, (W, H) in enumerate(SHAPES):
        est, gt, sensor, ray = _inputs(W, H, 500 + n)
        whole, d_sensor = _guarded(sensor, device)
        r = dict(est=est, gt=gt, sensor=sensor, ray=ray, d_est=torch.from_numpy(est).to(device),
                 d_gt=torch.from_numpy(gt).to(device), d_sensor=d_sensor, whole=whole,
                 d_ray=torch.from_numpy(ray).to(device), rec={}, sums={})
        for with_ray in (False, True):
            for shift in _shifts(W):
                rp = ray if with_ray else None
                rec, sums = SE.sensor_vsd_reference(est, gt, sensor, rp, shift, MIN_ALPHA, SENSOR_Q, DELTA_Q, TQ)
                terms = _terms(est, gt, sensor, rp, shift)
                assert terms.dtype == np.float32 and np.array_equal(terms.astype(np.float64).sum(axis=1), sums)
                pairwise = np.array([np.sum(t) for t in terms], np.float64)  # float32 pairwise sums
                have = sums > 0
                if have.any():
                    worst = max(worst, float((np.abs(pairwise[have] - sums[have]) / sums[have]).max()))
                assert (rec[:, 2] >= 1).all()  # (the inf pixel at least)
                r["rec"][(with_ray, shift)], r["sums"][(with_ray, shift)] = rec, sums
        assert (r["rec"][(False, (W, 0))][:, 10] == 0).all()
        out[(W, H)] = r
    out["restatement"] = worst
    out["bar"] = 4.0 * worst
    print(f"float32 pairwise restatement: max relative error {worst:.3e}; bar {4 * worst:.3e}")
    assert 0 < out["bar"] < 1e-5  # a float32 sum of a few thousand terms
    return out


def _run(device, d_est, d_gt, d_sensor, d_ray, shift, tq, records=None, min_alpha=MIN_ALPHA, sensor_q=SENSOR_Q,
         delta_q=DELTA_Q):
    """One call of the op; -> the records (uint32 [P, 32], host)."""
    P, H, W = (int(x) for x in d_est.shape[:3])
    if records is None:
        records = torch.full((P, REC), SENTINEL, dtype=torch.int32, device=device)
    ws = torch.empty(int(_lib.lib().pxt_sensor_vsd_workspace_bytes(P, W, H)), dtype=torch.uint8, device=device)
    ops.ops.sensor_vsd(d_est, d_gt, d_sensor, d_ray, list(shift), min_alpha, sensor_q, delta_q, tq, records, ws)
    return records.cpu().numpy().view(np.uint32)


def _want(rec, P, n_taus):
    w = rec[:P].copy()
    w[:, 6] = n_taus
    w[:, 16 + n_taus:] = 0
    return w


# ------------------------------------------------------------------------------------------------ 1. exact records
@pytest.mark.parametrize("n_taus", NTAUS)
@pytest.mark.parametrize("P", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_equal_the_restatement_bit_for_bit(device, refs, shape, P, n_taus):
    r = refs[shape]
    for with_ray in (False, True):
        for shift in _shifts(shape[0]):
            got = _run(device, r["d_est"][:P], r["d_gt"][:P], r["d_sensor"][:P], r["d_ray"] if with_ray else None, shift,
                       TQ[:n_taus])
            want = _want(r["rec"][(with_ray, shift)], P, n_taus)
            np.testing.assert_array_equal(got[:, EXACT_WORDS], want[:, EXACT_WORDS], err_msg=f"{with_ray} {shift}")
            assert (got[:, 2] <= np.minimum(got[:, 0], got[:, 1])).all()
            assert (got[:, 0] <= got[:, 8]).all() and (got[:, 1] <= got[:, 9]).all()
            assert (np.diff(got[:, 16:16 + n_taus].astype(np.int64), axis=1) >= 0).all()  # nested thresholds
            assert (got[:, 16 + n_taus - 1] < got[:, 2]).all()  # the inf pixel is within none
    assert _guards_untouched(r["whole"])


# ------------------------------------------------------------------------------------------------ 2. the float sum
def test_the_float_sum_stays_within_four_pairwise_errors(device, refs):
    worst = 0.0
    for shape in SHAPES:
        r = refs[shape]
        for with_ray in (False, True):
            for shift in _shifts(shape[0]):
                sums = r["sums"][(with_ray, shift)]
                got = _run(device, r["d_est"], r["d_gt"], r["d_sensor"], r["d_ray"] if with_ray else None, shift, TQ)
                got = got[:, 4].copy().view(np.float32).astype(np.float64)
                have = sums > 0
                assert (got[~have] == 0.0).all()
                if have.any():
                    worst = max(worst, float((np.abs(got[have] - sums[have]) / sums[have]).max()))
        print(f"{shape}: kernel sum max relative error so far {worst:.3e}")
    print(f"kernel sum: max relative error {worst:.3e}; float32 pairwise restatement {refs['restatement']:.3e}; "
          f"bar {refs['bar']:.3e}")
    assert worst <= refs["bar"], (worst, refs["bar"])


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("shape", ((160, 120), (2 * SHARE + 1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_record_depends_on_its_own_pair_only(device, refs, shape):
    r = refs[shape]
    shift = (1, 0)
    args = (r["d_ray"], shift, TQ)
    base = _run(device, r["d_est"], r["d_gt"], r["d_sensor"], *args)
    want = r["rec"][(True, shift)]
    np.testing.assert_array_equal(base[:, EXACT_WORDS], want[:, EXACT_WORDS])
    perm = np.random.default_rng(9).permutation(PMAX)
    idx = torch.from_numpy(perm).to(device)
    got = _run(device, r["d_est"][idx].contiguous(), r["d_gt"][idx].contiguous(), r["d_sensor"][idx].contiguous(), *args)
    np.testing.assert_array_equal(got, base[perm])
    for k in range(PMAX):
        one = _run(device, r["d_est"][k:k + 1], r["d_gt"][k:k + 1], r["d_sensor"][k:k + 1], *args)
        np.testing.assert_array_equal(one, base[k:k + 1])
    outs = [torch.full((PMAX, REC), SENTINEL, dtype=torch.int32, device=device) for _ in range(10)]
    ws = torch.empty(int(_lib.lib().pxt_sensor_vsd_workspace_bytes(PMAX, *shape)), dtype=torch.uint8, device=device)
    for o in outs:
        ops.ops.sensor_vsd(r["d_est"], r["d_gt"], r["d_sensor"], r["d_ray"], list(shift), MIN_ALPHA, SENSOR_Q, DELTA_Q, TQ,
                           o, ws)
    torch.cuda.synchronize(device)
    for o in outs:
        np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), base)
    assert _guards_untouched(r["whole"])


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_bad_arguments_are_refused_and_nothing_is_written(device, refs):
    r = refs[(63, 3)]
    L = _lib.lib()
    est, gt, sen, ray = r["d_est"][:3], r["d_gt"][:3], r["d_sensor"][:3], r["d_ray"]
    rec = torch.full((3, REC), SENTINEL, dtype=torch.int32, device=device)
    ws = torch.full((1 << 16,), 0xAB, dtype=torch.uint8, device=device)
    tq = (ctypes.c_float * 17)(*([0.5] * 17))
    s = _lib.stream_ptr(device)
    #     0 est            1 gt            2 sensor        3 ray          4 P 5 W 6 H 7 sx 8 sy 9 min_alpha 10 11    12  13
    a = (est.data_ptr(), gt.data_ptr(), sen.data_ptr(), ray.data_ptr(), 3, 63, 3, 1, 0, MIN_ALPHA, SENSOR_Q, DELTA_Q, tq, 10,
         rec.data_ptr(), ws.data_ptr(), s)  # 14 records 15 workspace 16 stream

    def call(**kw):
        args = list(a)
        for i, val in kw.items():
            args[int(i[1:])] = val
        return L.pxt_sensor_vsd(*args)

    cases = (dict(_4=0), dict(_4=65536), dict(_13=0), dict(_13=17), dict(_13=-1), dict(_5=0), dict(_6=0),
             dict(_5=1 << 15, _6=(1 << 13) + 1),                                       # W * H > 2^28
             dict(_0=est.data_ptr() + 4), dict(_1=gt.data_ptr() + 8), dict(_15=ws.data_ptr() + 8),  # 16-byte alignment
             dict(_2=sen.data_ptr() + 1), dict(_3=ray.data_ptr() + 2), dict(_14=rec.data_ptr() + 2),
             dict(_7=32768), dict(_7=-32768), dict(_8=32768), dict(_8=-32768),          # |shift| <= 32767
             dict(_2=None),                                                             # a NULL sensor
             dict(_0=None), dict(_1=None), dict(_12=None), dict(_14=None), dict(_15=None))
    for kw in cases:
        assert call(**kw) == -1, kw  # PXT_E_ARG
        with pytest.raises(_lib.PxtError):
            _lib.check(call(**kw), "pxt_sensor_vsd")
    for fn_args in ((0, 63, 3), (65536, 63, 3), (3, 0, 3), (3, 63, 0), (3, 1 << 15, (1 << 13) + 1)):
        assert L.pxt_sensor_vsd_workspace_bytes(*fn_args) < 0
    assert L.pxt_sensor_vsd_workspace_bytes(3, 63, 3) == 3 * 1 * REC * 4
    torch.cuda.synchronize(device)
    assert (rec.cpu() == SENTINEL).all() and (ws.cpu() == 0xAB).all()
    assert call() == 0 and call(_3=None) == 0 and call(_7=32767, _8=-32767) == 0
    assert call() == 0
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(rec.cpu().numpy().view(np.uint32), _run(device, est, gt, sen, ray, (1, 0), [0.5] * 10))
    assert _guards_untouched(r["whole"])


def test_the_op_checks_before_any_launch(device, refs):
    r = refs[(63, 3)]
    est, gt, sen, ray = r["d_est"][:3], r["d_gt"][:3], r["d_sensor"][:3], r["d_ray"]
    rec = torch.full((3, REC), SENTINEL, dtype=torch.int32, device=device)
    ws = torch.full((1 << 16,), 0xAB, dtype=torch.uint8, device=device)
    need = int(_lib.lib().pxt_sensor_vsd_workspace_bytes(3, 63, 3))

    def op(est=est, gt=gt, sen=sen, ray=ray, shift=(0, 0), tq=TQ, rec=rec, ws=ws):
        ops.ops.sensor_vsd(est, gt, sen, ray, list(shift), MIN_ALPHA, SENSOR_Q, DELTA_Q, tq, rec, ws)

    bad = (dict(tq=[]), dict(tq=[0.5] * 17), dict(est=est[:0], gt=gt[:0], sen=sen[:0], rec=rec[:0]), dict(gt=gt[:2]),
           dict(rec=rec[:2]), dict(rec=rec.float()), dict(est=est[..., :3], gt=gt[..., :3]),
           dict(sen=sen[:2]), dict(sen=sen.to(torch.int32)), dict(sen=sen.float()), dict(sen=sen[:, :, :62]),
           dict(ray=ray[:2]), dict(ray=ray.double()), dict(shift=(0,)), dict(shift=(40000, 0)),
           dict(ws=ws[:need - 1]), dict(ws=ws.to(torch.int8)),
           dict(ws=ws.cpu()), dict(sen=sen.cpu()), dict(ray=ray.cpu()), dict(rec=rec.cpu()), dict(gt=gt.cpu()))
    for kw in bad:
        with pytest.raises(_lib.PxtError):
            op(**kw)
    with pytest.raises((RuntimeError, NotImplementedError)):  # no kernel is registered for host tensors
        op(est=est.cpu(), gt=gt.cpu(), sen=sen.cpu(), ray=ray.cpu(), rec=rec.cpu(), ws=ws.cpu())
    torch.cuda.synchronize(device)
    assert (rec.cpu() == SENTINEL).all() and (ws.cpu() == 0xAB).all()
    op(ws=ws[:need])
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(rec.cpu().numpy().view(np.uint32)[:, EXACT_WORDS],
                                  r["rec"][(True, (0, 0))][:3][:, EXACT_WORDS])


# ------------------------------------------------------------------------------------------------ 5. real renders
W, H, N = 160, 120, 6
MAX_COUNT = 20000  # the farthest object pixel of the made-up sensor; its background stands at three times that


@pytest.fixture(scope="module")
def run(device):
    """Built once: synthetic assets, an r9 tracker over them, its six-frame run with ground truth attached, the query
    camera, the diameter, the Depth renders at the ground-truth poses and two sensor images per frame made of them: the
    ground truth's ray length, a far background, and (``occluded``) a slab in front of the left third of the object (the
    object covers a tenth of the image around its centre: a slab over the image's left third would hide nothing)."""
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
    gt_images = _renders(tr, camera, T_gt, device)
    zs = RE.z_scale(tr.testbed, tr.nerf2sfm)
    sx, sy, _ = SE.sensor_alignment(camera)
    g = gt_images.cpu().numpy()
    on = (g[..., 3] >= MIN_ALPHA) & (g[..., 0] > 0)
    with np.errstate(all="ignore"):
        length = np.where(on, g[..., 0] / np.where(on, g[..., 3], 1) * zs * SE.ray_factors(camera), 0.0)
    depth_scale = float(length.max() / MAX_COUNT)  # SfM units per raw count
    counts = np.rint(length / depth_scale)
    # the sensor's quantisation stays far below the visibility tolerance
    assert counts[on].min() > 100 and counts.max() == MAX_COUNT and depth_scale < 0.1 * SE.DEFAULT_DELTA
    free = np.where(on, counts, 3 * counts.max()).astype(np.uint16)  # the object in front of a far background
    occluded = free.copy()
    for k in range(N):  # a slab in front of the object's left third (and of everything left of it)
        cols = np.nonzero(on[k].any(axis=0))[0]
        occluded[k, :, :cols[0] + (cols[-1] - cols[0] + 1) // 3] = int(counts[on].min() // 2)
    to_sensor = lambda im: SE.shifted_sensor(im, (-sx, -sy))         # render pixel (x, y) -> sensor pixel (x + sx, y + sy)
    return dict(assets=assets, tr=tr, names=names, T_gt=T_gt, camera=camera, diameter=diameter, gt_images=gt_images,
                zs=zs, shift=(sx, sy), depth_scale=depth_scale, free=to_sensor(free), occluded=to_sensor(occluded))


def _renders(tr, camera, T, device):
    out = torch.empty(len(T), H, W, 4, dtype=torch.float32, device=device)
    for k in range(len(T)):
        RE._render_depth(tr.testbed, tr.nerf2sfm, T[k], camera, 8, out[k])
    return out


def _restated(run, est, sensor, d, delta=SE.DEFAULT_DELTA):
    """The restatement of the downloaded images with the scalars sensor_pose_errors forms."""
    zs = run["zs"]
    taus, tq = RE._thresholds(d, None, zs)
    return SE.sensor_vsd_reference(est.cpu().numpy(), run["gt_images"].cpu().numpy(), sensor, SE.ray_factors(run["camera"]),
                                   run["shift"], MIN_ALPHA, float(np.float32(run["depth_scale"] / zs)),
                                   float(np.float32(delta / zs)), tq)


def test_a_pose_agrees_with_itself_behind_an_occluder(device, run):
    tr, d = run["tr"], run["diameter"]
    kw = dict(sensor_depth_scale=run["depth_scale"], diameter=d)
    res = SE.sensor_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], run["T_gt"], run["T_gt"].copy(),
                                list(run["occluded"]), **kw)
    print("visib_fract", res["visib_fract"], "n_sil_gt", res["n_sil_gt"], "shift", res["shift"], res["residual_px"])
    assert res["ok"].all() and res["vsd"].shape == (N, 10) and (res["vsd"] == 0.0).all()
    assert (res["n_vis_est"] == res["n_vis_gt"]).all() and (res["n_vis_gt"] == res["n_inter"]).all()
    assert (res["n_inter"] == res["n_union"]).all() and (res["n_inter"] > 0).all()
    assert (res["mean_abs_dd"] == 0.0).all() and (res["max_abs_dd"] == 0.0).all()
    assert ((res["visib_fract"] > 0) & (res["visib_fract"] < 1)).all()
    want, _ = _restated(run, run["gt_images"], run["occluded"], d)
    fig = SE.sensor_frame_figures(want, run["zs"], n_taus=10, finite_slot=10)
    np.testing.assert_array_equal(res["visib_fract"], fig["visib_fract"])
    np.testing.assert_array_equal(res["n_vis_gt"], fig["n_vis_gt"])
    assert (want[:, 4] == 0).all() and (want[:, 5] == 0).all()  # +0.0, not -0.0
    # the slab removed: everything of the object is visible
    free = SE.sensor_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], run["T_gt"], run["T_gt"].copy(),
                                 list(run["free"]), **kw)
    assert (free["visib_fract"] == 1.0).all() and (free["vsd"] == 0.0).all()
    np.testing.assert_array_equal(free["n_sil_gt"], res["n_sil_gt"])
    assert (free["n_vis_gt"] == free["n_sil_gt"]).all() and (res["n_vis_gt"] < free["n_vis_gt"]).all()


def test_render_records_equal_the_restatement(device, run):
    from pixtrack_amd.synthetic import perturb_pose

    tr, d = run["tr"], run["diameter"]
    rng = np.random.default_rng(21)
    T_est = run["T_gt"].copy()
    for k in range(N):
        T_est[k, :3, :3], T_est[k, :3, 3] = perturb_pose(T_est[k, :3, :3], T_est[k, :3, 3], rng, 3.0, 0.02 * d,
                                                         run["assets"]["center"])
    est = _renders(tr, run["camera"], T_est, device)
    zs = run["zs"]
    taus, tq = RE._thresholds(d, None, zs)
    sensor = torch.from_numpy(run["occluded"].view(np.int16)).to(device)
    ray = torch.from_numpy(SE.ray_factors(run["camera"])).to(device)
    got = _run(device, est, run["gt_images"], sensor, ray, run["shift"], tq, sensor_q=float(np.float32(run["depth_scale"] / zs)),
               delta_q=float(np.float32(SE.DEFAULT_DELTA / zs)))
    want, sums = _restated(run, est, run["occluded"], d)
    np.testing.assert_array_equal(got[:, EXACT_WORDS], want[:, EXACT_WORDS])
    res = SE.sensor_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], T_est, run["T_gt"], list(run["occluded"]),
                                run["depth_scale"], d)
    fig = SE.sensor_frame_figures(got, zs, n_taus=10, finite_slot=10)
    for key in ("vsd", "visib_fract", "n_vis_est", "n_vis_gt", "n_inter", "n_union", "mean_abs_dd", "max_abs_dd"):
        np.testing.assert_array_equal(res[key], fig[key])
    print("3 deg / 2 % of the diameter behind the slab: vsd", res["vsd"].mean(axis=0), "visib_fract", res["visib_fract"],
          "mean |dd|", res["mean_abs_dd"], "diameter", d)
    assert (np.diff(res["vsd"], axis=1) <= 0).all() and (res["vsd"] > 0).all() and (res["vsd"][:, -1] < 1).all()
    # the occluder's pixels count neither for nor against: the union is smaller than the bare silhouettes' union
    bare = RE.render_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], T_est, run["T_gt"], d)
    assert (res["n_union"] < bare["n_union"]).all()
    # a non-finite pose is not rendered: a miss, and only that frame
    bad = T_est.copy()
    bad[2, 0, 3] = np.nan
    res2 = SE.sensor_pose_errors(tr.testbed, tr.nerf2sfm, [run["camera"]] * N, bad, run["T_gt"], list(run["occluded"]),
                                 run["depth_scale"], d)
    assert not res2["ok"][2] and (res2["vsd"][2] == 1).all() and res2["visib_fract"][2] == 0
    keep = [0, 1, 3, 4, 5]
    np.testing.assert_array_equal(res2["vsd"][keep], res["vsd"][keep])


def test_a_sideways_shift_by_one_diameter_scores_one(device, run):
    tr, d = run["tr"], run["diameter"]
    shifted = run["T_gt"].copy()
    shifted[:, 0, 3] += d  # along the camera's x axis
    off = SE.sensor_pose_errors(tr.testbed, tr.nerf2sfm, run["camera"], shifted, run["T_gt"], list(run["free"]),
                                run["depth_scale"], d)
    print("shifted by one diameter: n_inter", off["n_inter"], "n_union", off["n_union"], "vsd", off["vsd"][:, -1])
    assert (off["vsd"] == 1.0).all() and off["ok"].all() and (off["visib_fract"] == 1.0).all()


def test_the_command_line_adds_the_sensor_keys(device, run, tmp_path, capsys):
    import json

    from PIL import Image

    from pixtrack_amd.synthetic import write_object_dir
    from pixtrack_amd.utils.io import dump_reference_pickle

    obj = tmp_path / "object"
    write_object_dir(run["assets"], obj)
    poses = dict(run["tr"].pose_history)
    poses[run["names"][3]] = dict(poses[run["names"][3]], success=False)  # one lost frame: a miss above the cut
    dump_reference_pickle(poses, str(tmp_path / "poses.pkl"))
    (tmp_path / "depth").mkdir()
    for name, img in zip(run["names"], run["occluded"]):
        Image.fromarray(img).save(tmp_path / "depth" / (name[:-4] + "-depth.png"))
    aabb = [[float(x) for x in c] for c in run["assets"]["aabb"]]
    common = ["--poses", str(tmp_path / "poses.pkl"), "--object_path", str(obj), "--obj_aabb", json.dumps(aabb),
              "--device", str(device)]
    sensor = ["--sensor_depth_dir", str(tmp_path / "depth"), "--sensor_depth_template", "{stem}-depth.png",
              "--sensor_depth_scale", str(run["depth_scale"])]
    RE.main(common)
    before = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    res = SE.main(common + sensor + ["--json", str(tmp_path / "out.json")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(line)
    for key in ("vsd_sensor_mean", "visib_fract_mean", "n_below_visibility", "ar_vsd_sensor"):
        assert key in line and key not in before
    same = lambda a, b: json.dumps({k: a[k] for k in b}, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert same(line, before) and "ar_bop_sensor" not in line and "frames" not in line
    assert 0 < line["ar_vsd_sensor"] <= (N - 1) / N and line["n_below_visibility"] == 0 and line["n_evaluated"] == N - 1
    assert 0 < line["visib_fract_mean"] < 1 and len(line["vsd_sensor_mean"]) == 10
    lost = res["frames"][run["names"][3]]
    assert lost["vsd_sensor"] == [1.0] * 10 and 0 < lost["visib_fract"] < 1 and lost["n_vis_gt"] > 0
    saved = json.loads((tmp_path / "out.json").read_text())
    assert set(saved["frames"]) == set(run["names"]) and "visib_fract" in saved["frames"][run["names"][0]]
    # a cut above every frame's visible fraction leaves no frame to score
    SE.main(common + sensor + ["--min_visib_fract", "1.0"])
    cut = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert cut["n_below_visibility"] == N and np.isnan(cut["ar_vsd_sensor"])
    # --bop: render_evaluation's own --bop line is unchanged key for key, ar_bop_sensor stands beside it
    RE.main(common + ["--bop"])
    before = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    SE.main(common + sensor + ["--bop"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert same(line, before) and "ar_bop" in before
    assert line["ar_bop_sensor"] == pytest.approx((line["ar_vsd_sensor"] + line["ar_mssd"] + line["ar_mspd"]) / 3)
