"""pxt_score_pose_hypotheses_depth against its numpy restatement (relocalizer.score_hypotheses_depth_reference), all four
integers of every hypothesis, on the camera table of tests/camera_cases.py (ndist 0, 2 and 4).

The restatement runs in float32.  The kernel's float32 differs from numpy's where the compiler contracts a product and
a sum (transform_point and project_point are compiled with -ffp-contract=on), so a point that the FLOAT64 restatement
puts next to a decision boundary may be counted either way and is left out of the comparison:
  * within PX_MARGIN = 1e-3 px (tests/camera_cases.py; occlusion.FRAGILE_PX) of a pixel-rounding boundary (a half-integer
    u or v) or of an edge of project_point's image test,
  * within Z_MARGIN of z = eps or R2_REL_MARGIN of the distortion model's range limit (camera_cases.py),
  * | |r| - tolerance | < R_MARGIN = 8 ulp of a float32 in [4, 8) = 8 * 2^-21: p.z is four products and three sums of
    magnitudes below 8 (error <= 4 ulp with or without contraction), d one rounded product.
Those bands contain the one-ulp band around each boundary.  At most 1 % of a case's point evaluations may be left out
(asserted), and on all the others the float32 and the float64 restatement agree with each other on the CPU (asserted).
A hypothesis with F fragile points must give, per count, the restatement's count over its other points plus 0..F; with
F = 0 that is equality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import camera_cases as CC
from pixtrack_amd import _lib
from pixtrack_amd import relocalizer as RL
from pixtrack_amd.geometry import Camera
from pixtrack_amd.synthetic import rodrigues

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 1024.0   # SfM units per count, exact in float32
TOL = 0.0137
R_MARGIN = 8 * 2.0 ** -21
N_BANK = 700
COUNTS = (0, 1, 63, 64, 65, 300)
SIZES = {"64x48": (64, 48, 130), "5x3": (5, 3, 3), "1x1": (1, 1, 1)}
SENTINEL = -77


def table_camera(name, W, H):
    """The table's 320 x 240 camera resampled to W x H (pixel centres at integer coordinates) -> (10 floats, ndist)."""
    c = [float(x) for x in Camera.from_colmap(CC.colmap(name)).as10().tolist()]
    sx, sy = W / c[0], H / c[1]
    return [float(W), float(H), c[2] * sx, c[3] * sy, (c[4] + 0.5) * sx - 0.5, (c[5] + 0.5) * sy - 0.5, *c[6:]], CC.NDIST[name]


@functools.lru_cache(maxsize=None)
def make_case(name, size, masked=True, seed=0):
    """Bank, hypotheses and sensor plane of one case (``masked``: with a point mask), with both restatements and the
    fragile points; made once."""
    W, H, M = SIZES[size]
    cam = table_camera(name, W, H)
    rng = np.random.default_rng(1000 * seed + 17 * len(name) + W)
    p3d = (rng.normal(size=(N_BANK, 3)) * 0.25).astype(np.float32)
    mask = (rng.uniform(size=N_BANK) > 0.15).astype(np.uint8)
    valid = mask if masked else None
    fx, fy, cx, cy = cam[0][2:6]
    poses = np.zeros((M, 12), np.float32)
    for h in range(M):
        R = rodrigues(rng.normal(size=3) * rng.uniform(0, np.pi))
        z = rng.uniform(1.5, 4.0)
        # the object's centre on a pixel inside the image, or up to a quarter of the image outside it
        u, v = rng.uniform(-0.25 * W, 1.25 * W), rng.uniform(-0.25 * H, 1.25 * H)
        t = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        if M > 8 and h == 7:
            t[2] = -2.0  # the whole object behind the camera
        poses[h] = np.concatenate([R.reshape(-1), t])
    # ranges: every count of COUNTS, overlapping and out of order; one outside the bank
    ranges = np.zeros((M, 2), np.int32)
    for h in range(M):
        n = COUNTS[(h + 5) % len(COUNTS)] if M > 1 else 300
        ranges[h] = [rng.integers(0, N_BANK - n + 1), n]
    outside = 1 if M >= 3 else None
    if outside is not None:
        ranges[outside] = [N_BANK - 10, 300]
    if M >= 3:
        ranges[0][1] = 300  # the hypothesis the plane is built around
    # the plane: around hypothesis 0's points zeros, counts within the tolerance and counts on either side of it
    sensor = rng.integers(1, 5000, size=(H, W)).astype(np.uint16)
    sensor[rng.uniform(size=(H, W)) < 0.1] = 0
    first = RL.score_hypotheses_depth_reference(p3d, valid, poses[:1], ranges[:1], sensor, SCALE, TOL, cam, dtype=np.float64)
    pts = first["points"][0]
    for k in np.nonzero(pts["inside"])[0]:
        x, y = (int(np.floor(pts[c][k] + 0.5)) for c in ("u", "v"))
        kind = rng.integers(0, 5)
        tol_counts = TOL / SCALE
        offset = (0.0, rng.uniform(-0.9, 0.9) * tol_counts, rng.uniform(1.2, 40) * tol_counts, -rng.uniform(1.2, 40) * tol_counts)
        sensor[y, x] = 0 if kind == 4 else int(np.clip(np.rint(pts["pz"][k] / SCALE + offset[kind]), 1, 65535))
    r32 = RL.score_hypotheses_depth_reference(p3d, valid, poses, ranges, sensor, SCALE, TOL, cam)
    r64 = RL.score_hypotheses_depth_reference(p3d, valid, poses, ranges, sensor, SCALE, TOL, cam, dtype=np.float64)
    fragile, n_eval, n_fragile = [], 0, 0
    for h in range(M):
        q = r64["points"][h]
        if q is None:
            fragile.append(None)
            continue
        idx = q["index"]
        live = np.ones(len(idx), bool) if valid is None else valid[idx] != 0
        T = poses[h].astype(np.float64)
        x = p3d[idx].astype(np.float64)
        p_cam = x @ T[:9].reshape(3, 3).T + T[9:]
        u, v = q["u"], q["v"]
        with np.errstate(all="ignore"):
            half = lambda a: np.abs((a + 0.5) - np.rint(a + 0.5))
            near_px = (half(u) < CC.PX_MARGIN) | (half(v) < CC.PX_MARGIN)
            near_edge = (np.minimum(np.abs(u), np.abs(u - (W - 1))) < CC.PX_MARGIN) | (
                np.minimum(np.abs(v), np.abs(v - (H - 1))) < CC.PX_MARGIN)
            near_z = np.abs(p_cam[:, 2] - 1e-3) < CC.Z_MARGIN
            near_r2 = CC.r2_margin(cam[0][6:6 + cam[1]], p_cam) < CC.R2_REL_MARGIN
            near_tol = q["inside"] & (np.abs(np.abs(q["r"]) - TOL) < R_MARGIN)
        assert np.abs(p_cam[:, 2]).max(initial=0) < 8 and float(sensor.max()) * SCALE < 8  # what R_MARGIN assumes
        f = live & np.isfinite(u) & np.isfinite(v) & (near_px | near_edge | near_z | near_r2 | near_tol)
        fragile.append(f)
        n_eval += int(live.sum())
        n_fragile += int(f.sum())
        # float32 against float64 on the CPU: the same class for every point that is not left out
        p32 = r32["points"][h]
        for key in ("inside", "measured", "agree", "behind"):
            assert np.array_equal(p32[key][~f], q[key][~f]), (name, size, h, key)
    assert n_fragile <= 0.01 * max(n_eval, 1), (name, size, n_fragile, n_eval)
    # the restatement's counts over the points that are compared, and how many are not
    robust = np.full((M, 4), -1, np.int64)
    slack = np.zeros(M, np.int64)
    for h in range(M):
        p32 = r32["points"][h]
        if p32 is not None:
            keep = ~fragile[h]
            robust[h] = [int((p32[k] & keep).sum()) for k in ("inside", "measured", "agree", "behind")]
            slack[h] = int(fragile[h].sum())
    return dict(cam=cam, W=W, H=H, M=M, p3d=p3d, valid=valid, poses=poses, ranges=ranges, sensor=sensor, r32=r32,
                robust=robust, slack=slack, outside=outside, n_fragile=n_fragile, n_eval=n_eval)


def launch(case, device, poses=None, ranges=None, out=None, sensor=None):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    poses = case["poses"] if poses is None else poses
    ranges = case["ranges"] if ranges is None else ranges
    sensor = case["sensor"] if sensor is None else sensor
    return RL.score_hypotheses_depth(dev(case["p3d"]), None if case["valid"] is None else dev(case["valid"]), dev(poses), dev(ranges),
                                     dev(sensor.view(np.int16)), SCALE, TOL, case["cam"], out=out)


def check_against_restatement(case, got, robust, slack):
    got = got.cpu().numpy().astype(np.int64)
    for h in range(len(got)):
        if robust[h, 0] < 0:
            assert got[h].tolist() == [-1, -1, -1, -1], (h, got[h])
            continue
        low, high = robust[h], robust[h] + slack[h]
        assert (got[h] >= low).all() and (got[h] <= high).all(), (h, got[h], low, int(slack[h]), case["ranges"][h])


CASES = [(name, "64x48", masked) for name in CC.CAMERAS for masked in (True, False)] + [
    (name, size, masked) for name, masked in (("pinhole", False), ("k1_limit", True), ("opencv", True)) for size in ("5x3", "1x1")]


@pytest.mark.parametrize("name,size,masked", CASES, ids=[f"{n}-{s}-{'mask' if m else 'nomask'}" for n, s, m in CASES])
def test_kernel_matches_the_restatement(device, name, size, masked):
    case = make_case(name, size, masked)
    M = case["M"]
    counted = case["r32"]["out"][case["r32"]["out"][:, 0] >= 0].sum(0)
    print(f"{name} {size} mask {masked}: {case['n_fragile']} of {case['n_eval']} point evaluations left out; restatement "
          f"sums {counted.tolist()}")
    out = torch.full((M, 4), SENTINEL, dtype=torch.int32, device=device)
    got = launch(case, device, out=out)
    assert got is out
    check_against_restatement(case, got, case["robust"], case["slack"])
    exact = case["slack"] == 0
    assert np.array_equal(got.cpu().numpy()[exact], case["r32"]["out"][exact])  # (most hypotheses: plain equality)
    if size == "64x48":
        assert (counted > 0).all() and counted[1] < counted[0] and counted[2] + counted[3] < counted[1], counted
        assert set(COUNTS) <= set(case["ranges"][:, 1].tolist()) and case["outside"] is not None
        assert exact.sum() > M // 2


def test_the_hand_made_case_on_the_device(device):
    """tests/test_relocalize_depth_host.py's five points on its 4 x 3 plane (every value exact in float32: no margin), and
    a 1 x 1 plane whose one pixel a point on the optical axis hits."""
    from test_relocalize_depth_host import HAND_CAM, HAND_POINTS, IDENTITY, hand_sensor

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    poses = np.stack([IDENTITY, IDENTITY, IDENTITY]).astype(np.float32)
    ranges = np.array([[0, 5], [4, 2], [1, 2]], np.int32)
    for valid, want in ((None, [[3, 2, 1, 1], [-1] * 4, [2, 1, 0, 1]]),
                        (np.array([1, 0, 1, 1, 1], np.uint8), [[2, 1, 1, 0], [-1] * 4, [1, 0, 0, 0]])):
        got = RL.score_hypotheses_depth(dev(HAND_POINTS.astype(np.float32)), None if valid is None else dev(valid), dev(poses),
                                        dev(ranges), dev(hand_sensor().view(np.int16)), 0.5, 0.5, HAND_CAM)
        assert got.cpu().tolist() == want
        ref = RL.score_hypotheses_depth_reference(HAND_POINTS, valid, poses, ranges, hand_sensor(), 0.5, 0.5, HAND_CAM)
        assert ref["out"].tolist() == want
    one = ([1.0, 1.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 0)
    pts = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 2.5], [0.0, 0.0, 6.0], [0.1, 0.0, 3.0], [0.0, 0.0, -3.0]], np.float32)
    plane = np.array([[6]], np.uint16)  # d = 3
    got = RL.score_hypotheses_depth(dev(pts), None, dev(poses[:1]), dev(np.array([[0, 5]], np.int32)), dev(plane.view(np.int16)),
                                    0.5, 0.25, one)
    assert got.cpu().tolist() == [[3, 3, 1, 1]]  # on the surface, in front of it by two tolerances, behind it; two outside
    assert RL.score_hypotheses_depth_reference(pts, None, poses[:1], [[0, 5]], plane, 0.5, 0.25, one)["out"].tolist() == [[3, 3, 1, 1]]


def test_a_hypothesis_depends_on_its_own_inputs_only(device):
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    case = make_case("opencv", "64x48")
    M = case["M"]
    a = launch(case, device).cpu()
    assert torch.equal(a, launch(case, device).cpu())
    perm = np.random.default_rng(3).permutation(M)
    assert torch.equal(launch(case, device, poses=case["poses"][perm], ranges=case["ranges"][perm]).cpu(), a[perm])
    for lo, hi in ((5, 6), (0, 3), (2, 67), (M - 1, M)):  # M changes, and with it a hypothesis's wave and workgroup
        assert torch.equal(launch(case, device, poses=case["poses"][lo:hi], ranges=case["ranges"][lo:hi]).cpu(), a[lo:hi])
    # ... and 20 launches on a second stream beside UNet passes
    net = UNet(make_synthetic_unet_weights(7), device)
    img = torch.rand(96, 128, 3, device=device) * 255
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    args = (dev(case["p3d"]), dev(case["valid"]), dev(case["poses"]), dev(case["ranges"]), dev(case["sensor"].view(np.int16)))
    outs = [torch.full((M, 4), SENTINEL, dtype=torch.int32, device=device) for _ in range(20)]
    main, side = torch.cuda.current_stream(device), torch.cuda.Stream(device=device)
    side.wait_stream(main)
    for o in outs:
        net.forward_packed(img, None, True)
        with torch.cuda.stream(side):
            RL.score_hypotheses_depth(*args, SCALE, TOL, case["cam"], out=o)
    torch.cuda.synchronize(device)
    bad = [i for i, o in enumerate(outs) if not torch.equal(o.cpu(), a)]
    assert not bad, bad


def test_bad_arguments_are_refused_and_write_nothing(device):
    case = make_case("radial_k2", "64x48")
    M, W, H = case["M"], case["W"], case["H"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    p3d, valid, sensor = dev(case["p3d"]), dev(case["valid"]), dev(case["sensor"].view(np.int16))
    # (one float / int32 / int16 of slack in front, so that a misaligned pointer still lies inside the tensor)
    poses = torch.zeros(M * 12 + 4, device=device)
    poses[4:] = dev(case["poses"]).reshape(-1)
    ranges = torch.zeros(M * 2 + 2, dtype=torch.int32, device=device)
    ranges[2:] = dev(case["ranges"]).reshape(-1)
    out = torch.full((M * 4 + 4,), SENTINEL, dtype=torch.int32, device=device)
    L, s = _lib.lib(), _lib.stream_ptr(device)
    cam = (C.c_float * 10)(*case["cam"][0])
    wrong_cam = (C.c_float * 10)(*([W + 1.0] + case["cam"][0][1:]))
    bank = _lib.RelocBank(p3d.data_ptr(), None, valid.data_ptr(), N_BANK)
    ok = dict(bank=C.byref(bank), poses=poses.data_ptr() + 16, ranges=ranges.data_ptr() + 8, M=M, sensor=sensor.data_ptr(),
              W=W, H=H, cam=cam, ndist=case["cam"][1], out=out.data_ptr() + 16)

    def call(**kw):
        a = {**ok, **kw}
        return L.pxt_score_pose_hypotheses_depth(a["bank"], a["poses"], a["ranges"], a["M"], a["sensor"], a["W"], a["H"],
                                                 SCALE, TOL, a["cam"], a["ndist"], a["out"], s)

    bad = {"no bank": dict(bank=None), "no poses": dict(poses=None), "no ranges": dict(ranges=None), "no sensor": dict(sensor=None),
           "no camera": dict(cam=None), "no out": dict(out=None), "M = 0": dict(M=0), "M < 0": dict(M=-2),
           "M > 2^22": dict(M=(1 << 22) + 1), "width 0": dict(W=0), "height 0": dict(H=0), "height < 0": dict(H=-H),
           "more than 2^28 pixels": dict(W=1 << 15, H=(1 << 13) + 1), "ndist 1": dict(ndist=1), "ndist 3": dict(ndist=3),
           "ndist 6": dict(ndist=6), "poses 8-byte aligned": dict(poses=poses.data_ptr() + 8),
           "out 4-byte aligned": dict(out=out.data_ptr() + 4), "ranges 4-byte aligned": dict(ranges=ranges.data_ptr() + 4),
           "sensor at an odd address": dict(sensor=sensor.data_ptr() + 1),
           "a bank without points": dict(bank=C.byref(_lib.RelocBank(None, None, valid.data_ptr(), N_BANK))),
           "an empty bank": dict(bank=C.byref(_lib.RelocBank(p3d.data_ptr(), None, valid.data_ptr(), 0))),
           "another camera's size": dict(cam=wrong_cam)}
    for what, kw in bad.items():
        assert call(**kw) == -1, what  # PXT_E_ARG
    torch.cuda.synchronize(device)
    assert bool((out == SENTINEL).all())
    assert call() == 0  # ... and the very same call with nothing wrong
    torch.cuda.synchronize(device)
    assert torch.equal(out[4:].view(M, 4).cpu(), launch(case, device).cpu()) and bool((out[:4] == SENTINEL).all())
    # the wrapper's own checks: a host tensor, a wrong dtype, a non-contiguous plane, the camera of another size
    good = (p3d, valid, dev(case["poses"]), dev(case["ranges"]), sensor)
    for k, wrong in ((0, p3d.cpu()), (0, p3d.double()), (1, valid.float()), (2, good[2][:, :11]), (3, good[3].long()),
                     (4, sensor.float()), (4, sensor.t()), (4, sensor[:, :-1].contiguous())):
        with pytest.raises(_lib.PxtError):
            RL.score_hypotheses_depth(*(good[:k] + (wrong,) + good[k + 1:]), SCALE, TOL, case["cam"])
    with pytest.raises(_lib.PxtError):
        RL.score_hypotheses_depth(*good, SCALE, TOL, case["cam"], out=torch.zeros(M, 4, device=device))


def test_the_ground_truth_pose_agrees_on_the_meshs_own_depth_plane(device):
    """Points taken from a mesh's depth plane (one per covered pixel of a lattice, back-projected through the pixel's
    centre), the plane quantised to counts: at the pose it was drawn with every such point is in the image, measured and
    agrees; pushed back by ten tolerances none agrees and the sensor sees none of them behind it."""
    from pixtrack_amd import mesh_render as R
    from pixtrack_amd.synthetic import look_at_pose, make_bumpy_mesh

    W, H = 96, 72
    V, F = make_bumpy_mesh(1041, subdivisions=2)[:2]
    renderer = R.MeshRenderer(V, F, device, colors=np.full(V.shape, 0.5, np.float32))
    cam = Camera.from_colmap(dict(model="PINHOLE", width=W, height=H, params=[110.0, 108.0, W / 2.0 - 3, H / 2.0 + 2]))
    Rg, tg = look_at_pose(np.array([2.2, -1.4, 1.1]), np.zeros(3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rg, tg
    depth, _, _ = renderer.render_depth(R.view_record(cam, T)[None], W, H)
    g = depth[0].cpu().numpy().astype(np.float64)
    z = np.where(g[..., 3] > 0, g[..., 0], 0.0)
    scale = float(z.max() / 20000)
    sensor = np.rint(z / scale).astype(np.uint16)  # 0 off the object
    ys, xs = np.nonzero(z[::2, ::2] > 0)
    ys, xs = 2 * ys, 2 * xs
    assert len(ys) > 300
    c10 = [float(x) for x in cam.as10().tolist()]
    zc = z[ys, xs]
    p_cam = np.stack([(xs - c10[4]) / c10[2] * zc, (ys - c10[5]) / c10[3] * zc, zc], 1)
    p3d = ((p_cam - tg) @ Rg).astype(np.float32)  # R^T (p - t)
    tol = 4 * scale  # half a count of quantisation, and float32 round-off in the back-projection well below a count
    back = tg + np.array([0.0, 0.0, 10 * tol])
    poses = np.stack([np.concatenate([Rg.reshape(-1), tg]), np.concatenate([Rg.reshape(-1), back])]).astype(np.float32)
    ranges = np.array([[0, len(p3d)], [0, len(p3d)]], np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = RL.score_hypotheses_depth(dev(p3d), None, dev(poses), dev(ranges), dev(sensor.view(np.int16)), scale, tol, cam).cpu().numpy()
    n_in, n_measured, n_agree, n_behind = out[0].tolist()
    assert n_in == n_measured == n_agree == len(p3d) and n_behind == 0, out
    assert out[1, 2] == 0 and out[1, 3] == 0 and out[1, 1] <= out[1, 0] <= len(p3d), out
    ref = RL.score_hypotheses_depth_reference(p3d, None, poses, ranges, sensor, scale, tol, cam)
    assert np.array_equal(ref["out"][0], out[0])
