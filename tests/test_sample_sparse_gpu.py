"""The sparse sampler (csrc/pxt_lm.hip sample_sparse_kernel) against a float64 restatement, row by row - and, on maps
that are affine in the texel coordinates, as a probe of the projection arithmetic every projecting kernel shares
(csrc/pxt_common.h project_point, csrc/pxt_lm_point.h point_in_window / sample_texels).

The sampler is the one kernel whose own (u, v) can be read back: bilinear interpolation of an affine map returns the
affine function of (u, v), so with normalize = 0 and the descriptor channels x, y, 0.5 x - 0.25 y + 3, 1 (confidence
0.125 x + 0.0625 y) an output row IS the kernel's projection, and channel 3 (1 on a valid row, 0 on an invalid one) its
per-level validity.  The restatement is oracle/lm_oracle.py interp_sparse_observations in float64 (then l2_normalize),
on the float32 inputs the kernel was given, widened; one call per level, with that level's float32 camera record.

What is held, for every point of every launch (check_launch)
  * a level's row of a point the float64 oracle calls valid on that level: channels [0, C) and channel C within the
    bars; every element of [C + 1, cstride) exactly 0 (the maps hold 7.0 there);
  * a level's row of a point invalid on that level: exactly 0 over the whole cstride (the buffers start as NaN);
  * valid[n]: the AND over the levels (the buffer starts as 0xFF).
  A decision is DECIDABLE when the float64 point lies farther than 1e-3 px from the image border and the padded border
  of the level, farther than relative 1e-5 from the range limit in r^2 and farther than 1e-6 from eps in z
  (tests/camera_cases.py).  An undecidable row is not skipped: it must be exactly 0 or within the bars, and the
  undecidable points are counted, printed and held below 2 % of the launch.

Bars (measured by this file's __main__ on the CPU: the float32 oracle - the same calls in float32 - against the float64
oracle over the same launches, rows valid in both; a bar is 4 x the worst value, the factor the project uses for another
order of operations, as tests/test_lm_steps_gpu.py; the device's own output never enters)
  F32_PROBE[w]   the probe's rows (u, v and their affine images) per level width
  F32_RAW / F32_NORM / F32_CONF   random maps: the raw descriptor, the normalised one, the confidence
For orientation: a swapped p1 / p2 moves a point by 0.04 px at 320 x 240, 0.01 px at 80 x 60, 6e-4 px at 5 x 4."""
import functools
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
from pixtrack_amd.geometry import Camera
from pixtrack_amd.synthetic import make_lm_scene, perturb_pose

pytestmark = pytest.mark.gpu

# measured on the CPU by this file's __main__ (float32 oracle vs float64 oracle, worst over every valid row)
F32_PROBE = {80: 2.81e-5, 20: 7.01e-6, 5: 1.87e-6}  # px (measured 2.801e-5, 7.003e-6, 1.867e-6: all k2_limit, ground-truth pose)
F32_RAW = 4.53e-5  # raw descriptor, values of magnitude 4 (4.521e-5: k1_limit BAD pad 0 normalize 0 n 9, the 80 x 60 level)
F32_NORM = 1.91e-5  # normalised descriptor (1.904e-5: k1_limit SAD pad 1 normalize 1 n 1201, the 32-channel level)
F32_CONF = 8.83e-6  # confidence (8.825e-6: k1_limit B pad 0 normalize 1 n 1201)
UNDECIDABLE_SHARE = 0.02
PXT_E_ARG = -1  # (include/pixtrack_hip.h)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
TAIL_FILL = 7.0  # what the maps hold in [C + 1, cstride): the rows' zero tails are the kernel's, not the map's


# ------------------------------------------------------------------------------------------------ host inputs
def affine_map(h, w):
    """[h, w, 8]: descriptor x, y, 0.5 x - 0.25 y + 3, 1; confidence 0.125 x + 0.0625 y; every value exact in float32."""
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    m = torch.full((h, w, 8), TAIL_FILL)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3], m[..., 4] = x, y, 0.5 * x - 0.25 * y + 3, 1.0, 0.125 * x + 0.0625 * y
    return m


def affine_row(u, v):
    return [u, v, 0.5 * u - 0.25 * v + 3, 1.0, 0.125 * u + 0.0625 * v, 0.0, 0.0, 0.0]


@functools.lru_cache(maxsize=None)
def random_map(h, w, Cc, cs, seed=0):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + Cc + seed)
    m = torch.full((h, w, cs), TAIL_FILL)
    m[..., :Cc] = torch.randn(h, w, Cc, generator=g)
    m[..., Cc] = 0.05 + 0.9 * torch.rand(h, w, generator=g)
    return m


def level(fmap, Cc, cam10, ndist, window=None, full=None):
    """One level of a launch.  window = (x0, y0, full_w, full_h) and full = the whole level's map, of which fmap is the
    window (the restatement samples `full`)."""
    return dict(fmap=fmap, C=Cc, cam10=np.asarray(cam10, np.float32), ndist=ndist, window=window, full=full)


def table_level(name, fmap, Cc):
    """The table camera `name`, scaled from 320 x 240 to the map's size through Camera.scale."""
    h, w = fmap.shape[:2]
    cam = Camera.from_colmap(CC.colmap(name)).scale((w / CC.WIDTH, h / CC.HEIGHT))
    return level(fmap, Cc, cam.as10().numpy(), CC.NDIST[name])


@functools.lru_cache(maxsize=None)
def table_points(name, n):
    """-> (p3d float32 [n, 3], {pose name: 12 float32}): the first n points of the case's scene, a few of them moved
    behind the camera, under the ground-truth pose and a pose 15 degrees off it (points leave the image)."""
    sc = make_lm_scene(seed=1501, n_points=1201, **CC.SCENE_KW[name])
    p3d = sc.p3d[:n].copy()
    eye = -sc.R_gt.T @ sc.t_gt
    k = min(12, n // 3)
    p3d[n - k:] = eye + (eye - sc.center) * np.linspace(0.2, 2.0, k)[:, None] + 0.1 * (p3d[n - k:] - sc.center)
    rng = np.random.default_rng(77)
    R15, t15 = perturb_pose(sc.R_gt, sc.t_gt, rng, 15.0, 0.05, sc.center)
    poses = {"gt": np.concatenate([sc.R_gt.reshape(-1), sc.t_gt]).astype(np.float32),
             "rot15": np.concatenate([R15.reshape(-1), t15]).astype(np.float32)}
    return p3d.astype(np.float32), poses


# ------------------------------------------------------------------------------------------------ the restatement
def restate(levels, p3d, T12, pad, normalize, dtype=torch.float64):
    """Per level: dict(desc [n, C], conf [n], valid [n], p2d [n, 2]) from the oracle in `dtype`."""
    T = torch.from_numpy(np.asarray(T12, np.float32).copy()).to(dtype)
    R, t = T[:9].reshape(3, 3), T[9:]
    P = torch.from_numpy(np.asarray(p3d, np.float32).copy()).to(dtype)
    out = []
    for lv in levels:
        Cc = lv["C"]
        src = lv["full"] if lv["full"] is not None else lv["fmap"]
        chw = src[..., :Cc + 1].permute(2, 0, 1).contiguous().to(dtype)
        cam = torch.from_numpy(lv["cam10"][:6 + lv["ndist"]].copy()).to(dtype)
        obs, valid = O.interp_sparse_observations([chw], [(1.0, 1.0)], cam, 1.0, R, t, P, pad)
        desc = obs[0][:, :Cc]
        if normalize:
            desc = O.l2_normalize(desc, dim=1)
        p2d, _ = O.world2image(cam, O.pose_transform(R, t, P))
        out.append(dict(desc=desc, conf=obs[0][:, Cc], valid=valid, p2d=p2d))
    return out


def decidable(levels, p3d, T12, pad):
    """Per level, per point: may a float32 kernel be held to the float64 decision?  (module docstring)"""
    T = np.asarray(T12, np.float32).astype(np.float64)
    pc = np.asarray(p3d, np.float32).astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:]
    z_ok = np.abs(pc[:, 2] - O.CAM_EPS) > CC.Z_MARGIN
    out = []
    for lv, want in zip(levels, restate(levels, p3d, T12, pad, 0)):
        fw, fh = (lv["window"][2], lv["window"][3]) if lv["window"] else (lv["fmap"].shape[1], lv["fmap"].shape[0])
        assert fw == int(lv["cam10"][0]) and fh == int(lv["cam10"][1])
        uv = want["p2d"].numpy()
        ok = z_ok & (CC.r2_margin(lv["cam10"][6:6 + lv["ndist"]], pc) > CC.R2_REL_MARGIN)
        for k, size in ((0, fw), (1, fh)):
            for border in (0.0, float(pad), size - 1.0, size - 1.0 - pad):
                ok &= ~(np.abs(uv[:, k] - border) <= CC.PX_MARGIN)
        out.append(ok)
    return out


# ------------------------------------------------------------------------------------------------ the device side
def launch(device, levels, p3d, T12, pad, normalize):
    """One pxt_sample_sparse over buffers pre-filled with NaN / 0xFF -> (rows per level [n, cstride], valid [n]) on the host."""
    from pixtrack_amd.ops import ops

    n = len(p3d)
    pd = torch.from_numpy(np.ascontiguousarray(p3d, np.float32)).to(device)
    maps = [lv["fmap"].to(device).contiguous() for lv in levels]
    outs = [torch.full((n, int(m.shape[2])), float("nan"), device=device) for m in maps]
    valid = torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
    cams = [float(x) for lv in levels for x in lv["cam10"]]
    windows = None
    if any(lv["window"] for lv in levels):
        windows = [int(x) for lv in levels for x in (lv["window"] or (0, 0, 0, 0))]
    ops.sample_sparse(pd, [float(x) for x in T12], maps, [lv["C"] for lv in levels], cams, [lv["ndist"] for lv in levels],
                      pad, bool(normalize), outs, valid, windows)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], valid.cpu()


def check_launch(what, levels, p3d, T12, pad, normalize, outs, valid, desc_bars, conf_bars, hand_placed=False):
    """Everything the module docstring lists, for one launch.  -> per level, the float64 validity."""
    n = len(p3d)
    want = restate(levels, p3d, T12, pad, normalize)
    dec = decidable(levels, p3d, T12, pad)
    all_dec = np.logical_and.reduce(dec)
    n_undecidable = int((~all_dec).sum())
    print(f"{what}: {n_undecidable} of {n} points undecidable ({n_undecidable / n:.2%}); valid per level "
          f"{[int(w['valid'].sum()) for w in want]}")
    if n >= 100 and not hand_placed:  # (hand-placed points sit ON borders; their bytes are written out by their tests)
        assert n_undecidable <= UNDECIDABLE_SHARE * n, (what, n_undecidable)
    assert set(np.unique(valid.numpy())) <= {0, 1}, what
    v64 = np.logical_and.reduce([w["valid"].numpy() for w in want])
    assert np.array_equal(valid.numpy()[all_dec].astype(bool), v64[all_dec]), what
    for li, (lv, w, o, d, dbar, cbar) in enumerate(zip(levels, want, outs, dec, desc_bars, conf_bars)):
        Cc = lv["C"]
        o = o.double()
        assert bool(torch.isfinite(o).all()), (what, li, "a row was not written")
        zero_row = (o == 0).all(1).numpy()
        err_d = (o[:, :Cc] - w["desc"]).abs().amax(1).numpy()
        err_c = (o[:, Cc] - w["conf"]).abs().numpy()
        within = (err_d <= dbar) & (err_c <= cbar) & (o[:, Cc + 1:] == 0).all(1).numpy()
        wv = w["valid"].numpy()
        bad_valid = d & wv & ~within
        bad_invalid = d & ~wv & ~zero_row
        bad_undecided = ~d & ~(within | zero_row)
        assert not bad_valid.any(), (what, li, "valid rows off", np.nonzero(bad_valid)[0][:5], err_d[bad_valid][:5],
                                     err_c[bad_valid][:5], dbar, cbar)
        assert not bad_invalid.any(), (what, li, "invalid rows not zero", np.nonzero(bad_invalid)[0][:5])
        assert not bad_undecided.any(), (what, li, "undecidable rows neither zero nor sampled", np.nonzero(bad_undecided)[0][:5])
        if (d & wv).any():
            print(f"    level {li} ({lv['fmap'].shape[1]}x{lv['fmap'].shape[0]}): worst descriptor error "
                  f"{err_d[d & wv].max():.2e} (bar {dbar:.2e}), confidence {err_c[d & wv].max():.2e} (bar {cbar:.2e})")
    return [w["valid"].numpy() for w in want], dec


# ------------------------------------------------------------------------------------------------ 3. the probe
PROBE_SIZES = [(60, 80), (15, 20), (4, 5)]
PROBE_N = 1001
PROBE_CASES = [(name, pose) for name in CC.CAMERAS for pose in ("gt", "rot15")]
PROBE_PAD = {"gt": 0, "rot15": 1}


def probe_problem(name, pose):
    levels = [table_level(name, affine_map(h, w), 4) for h, w in PROBE_SIZES]
    p3d, poses = table_points(name, PROBE_N)
    return levels, p3d, poses[pose], PROBE_PAD[pose]


@pytest.mark.parametrize("name,pose", PROBE_CASES, ids=[f"{n}-{p}" for n, p in PROBE_CASES])
def test_probe_rows_are_the_float64_projection(device, name, pose):
    levels, p3d, T12, pad = probe_problem(name, pose)
    outs, valid = launch(device, levels, p3d, T12, pad, 0)
    bars = [4 * F32_PROBE[lv["fmap"].shape[1]] for lv in levels]
    valid64, _ = check_launch(f"probe {name} {pose}", levels, p3d, T12, pad, 0, outs, valid, bars, bars)
    # the launch reaches every verdict on the two finer levels
    for v in valid64[:2]:
        assert 50 <= int(v.sum()) <= PROBE_N - 12


# ---- hand-placed exact decisions: identity pose, unit camera, points (x, y, 1) with float32-exact x and y
def ulp_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def ulp_down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


HAND_W, HAND_H = 7, 5


def hand_points(pad):
    """-> [(x, y, z, expected valid byte)]: on, and one ulp either side of, pad and size - 1 - pad; half-integers.
    (The bytes follow from pad <= u <= size - 1 - pad on exact numbers; EXPECTED_BYTES writes them out.)"""
    lo, hx, hy = float(pad), HAND_W - 1.0 - pad, HAND_H - 1.0 - pad
    pts = []
    for x in (ulp_down(lo), lo, ulp_up(lo), lo + 0.5, hx - 0.5, ulp_down(hx), hx, ulp_up(hx)):
        pts.append((x, 2.0, 1.0, int(lo <= x <= hx)))  # y = 2 is inside for every pad: 2 <= HAND_H - 1 - 2
    for y in (ulp_down(lo), lo, ulp_up(lo), lo + 0.5, hy - 0.5, ulp_down(hy), hy, ulp_up(hy)):
        pts.append((3.0, y, 1.0, int(lo <= y <= hy)))  # x = 3 is inside for every pad
    pts.append((hx, hy, 1.0, 1))  # the corner: both second taps masked at pad 0
    return pts


EXPECTED_BYTES = {  # written out: hand_points(pad) must reproduce these
    0: [0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1],
    1: [0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1],
    2: [0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1],  # (5 rows: pad = HAND_H - 1 - pad = 2, one valid y)
}


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_hand_placed_points_decide_exactly(device, pad):
    pts = hand_points(pad)
    assert [p[3] for p in pts] == EXPECTED_BYTES[pad]
    xyz = np.asarray([p[:3] for p in pts], np.float32)
    lv = level(affine_map(HAND_H, HAND_W), 4, [HAND_W, HAND_H, 1, 1, 0, 0, 0, 0, 0, 0], 0)
    outs, valid = launch(device, [lv], xyz, IDENTITY, pad, 0)
    assert valid.tolist() == EXPECTED_BYTES[pad], (valid.tolist(), EXPECTED_BYTES[pad])
    for (x, y, _, ok), row in zip(pts, outs[0].double().numpy()):
        if not ok:
            assert (row == 0).all(), (x, y, row)
            continue
        want = np.asarray(affine_row(float(np.float32(x)), float(np.float32(y))))
        if (2 * x).is_integer() and (2 * y).is_integer():
            # weights 0, 0.25, 0.5, 1 on small integers: every product and sum is exact, a masked tap contributes 0
            assert np.array_equal(row, want), (x, y, row, want)
        else:
            # four products and three sums of terms no larger than max |texel| = 6: 7 roundings of 2^-24 x 6
            assert np.abs(row - want).max() <= 7 * 2.0 ** -24 * 6, (x, y, row, want)
            assert (row[5:] == 0).all()


def test_eps_in_z_decides_exactly(device):
    eps32 = np.float32(1e-3)
    above = np.nextafter(eps32, np.float32(1))
    xyz = np.asarray([(3.0 * eps32, 2.0 * eps32, eps32), (3.0 * above, 2.0 * above, above), (3.0, 2.0, 0.0),
                      (3.0, 2.0, -1.0)], np.float32)
    lv = level(affine_map(HAND_H, HAND_W), 4, [HAND_W, HAND_H, 1, 1, 0, 0, 0, 0, 0, 0], 0)
    outs, valid = launch(device, [lv], xyz, IDENTITY, 0, 0)
    assert valid.tolist() == [0, 1, 0, 0]
    rows = outs[0].double().numpy()
    assert (rows[[0, 2, 3]] == 0).all()
    # u = (3 z) (1 / z): two roundings of 2^-24 x 3, then the interpolation's seven
    assert np.abs(rows[1] - np.asarray(affine_row(3.0, 2.0))).max() <= 9 * 2.0 ** -24 * 6, rows[1]


# ------------------------------------------------------------------------------------------------ 4. values and edges
SHAPES = {"A": (15, 20, 128, 132), "B": (60, 80, 128, 136), "S": (60, 80, 32, 36), "D": (5, 7, 4, 8)}
VALUE_CASES = [  # camera, levels, pad, normalize, n
    ("opencv", "SAD", 0, 1, 1201),
    ("opencv", "BAD", 1, 0, 1201),
    ("k1_limit", "SAD", 1, 1, 1201),
    ("k1_limit", "BSA", 2, 1, 1201),  # pad 2 on 15 x 20: points valid on the fine levels only
    ("opencv", "BSA", 2, 0, 1201),
    ("k1_limit", "BAD", 0, 0, 9),
    ("opencv", "SAD", 2, 1, 2),
    ("k1_limit", "SAD", 0, 1, 1),
    ("opencv", "A", 1, 1, 2),
    ("k1_limit", "B", 0, 1, 1201),
    ("opencv", "S", 2, 0, 1),
    ("k1_limit", "D", 0, 1, 9),
    ("opencv", "D", 1, 0, 1201),
    ("k1_limit", "A", 2, 0, 1201),
]


FINE_ONLY_CASE = ("k1_limit", "BSA", 1201)  # the overfilled image: many points in the 15 x 20 level's two-texel rim


def value_problem(name, shapes, n, pose="rot15"):
    levels = [table_level(name, random_map(*SHAPES[s]), SHAPES[s][2]) for s in shapes]
    p3d, poses = table_points(name, n)
    return levels, p3d, poses[pose]


def value_bars(levels, normalize):
    return [4 * (F32_NORM if normalize else F32_RAW)] * len(levels), [4 * F32_CONF] * len(levels)


@pytest.mark.parametrize("name,shapes,pad,normalize,n", VALUE_CASES,
                         ids=[f"{c[0]}-{c[1]}-pad{c[2]}-norm{c[3]}-n{c[4]}" for c in VALUE_CASES])
def test_rows_match_the_float64_restatement(device, name, shapes, pad, normalize, n):
    levels, p3d, T12 = value_problem(name, shapes, n)
    outs, valid = launch(device, levels, p3d, T12, pad, normalize)
    dbars, cbars = value_bars(levels, normalize)
    valid64, dec = check_launch(f"{name} {shapes} pad {pad} normalize {normalize} n {n}", levels, p3d, T12, pad, normalize,
                                outs, valid, dbars, cbars)
    if (name, shapes, n) == FINE_ONLY_CASE:
        # valid on both fine levels, not on the 15 x 20 one: the byte is 0, the fine rows still hold the samples
        fine_only = valid64[0] & valid64[1] & ~valid64[2] & np.logical_and.reduce(dec)
        assert int(fine_only.sum()) >= 20, int(fine_only.sum())
        assert not valid.numpy()[fine_only].any()
        assert bool((outs[0][fine_only] != 0).any(1).all()) and bool((outs[1][fine_only] != 0).any(1).all())
        assert bool((outs[2][fine_only] == 0).all())
    if n == 1201:
        assert 0 < int(valid.sum()) < n


def test_zero_descriptor_normalises_to_zero(device):
    """The four texels of a point hold an exactly zero descriptor: with normalize = 1 the row is 0 / max(0, 1e-12) = 0,
    finite; the confidence is still interpolated."""
    h, w, Cc, cs = SHAPES["D"]
    m = random_map(h, w, Cc, cs).clone()
    m[1:3, 2:4, :Cc] = 0.0
    lv = level(m, Cc, [w, h, 1, 1, 0, 0, 0, 0, 0, 0], 0)
    xyz = np.asarray([(2.5, 1.5, 1.0), (2.25, 1.75, 1.0), (4.5, 1.5, 1.0)], np.float32)
    outs, valid = launch(device, [lv], xyz, IDENTITY, 0, 1)
    rows = outs[0].double()
    assert valid.tolist() == [1, 1, 1] and bool(torch.isfinite(rows).all())
    assert bool((rows[:2, :Cc] == 0).all()) and bool((rows[2, :Cc] != 0).any())
    assert abs(float(rows[0, Cc]) - float(m[1:3, 2:4, Cc].double().mean())) <= 7 * 2.0 ** -24
    assert bool((rows[:, Cc + 1:] == 0).all())
    dbars, cbars = value_bars([lv], 1)
    check_launch("zero descriptor", [lv], xyz, IDENTITY, 0, 1, outs, valid, dbars, cbars)


def test_window_touching_the_right_and_bottom_edges(device):
    """A 32 x 32 window at the right and bottom edges of the 80 x 60 level: its rows are those of the whole level, in
    float64 and bit for bit, the last column and row at pad 0 included."""
    h, w, Cc, cs = SHAPES["S"]
    full = random_map(h, w, Cc, cs)
    x0, y0, ww, wh = 48, 28, 32, 32
    cam10 = [w, h, 1, 1, 0, 0, 0, 0, 0, 0]
    win = level(full[y0:y0 + wh, x0:x0 + ww].contiguous(), Cc, cam10, 0, window=(x0, y0, w, h), full=full)
    whole = level(full, Cc, cam10, 0)
    rng = np.random.default_rng(9)
    xs = np.r_[rng.uniform(x0 + 0.01, w - 1, 150), np.full(20, w - 1.0), rng.uniform(x0 + 0.01, w - 1, 20), w - 1.0, w - 0.5]
    ys = np.r_[rng.uniform(y0 + 0.01, h - 1, 150), rng.uniform(y0 + 0.01, h - 1, 20), np.full(20, h - 1.0), h - 1.0, h - 2.0]
    xyz = np.stack([xs, ys, np.ones_like(xs)], 1).astype(np.float32)
    for normalize in (0, 1):
        outs_w, valid_w = launch(device, [win], xyz, IDENTITY, 0, normalize)
        outs_f, valid_f = launch(device, [whole], xyz, IDENTITY, 0, normalize)
        dbars, cbars = value_bars([win], normalize)
        check_launch(f"window normalize {normalize}", [win], xyz, IDENTITY, 0, normalize, outs_w, valid_w, dbars, cbars,
                     hand_placed=True)
        assert torch.equal(valid_w, valid_f) and valid_w.tolist() == [1] * 191 + [0]
        assert np.array_equal(outs_w[0].numpy().view(np.uint32), outs_f[0].numpy().view(np.uint32))


def test_rows_keep_their_bits_under_another_order_subset_or_count(device):
    name, shapes, pad = "opencv", "SAD", 1
    levels, p3d, T12 = value_problem(name, shapes, 1201)
    for normalize in (0, 1):
        outs, valid = launch(device, levels, p3d, T12, pad, normalize)
        perm = np.random.default_rng(3).permutation(len(p3d))
        subset = np.arange(5, 1201, 7)  # 171 points: each lands in another lane group of another wave
        for what, idx in (("permuted", perm), ("subset", subset), ("n 1200", np.arange(1200)), ("n 1", np.arange(700, 701))):
            o2, v2 = launch(device, levels, p3d[idx], T12, pad, normalize)
            assert torch.equal(v2, valid[idx]), what
            for a, b in zip(o2, outs):
                assert np.array_equal(a.numpy().view(np.uint32), b[idx].numpy().view(np.uint32)), what


def test_unknown_ndist_is_refused_before_anything_is_launched(device):
    """check_level's rule (csrc/pxt_common.h): ndist is 0, 2 or 4.  The refusal comes back as PXT_E_ARG and no buffer of
    any level is touched - also where only the LAST level is wrong."""
    levels, p3d, T12 = value_problem("opencv", "SAD", 9)
    n = len(p3d)
    pd = torch.from_numpy(p3d).to(device)
    maps = [lv["fmap"].to(device).contiguous() for lv in levels]
    import ctypes

    T = (ctypes.c_float * 12)(*[float(x) for x in T12])
    for bad_level, bad in ((0, 1), (2, 3), (2, -1), (1, 6), (2, 5)):
        outs = [torch.full((n, int(m.shape[2])), float("nan"), device=device) for m in maps]
        valid = torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
        arr = (_lib.SampleLevel * 3)()
        for i, (lv, m, o) in enumerate(zip(levels, maps, outs)):
            arr[i].fmap, arr[i].out = m.data_ptr(), o.data_ptr()
            arr[i].h, arr[i].w, arr[i].C, arr[i].cstride = m.shape[0], m.shape[1], lv["C"], m.shape[2]
            arr[i].cam[:] = [float(x) for x in lv["cam10"]]
            arr[i].ndist = bad if i == bad_level else lv["ndist"]
        rc = _lib.lib().pxt_sample_sparse(pd.data_ptr(), n, T, arr, 3, 1, 1, valid.data_ptr(), _lib.stream_ptr(device))
        torch.cuda.synchronize()
        assert rc == PXT_E_ARG, (bad_level, bad, rc)
        assert bool((valid == 0xFF).all()) and all(bool(torch.isnan(o).all()) for o in outs), (bad_level, bad)
    # and the same record with the level's own ndist goes through
    outs, valid = launch(device, levels, p3d, T12, 1, 1)
    assert all(bool(torch.isfinite(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ CPU calibration
def f32_against_f64(levels, p3d, T12, pad, normalize):
    """-> per level (worst descriptor error, worst confidence error, rows compared) of the float32 oracle against the
    float64 oracle, over the rows valid in both and decidable."""
    a = restate(levels, p3d, T12, pad, normalize, torch.float32)
    b = restate(levels, p3d, T12, pad, normalize, torch.float64)
    dec = decidable(levels, p3d, T12, pad)
    out = []
    for x, y, d in zip(a, b, dec):
        both = x["valid"].numpy() & y["valid"].numpy() & d
        assert np.array_equal(x["valid"].numpy()[d], y["valid"].numpy()[d]), "the float32 oracle decides a decidable point otherwise"
        if not both.any():
            out.append((0.0, 0.0, 0))
            continue
        out.append((float((x["desc"].double() - y["desc"])[both].abs().max()), float((x["conf"].double() - y["conf"])[both].abs().max()),
                    int(both.sum())))
    return out


if __name__ == "__main__":
    # No GPU.  The float32 oracle against the float64 oracle over every probe and value launch; the share of
    # undecidable points per launch; the conditions the cases must meet.
    worst_probe = {w: (0.0, None) for w in F32_PROBE}
    for name, pose in PROBE_CASES:
        levels, p3d, T12, pad = probe_problem(name, pose)
        dec = np.logical_and.reduce(decidable(levels, p3d, T12, pad))
        share = float((~dec).mean())
        assert share <= UNDECIDABLE_SHARE, (name, pose, share)
        res = f32_against_f64(levels, p3d, T12, pad, 0)
        print(f"probe {name:10s} {pose:6s} pad {pad}: undecidable {int((~dec).sum())} of {len(p3d)} ({share:.2%}); per level "
              + "  ".join(f"{lv['fmap'].shape[1]}x{lv['fmap'].shape[0]}: {max(e[0], e[1]):.2e} over {e[2]}" for lv, e in zip(levels, res)))
        for lv, e in zip(levels, res):
            w = lv["fmap"].shape[1]
            if max(e[0], e[1]) > worst_probe[w][0]:
                worst_probe[w] = (max(e[0], e[1]), f"{name} {pose}")
    worst = {"raw": (0.0, None), "norm": (0.0, None), "conf": (0.0, None)}
    for name, shapes, pad, normalize, n in VALUE_CASES:
        levels, p3d, T12 = value_problem(name, shapes, n)
        dec = np.logical_and.reduce(decidable(levels, p3d, T12, pad))
        if n >= 100:
            assert float((~dec).mean()) <= UNDECIDABLE_SHARE, (name, shapes, pad, n)
        res = f32_against_f64(levels, p3d, T12, pad, normalize)
        what = f"{name} {shapes} pad {pad} normalize {normalize} n {n}"
        if (name, shapes, n) == FINE_ONLY_CASE:
            v = [w["valid"].numpy() for w in restate(levels, p3d, T12, pad, normalize)]
            fine_only = int((v[0] & v[1] & ~v[2] & dec).sum())
            print(f"{what:44s} {fine_only} decidable points valid on the two fine levels only")
            assert fine_only >= 20
        print(f"{what:44s} undecidable {int((~dec).sum())}; per level " + "  ".join(f"{e[0]:.2e} / {e[1]:.2e} over {e[2]}" for e in res))
        for e in res:
            key = "norm" if normalize else "raw"
            if e[0] > worst[key][0]:
                worst[key] = (e[0], what)
            if e[1] > worst["conf"][0]:
                worst["conf"] = (e[1], what)
    print("worst float32-vs-float64, probe rows per level width:", worst_probe)
    print("worst float32-vs-float64, random maps:", worst)
    print("constants in this file: F32_PROBE", F32_PROBE, "F32_RAW", F32_RAW, "F32_NORM", F32_NORM, "F32_CONF", F32_CONF)
    for w, (val, _) in worst_probe.items():
        assert val <= F32_PROBE[w] <= 1.1 * val + 1e-12, (w, val, F32_PROBE[w], "the constants are stale: measure again")
    for key, c in (("raw", F32_RAW), ("norm", F32_NORM), ("conf", F32_CONF)):
        assert worst[key][0] <= c <= 1.1 * worst[key][0] + 1e-12, (key, worst[key], c, "the constants are stale: measure again")
