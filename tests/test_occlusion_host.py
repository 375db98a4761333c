"""pixtrack_amd/occlusion.py on the host: the numpy restatements of pxt_occlusion_mask / pxt_points_visible held to an
independent statement written here (float64 per-pixel rule on inputs where float32 and float64 agree; the box morphology
as r iterations of a 3 x 3 min / max that ignores the border), the rule's edge cases, conf resolution and the refusals."""
import numpy as np
import pytest

from pixtrack_amd import occlusion as OC
from pixtrack_amd.sensor_evaluation import shifted_sensor

MIN_ALPHA, SENSOR_Q, DELTA_Q = 0.5, 0.25, 0.25


def _inputs(W, H, seed):
    """Quarter-integer depths over alpha in {0, 0.5, 1} (quotients exact in float32 and float64), raw counts 0 ... 24, a
    solid occluder rectangle, a random mask."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W, 4), np.float32)
    img[..., 3] = rng.choice(np.array([0, 0.5, 1], np.float32), size=(H, W))
    img[..., 0] = rng.integers(-4, 25, size=(H, W)).astype(np.float32) * np.float32(0.25)
    sensor = rng.integers(0, 25, size=(H, W)).astype(np.uint16)
    sensor[rng.random((H, W)) < 1 / 7] = 0
    y0, x0 = H // 4, W // 5
    img[y0:y0 + H // 2, x0:x0 + W // 2, 3] = 1.0
    img[y0:y0 + H // 2, x0:x0 + W // 2, 0] = 5.0
    sensor[y0:y0 + H // 2, x0:x0 + W // 2] = 2
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    return img, sensor, mask


def _rule64(img, sensor, shift):
    """O in float64, pixel by pixel."""
    H, W = sensor.shape
    O = np.zeros((H, W), bool)
    sil = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            d, a = float(img[y, x, 0]), float(img[y, x, 3])
            xs, ys = x + shift[0], y + shift[1]
            raw = int(sensor[ys, xs]) if (0 <= xs < W and 0 <= ys < H) else 0
            sil[y, x] = a >= MIN_ALPHA and d > 0
            if sil[y, x] and raw != 0:
                O[y, x] = d / a - raw * SENSOR_Q > DELTA_Q
    return sil, O


def _iterate3x3(plane, r, erode):
    """r iterations of a 3 x 3 min (erode) / max over the neighbours that lie inside the image."""
    H, W = plane.shape
    cur = plane.copy()
    for _ in range(r):
        nxt = cur.copy()
        for y in range(H):
            for x in range(W):
                win = cur[max(y - 1, 0):min(y + 2, H), max(x - 1, 0):min(x + 2, W)]
                nxt[y, x] = win.all() if erode else win.any()
        cur = nxt
    return cur


@pytest.mark.parametrize("shape", ((1, 1), (7, 5), (23, 17), (40, 9)))
@pytest.mark.parametrize("radii", ((0, 0), (1, 3), (2, 0), (0, 4), (3, 2)))
@pytest.mark.parametrize("shift", ((0, 0), (1, 0), (-3, 2)))
def test_restatement_matches_an_independent_statement(shape, radii, shift):
    W, H = shape
    img, sensor, mask = _inputs(W, H, 7 * W + H)
    ref = OC.occlusion_mask_reference(img, sensor, mask, shift, MIN_ALPHA, SENSOR_Q, DELTA_Q, *radii)
    sil, O = _rule64(img, sensor, shift)
    E = _iterate3x3(O, radii[0], True)
    G = _iterate3x3(E, radii[1], False)
    assert np.array_equal(ref["sil"], sil) and np.array_equal(ref["occluded"], O)
    assert np.array_equal(ref["opened"], E) and np.array_equal(ref["occluder"], G.astype(np.uint8))
    mo = (mask != 0) & ~G
    assert np.array_equal(ref["mask"], mo.astype(np.uint8))
    raw = shifted_sensor(sensor, shift)
    want = [sil.sum(), (sil & (raw != 0)).sum(), O.sum(), E.sum(), G.sum(), (mask != 0).sum(), mo.sum(), (sil & G).sum()]
    assert ref["record"][:8].tolist() == [int(x) for x in want] and not ref["record"][8:].any()
    assert ref["mask"].dtype == np.uint8 and ref["occluder"].dtype == np.uint8 and ref["record"].dtype == np.int32


def test_rule_edge_cases():
    img, sensor, mask = _inputs(23, 17, 3)
    zero = OC.occlusion_mask_reference(img, sensor, mask, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 0, 0)
    assert np.array_equal(zero["occluder"] != 0, zero["occluded"])  # r = (0, 0): G == O
    assert zero["occluded"].any()
    # an empty O: the mask passes through
    none = OC.occlusion_mask_reference(img, np.zeros_like(sensor), mask, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 1, 3)
    assert not none["occluded"].any() and np.array_equal(none["mask"], mask) and none["record"][4] == 0
    # raw == 0 is never occluded, whatever the depth
    assert not zero["occluded"][sensor == 0].any()
    # a one-pixel speck vanishes at r_open = 1 and survives at 0
    one = np.zeros((9, 9, 4), np.float32)
    one[..., 3], one[..., 0] = 1.0, 5.0
    s = np.full((9, 9), 20, np.uint16)  # 5.0: q - d_s = 0
    s[4, 4] = 2
    m = np.ones((9, 9), np.uint8)
    assert OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 0, 1)["record"][2:5].tolist() == [1, 1, 9]
    speck = OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 1, 3)
    assert speck["record"][2:5].tolist() == [1, 0, 0] and np.array_equal(speck["mask"], m)
    # q - d_s == delta_q exactly is not occluded; one count closer is
    s[...] = 19  # 4.75: q - d_s = 0.25 == delta_q
    assert OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 0, 0)["record"][2] == 0
    s[...] = 18
    assert OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 0, 0)["record"][2] == 81
    # non-finite pixels: a NaN alpha is off the silhouette, a -inf depth too, inf / inf is a NaN quotient, which is
    # above nothing: O = 0 at all three.  (A +inf depth over a finite alpha is a quotient of +inf, which the stated
    # comparison q - d_s > delta_q does hold for: such a pixel is "infinitely far behind" the sensor's surface.)
    one[2, 2, 3] = np.nan
    one[3, 3, 0] = -np.inf
    one[5, 5, 0], one[5, 5, 3] = np.inf, np.inf
    one[6, 6, 0] = np.inf
    r = OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 0, 0)
    assert not r["occluded"][2, 2] and not r["occluded"][3, 3] and not r["occluded"][5, 5]
    assert r["occluded"][6, 6] and r["record"][2] == 78
    # a border erosion ignores what lies outside: a full plane stays full
    s[...] = 2
    one[...] = 0
    one[..., 3], one[..., 0] = 1.0, 5.0
    full = OC.occlusion_mask_reference(one, s, m, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 4, 0)
    assert full["record"][2:5].tolist() == [81, 81, 81] and not full["mask"].any()


@pytest.mark.parametrize("shift", ((0, 0), (1, 0), (-3, 2), (0, -1), (23, 0), (0, 17), (-40, -40)))
def test_shift_is_shifted_sensor(shift):
    img, sensor, mask = _inputs(23, 17, 5)
    a = OC.occlusion_mask_reference(img, sensor, mask, shift, MIN_ALPHA, SENSOR_Q, DELTA_Q, 1, 2)
    b = OC.occlusion_mask_reference(img, shifted_sensor(sensor, shift), mask, (0, 0), MIN_ALPHA, SENSOR_Q, DELTA_Q, 1, 2)
    for k in ("mask", "occluder", "record"):
        assert np.array_equal(a[k], b[k])
    if abs(shift[0]) >= 23 or abs(shift[1]) >= 17:
        assert a["record"][1] == 0 and np.array_equal(a["mask"], mask)


def test_point_rule():
    W, H = 16, 12
    cam = ([float(W), float(H), 20.0, 20.0, 7.5, 5.5, 0.0, 0.0, 0.0, 0.0], 0)
    T = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    occ = np.zeros((H, W), np.uint8)
    occ[5, 7] = 1   # under the principal point (7.5 rounds half up to texel 8; 7.4 to texel 7)
    occ[0, 0] = 1
    pts = np.array([[-0.1 / 20, -0.5 / 20 + 1e-3, 1.0],    # u = 7.4, v = 5.02 -> texel (7, 5): gated
                    [0.0, 0.0, -1.0],                       # behind the camera: keeps its bit
                    [-8.0 / 20, 0.0, 1.0],                  # u = -0.5: outside the image test: keeps its bit
                    [1.0, 0.0, 1.0],                        # u = 27.5: outside: keeps its bit
                    [0.3 / 20, 0.4 / 20, 1.0],              # texel (8, 6): free
                    [-0.1 / 20, -0.5 / 20 + 1e-3, 1.0]], np.float32)
    r = OC.points_visible_reference(pts, None, T, cam, occ)
    assert r["valid"].tolist() == [0, 1, 1, 1, 1, 0] and r["counts"] == (6, 6, 4)
    assert r["texel"][0].tolist() == [7, 5] and r["texel"][4].tolist() == [8, 6]
    assert r["projects"].tolist() == [True, False, False, False, True, True]
    vin = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    r = OC.points_visible_reference(pts, vin, T, cam, occ)
    assert r["valid"].tolist() == [0, 0, 1, 0, 1, 0] and r["counts"] == (6, 3, 2) and r["gated"].tolist() == [True] + [False] * 5
    # a point at a half-integer coordinate (u = 7.5: between texels 7 and 8) is fragile; one at a texel's centre is not
    edge = np.array([[0.0, 0.0, 1.0], [0.5 / 20, 0.5 / 20, 1.0]], np.float32)
    assert OC.points_visible_reference(edge, None, T, cam, occ)["fragile"].tolist() == [True, False]
    assert OC.points_visible_reference(pts[:0], None, T, cam, occ)["counts"] == (0, 0, 0)
    with pytest.raises(ValueError):
        OC.points_visible_reference(pts, None, T, cam, np.zeros((H, W + 1), np.uint8))


def test_conf_and_refusals():
    c = OC.OcclusionConf()
    assert (c.delta, c.relative, c.r_open, c.r_grow, c.min_alpha, c.allow_misaligned) == (0.1, True, 1, 3, 0.5, False)
    a = c.resolve(2.5)
    assert a.delta == 0.25 and not a.relative and a.resolve(100.0) is a
    assert OC.OcclusionConf(delta=0.3, relative=False).resolve(7.0).delta == 0.3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            c.resolve(bad)
    for kw in (dict(r_open=-1), dict(r_grow=-1), dict(r_open=9, r_grow=8), dict(r_open=1.5), dict(delta=-0.1),
               dict(delta=float("nan"))):
        with pytest.raises(ValueError):
            OC.OcclusionConf(**kw)
    assert OC.OcclusionConf(r_open=8, r_grow=8).r_grow == 8
    sq, dq = OC.quantize(0.25, 0.001, 0.37)
    assert sq == float(np.float32(0.001 / 0.37)) and dq == float(np.float32(0.25 / 0.37))
    for bad in ((0.1, 0.001, 0.0), (0.1, 0.0, 1.0), (0.1, 0.001, float("nan"))):
        with pytest.raises(ValueError):
            OC.quantize(*bad)
    img, sensor, mask = _inputs(8, 6, 1)
    with pytest.raises(ValueError):
        OC.occlusion_mask_reference(img, sensor, mask, (0, 0), 0.5, 0.25, 0.25, 9, 8)
    with pytest.raises(ValueError):
        OC.occlusion_mask_reference(img, sensor.astype(np.int32), mask, (0, 0), 0.5, 0.25, 0.25, 1, 1)
    with pytest.raises(ValueError):
        OC.occlusion_mask_reference(img, sensor, mask[:, :-1], (0, 0), 0.5, 0.25, 0.25, 1, 1)
    assert OC.HISTORY_KEYS == ("occluded_fraction", "n_occluder_pixels", "n_points_gated", "occlusion_applied")
    assert OC.decode_record(np.arange(16))["n_points_out"] == 10


def test_alignment_follows_the_camera():
    import torch

    from pixtrack_amd.geometry import Camera

    def cam(W, H, fx, fy, cx, cy):  # COLMAP's principal point is Camera.c + 0.5
        return Camera(torch.tensor([W, H, fx, fy, cx - 0.5, cy - 0.5], dtype=torch.float64))

    assert OC.alignment(cam(160, 120, 190.0, 190.0, 80.0, 60.0)) == (0, 0, 0.0)
    sx, sy, res = OC.alignment(cam(160, 120, 190.0, 190.0, 83.2, 58.0))
    assert (sx, sy) == (3, -2) and abs(res - 0.2) < 1e-9
    skew = cam(640, 480, 500.0, 520.0, 320.0, 240.0)  # |fy / fx - 1| * H / 2 = 9.6 px
    with pytest.raises(ValueError):
        OC.alignment(skew)
    assert OC.alignment(skew, allow_misaligned=True)[2] > 1.0
