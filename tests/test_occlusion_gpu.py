"""pxt_occlusion_mask / pxt_points_visible (csrc/pxt_occlusion.hip; torch.ops.pixtrack.occlusion_mask / points_visible).

Oracle: occlusion.occlusion_mask_reference, a numpy float32 restatement of the per-pixel rules and the box morphology
(itself held to an independent statement in tests/test_occlusion_host.py).  Division, multiplication, subtraction and
comparison are single IEEE operations on both sides and the counts are integers: both planes and all eight counts are
compared BIT FOR BIT, no tolerance, no pixel left out.

The point gate projects with the LM's project_point, which the compiler contracts into FMAs and numpy does not: a point
whose projection lies within 1e-3 px of a texel boundary (a half-integer coordinate) is *fragile* and left out of the
comparison; at most 2 % of a case may be.  The seeded inputs keep the reference itself under that cap (about 0.4 %, the
share of a 2e-3 px band in a texel for uniform projections - asserted below, on the host) and place no point within
1e-3 px of the edge of project_point's image test.  The gate also runs under two cameras of tests/camera_cases.py:
OPENCV (ndist 4) and a range limit inside the image, where points beyond the range land on occluder texels and must
be kept."""
import ctypes

import numpy as np
import pytest
import torch

import camera_cases as CC
from pixtrack_amd import _lib, ops
from pixtrack_amd import occlusion as OC

pytestmark = pytest.mark.gpu

# one pixel, odd sizes, one tile row exactly, below / above one tile, three tiles with a one-pixel tail, many tiles,
# rows 16 tiles wide with a one-column tail
SHAPES = ((1, 1), (7, 5), (64, 1), (63, 3), (65, 17), (129, 33), (257, 3), (160, 120), (1023, 1), (1025, 2))
RADII = ((0, 0), (1, 3), (0, 8), (2, 0), (8, 8))
MIN_ALPHA = 0.5
SENSOR_Q = 0.25   # a raw count is a quarter: quarter-integer sensor depths
DELTA_Q = 0.25    # like most q - d_s: many equal it exactly
GUARD = 4099      # odd: the sensor array behind it is 2-byte aligned and no more
GUARD_VALUE = 0x5A5A
CANARY = 0xA5
TAIL = 64
SENTINEL = -777


def _shifts(W):
    return ((0, 0), (1, 0), (-3, 2), (W, 0))  # the last one puts every sensor pixel outside the image


def _radii(W, H):
    """The issue's radii, capped to the image where it is smaller - and as they are (the kernel's halo then reaches past
    the image on every side)."""
    cap = max(W, H) - 1
    return tuple(dict.fromkeys([(min(a, cap), min(b, cap)) for a, b in RADII] + list(RADII)))


def _inputs(W, H, seed):
    """A disc whose alpha is drawn from {0, 0.25, 0.5, 0.75, 1} and whose channel 0 from the quarter-integers of
    [-1, 6]; raw counts 0 ... 24, a seventh of them 0 - q - d_s equals delta_q at many pixels.  Two rectangles hold a
    solid occluder (alpha 1, depth 3 ... 6, counts 1 ... 2; in the second a fiftieth of them 0) so that the opening
    leaves something, removes something, and the growth has something to grow.  One inf depth and one NaN alpha; a random mask."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.45 * max(W, H) + 0.5
    disc = (xx - (W - 1) / 2) ** 2 + (yy - (H - 1) / 2) ** 2 <= r * r
    img = rng.normal(size=(H, W, 4)).astype(np.float32)
    img[..., 3] = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], np.float32), size=(H, W)) * disc
    img[..., 0] = rng.integers(-4, 25, size=(H, W)).astype(np.float32) * np.float32(0.25) * disc
    sensor = rng.integers(0, 25, size=(H, W)).astype(np.uint16)
    sensor[rng.random((H, W)) < 1 / 7] = 0
    for k in range(2):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        x1, y1 = min(W, x0 + max(1, W // 3) + 1), min(H, y0 + max(1, H // 2) + 1)
        n = (y1 - y0, x1 - x0)
        img[y0:y1, x0:x1, 3] = 1.0
        img[y0:y1, x0:x1, 0] = rng.integers(12, 25, size=n).astype(np.float32) * np.float32(0.25)
        blk = rng.integers(1, 3, size=n).astype(np.uint16)
        if k == 1:
            blk[rng.random(n) < 1 / 50] = 0
        sensor[y0:y1, x0:x1] = blk
    iy, ix = (H - 1) // 2, (W - 1) // 2
    img[iy, ix, 0], img[iy, ix, 3] = np.inf, 1.0
    if W * H > 1:
        jy, jx = divmod((iy * W + ix + 1) % (W * H), W)
        img[jy, jx, 3] = np.nan
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    return img, sensor, mask


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
    """Per shape: the inputs on the host and on the device (the sensor between its guards) and the oracle's planes and
    record for every (radii, shift)."""
    out = {}
    for n, (W, H) in enumerate(SHAPES):
        img, sensor, mask = _inputs(W, H, 900 + n)
        whole, d_sensor = _guarded(sensor, device)
        r = dict(img=img, sensor=sensor, mask=mask, d_img=torch.from_numpy(img).to(device), d_sensor=d_sensor,
                 whole=whole, d_mask=torch.from_numpy(mask).to(device), ref={})
        for radii in _radii(W, H):
            for shift in _shifts(W):
                r["ref"][(radii, shift)] = OC.occlusion_mask_reference(img, sensor, mask, shift, MIN_ALPHA, SENSOR_Q,
                                                                      DELTA_Q, *radii)
        assert r["ref"][((0, 0), (W, 0))]["record"][1] == 0  # (nothing measured when every sensor pixel is outside)
        out[(W, H)] = r
    big = out[(160, 120)]["ref"]
    assert big[((1, 3), (0, 0))]["record"][3] > 0 and big[((8, 8), (0, 0))]["record"][3] > 0  # the opening leaves something
    assert big[((1, 3), (0, 0))]["record"][2] > big[((1, 3), (0, 0))]["record"][3]            # ... and removes something
    assert 0 < big[((1, 3), (0, 0))]["record"][6] < big[((1, 3), (0, 0))]["record"][5]
    return out


class _Out:
    """mask, occluder and record with canaries behind them; one workspace."""

    def __init__(self, W, H, device, pinned_record=False):
        n = H * W
        self.n = n
        self.flat = [torch.full((n + TAIL,), CANARY, dtype=torch.uint8, device=device) for _ in range(2)]
        self.mask, self.occluder = (f[:n].view(H, W) for f in self.flat)
        rec = torch.full((OC.RECORD + 8,), SENTINEL, dtype=torch.int32)
        self.rec_all = rec.pin_memory() if pinned_record else rec.to(device)
        self.record = self.rec_all[:OC.RECORD]
        need = int(_lib.lib().pxt_occlusion_mask_workspace_bytes(W, H))
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device=device)

    def run(self, r, radii, shift):
        ops.ops.occlusion_mask(r["d_img"], r["d_sensor"], r["d_mask"], list(shift), MIN_ALPHA, SENSOR_Q, DELTA_Q,
                               list(radii), self.mask, self.occluder, self.record, self.ws)

    def get(self):
        torch.cuda.synchronize()
        for f in self.flat:
            assert (f[self.n:] == CANARY).all()
        assert (self.rec_all[OC.RECORD:] == SENTINEL).all()
        return self.mask.cpu().numpy().copy(), self.occluder.cpu().numpy().copy(), self.record.cpu().numpy().copy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_matches_the_restatement_bit_for_bit(refs, device, shape):
    W, H = shape
    r = refs[shape]
    out = _Out(W, H, device)
    for (radii, shift), ref in r["ref"].items():
        out.run(r, radii, shift)
        mask, occ, rec = out.get()
        what = f"{W}x{H} radii {radii} shift {shift}"
        assert np.array_equal(occ, ref["occluder"]), what
        assert np.array_equal(mask, ref["mask"]), what
        assert np.array_equal(rec, ref["record"]), (what, rec.tolist(), ref["record"].tolist())
    assert _guards_untouched(r["whole"])


def test_a_call_does_not_depend_on_its_neighbours(refs, device):
    """The same call twice, and beside a different call that shares its workspace, on one stream: bit-equal."""
    r = refs[(160, 120)]
    a, b = _Out(160, 120, device, pinned_record=True), _Out(160, 120, device)
    b.ws = a.ws
    a.run(r, (1, 3), (0, 0))
    first = a.get()
    b.run(r, (8, 8), (-3, 2))
    a.run(r, (1, 3), (0, 0))
    b.run(r, (0, 8), (1, 0))
    second = a.get()
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    ref = r["ref"][((1, 3), (0, 0))]
    assert np.array_equal(second[2], ref["record"]) and np.array_equal(second[0], ref["mask"])
    mask, occ, rec = b.get()
    assert np.array_equal(rec, r["ref"][((0, 8), (1, 0))]["record"])


def test_bad_arguments_launch_nothing(refs, device):
    W, H = 160, 120
    r = refs[(W, H)]
    out = _Out(W, H, device)
    L = _lib.lib()
    stream = _lib.stream_ptr(device)
    good = dict(depth=r["d_img"].data_ptr(), sensor=r["d_sensor"].data_ptr(), mask_in=r["d_mask"].data_ptr(), W=W, H=H,
                ro=1, rg=3, mask=out.mask.data_ptr(), occ=out.occluder.data_ptr(), rec=out.record.data_ptr(),
                ws=out.ws.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.pxt_occlusion_mask(a["depth"], a["sensor"], a["mask_in"], a["W"], a["H"], 0, 0, MIN_ALPHA, SENSOR_Q,
                                    DELTA_Q, a["ro"], a["rg"], a["mask"], a["occ"], a["rec"], a["ws"], stream)

    bad = [dict(ro=9, rg=8), dict(ro=17, rg=0), dict(ro=-1), dict(rg=-1), dict(depth=None), dict(sensor=None),
           dict(mask_in=None), dict(mask=None), dict(occ=None), dict(rec=None), dict(ws=None), dict(W=0), dict(H=0),
           dict(W=-4), dict(H=-1), dict(occ=good["mask"]), dict(depth=good["depth"] + 4)]
    for kw in bad:
        assert call(**kw) == -1, kw  # PXT_E_ARG
    assert int(L.pxt_occlusion_mask_workspace_bytes(0, 5)) < 0 and int(L.pxt_occlusion_mask_workspace_bytes(5, -1)) < 0
    torch.cuda.synchronize()
    assert (out.flat[0] == CANARY).all() and (out.flat[1] == CANARY).all() and (out.rec_all == SENTINEL).all()
    with pytest.raises(_lib.PxtError):
        ops.ops.occlusion_mask(r["d_img"], r["d_sensor"], r["d_mask"], [0, 0], MIN_ALPHA, SENSOR_Q, DELTA_Q, [9, 8],
                               out.mask, out.occluder, out.record, out.ws)
    assert call() == 0
    mask, occ, rec = out.get()
    assert np.array_equal(rec, r["ref"][((1, 3), (0, 0))]["record"])


# ------------------------------------------------------------------------------------------------- the point gate
PW, PH = 160, 120
COUNTS = (0, 1, 63, 64, 65, 1025, 4097)
CAM10 = [float(PW), float(PH), 190.0, 185.0, 79.5, 59.5, -0.12, 0.0, 0.0, 0.0]
NDIST = 2


def point_inputs(n, seed, cam10=None):
    """n points seen from a seeded pose: a tenth behind the camera, the rest in a frustum one and a half times as wide
    as the image; a mask that keeps four in five; an occluder plane of two rectangles and a little salt."""
    from scipy.spatial.transform import Rotation

    cam10 = CAM10 if cam10 is None else cam10
    rng = np.random.default_rng(seed)
    Rm = Rotation.from_rotvec(rng.normal(size=3) * 0.4).as_matrix()
    t = rng.normal(size=3) * 0.3 + np.array([0.0, 0.0, 2.0])
    z = rng.uniform(1.0, 3.0, size=n)
    z[rng.random(n) < 0.1] *= -1.0
    xn = rng.uniform(-1.5, 1.5, size=n) * (PW / 2) / cam10[2]
    yn = rng.uniform(-1.5, 1.5, size=n) * (PH / 2) / cam10[3]
    pc = np.stack([xn * z, yn * z, z], 1)
    X = ((pc - t) @ Rm).astype(np.float32)  # R^T (p - t)
    T12 = np.concatenate([Rm.reshape(-1), t]).astype(np.float32)
    valid = (rng.random(n) < 0.8).astype(np.uint8)
    occ = (rng.random((PH, PW)) < 0.02).astype(np.uint8)
    occ[20:70, 30:90] = 1
    occ[80:118, 100:158] = 1
    return X, T12, valid, occ


@pytest.mark.parametrize("with_mask", (False, True), ids=("all", "masked"))
@pytest.mark.parametrize("n", COUNTS)
def test_points_match_the_restatement(device, n, with_mask):
    X, T12, valid, occ = point_inputs(n, 4000 + n)
    vin = valid if with_mask else None
    ref = OC.points_visible_reference(X, vin, T12, (CAM10, NDIST), occ)
    fragile = ref["fragile"]
    # the inputs' own properties, decided on the host: the reference under the cap, nothing at the image test's edge
    assert fragile.sum() <= 0.02 * max(n, 1) and not ref["near_edge"].any()
    if n >= 1025:  # a case that says something: gated, kept, behind the camera and outside the image all occur
        assert ref["gated"].sum() > n // 20 and (~ref["projects"]).sum() > n // 10 and (ref["valid"] != 0).sum() > n // 10
    d_occ = torch.from_numpy(occ).to(device)
    rec = torch.full((OC.RECORD,), SENTINEL, dtype=torch.int32, device=device)
    out_all = torch.full((n + TAIL,), CANARY, dtype=torch.uint8, device=device)
    out = out_all[:n]
    d_X = torch.from_numpy(X).to(device).reshape(n, 3)
    d_vin = None if vin is None else torch.from_numpy(vin).to(device)
    got, _ = OC.points_visible(d_X, d_vin, T12, (CAM10, NDIST), d_occ, record=rec, valid=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    words = rec.cpu().numpy()
    assert (out_all[n:] == CANARY).all()
    assert set(np.unique(got)) <= {0, 1}
    keep = ~fragile
    assert np.array_equal(got[keep], ref["valid"][keep]), np.nonzero(got[keep] != ref["valid"][keep])
    n_in = n if vin is None else int(vin.sum())
    assert words[8:11].tolist() == [n, n_in, int(got.sum())]  # exact given the output bits
    assert (words[:8] == SENTINEL).all() and (words[11:] == SENTINEL).all()  # the mask call's words stay
    if not fragile.any():
        assert words[8:11].tolist() == list(ref["counts"])


# two cameras of tests/camera_cases.py at this plane's size (focal lengths and principal points halved): OPENCV, and
# the k1 > 0 range limit, whose radius (78 px from the principal point, distorted) lies inside the image - a point beyond
# it does not project, so the plane must not gate it, whatever texel its (u, v) would name
TABLE_CAMERAS = {
    "opencv": ([float(PW), float(PH), 192.0, 189.5, 77.75, 62.0, -0.08, 0.03, 0.004, -0.007], 4),
    "k1_limit": ([float(PW), float(PH), 96.0, 96.0, 78.75, 60.75, 0.9, 0.0, 0.0, 0.0], 2),
}


@pytest.mark.parametrize("n", (65, 4097))
@pytest.mark.parametrize("name", list(TABLE_CAMERAS))
def test_points_match_the_restatement_on_the_camera_table(device, name, n):
    cam10, ndist = TABLE_CAMERAS[name]
    assert cam10[6:6 + ndist] == CC.CAMERAS[name]["params"][-ndist:] and ndist == CC.NDIST[name]
    X, T12, valid, occ = point_inputs(n, 5500 + n, cam10)
    ref = OC.points_visible_reference(X, valid, T12, (cam10, ndist), occ)
    T = T12.astype(np.float64)
    pc = X.astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:]
    at_limit = CC.r2_margin(cam10[6:6 + ndist], pc) <= CC.R2_REL_MARGIN
    fragile = ref["fragile"] | at_limit
    assert fragile.sum() <= 0.02 * n and not ref["near_edge"].any()
    with np.errstate(all="ignore"):
        xt, yt = np.floor(ref["u"] + 0.5), np.floor(ref["v"] + 0.5)
        lands = (pc[:, 2] > 1e-3) & ~ref["projects"] & (ref["u"] >= 0) & (ref["v"] >= 0) & (ref["u"] <= PW - 1) & (ref["v"] <= PH - 1)
        lands &= occ[np.where(lands, yt, 0).astype(int), np.where(lands, xt, 0).astype(int)] != 0
    lands &= valid != 0
    if n >= 1025:
        assert ref["gated"].sum() > n // 20 and (~ref["projects"]).sum() > n // 10 and (ref["valid"] != 0).sum() > n // 10
        if name in CC.LIMIT_CASES:  # beyond the range, inside the image, over an occluder texel: kept
            assert lands.sum() >= 10, lands.sum()
    d_occ = torch.from_numpy(occ).to(device)
    rec = torch.full((OC.RECORD,), SENTINEL, dtype=torch.int32, device=device)
    out_all = torch.full((n + TAIL,), CANARY, dtype=torch.uint8, device=device)
    out = out_all[:n]
    got, _ = OC.points_visible(torch.from_numpy(X).to(device).reshape(n, 3), torch.from_numpy(valid).to(device), T12,
                               (cam10, ndist), d_occ, record=rec, valid=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    words = rec.cpu().numpy()
    assert (out_all[n:] == CANARY).all() and set(np.unique(got)) <= {0, 1}
    keep = ~fragile
    assert np.array_equal(got[keep], ref["valid"][keep]), np.nonzero(got[keep] != ref["valid"][keep])
    assert (got[lands & keep] == 1).all()
    assert words[8:11].tolist() == [n, int(valid.sum()), int(got.sum())]
    if not fragile.any():
        assert words[8:11].tolist() == list(ref["counts"])


def test_points_bad_arguments_launch_nothing(device):
    X, T12, valid, occ = point_inputs(65, 1)
    d_X, d_occ = torch.from_numpy(X).to(device), torch.from_numpy(occ).to(device)
    out = torch.full((65,), CANARY, dtype=torch.uint8, device=device)
    rec = torch.full((OC.RECORD,), SENTINEL, dtype=torch.int32, device=device)
    L = _lib.lib()
    T = (ctypes.c_float * 12)(*[float(x) for x in T12])
    cam = (ctypes.c_float * 10)(*CAM10)
    small = (ctypes.c_float * 10)(*([80.0] + CAM10[1:]))
    s = _lib.stream_ptr(device)
    args = lambda **kw: [kw.get("p3d", d_X.data_ptr()), None, kw.get("n", 65), kw.get("T", T), kw.get("cam", cam),
                         kw.get("ndist", NDIST), kw.get("occ", d_occ.data_ptr()), kw.get("W", PW), kw.get("H", PH),
                         kw.get("out", out.data_ptr()), kw.get("rec", rec.data_ptr()), s]
    for kw in (dict(n=-1), dict(p3d=None), dict(out=None), dict(occ=None), dict(rec=None), dict(ndist=3), dict(W=0),
               dict(H=0), dict(cam=small), dict(T=None), dict(cam=None)):
        assert L.pxt_points_visible(*args(**kw)) == -1, kw
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (rec == SENTINEL).all()
    with pytest.raises(_lib.PxtError):
        ops.ops.points_visible(d_X, None, [0.0] * 12, [80.0] + CAM10[1:], NDIST, d_occ, out, rec)
