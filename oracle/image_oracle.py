"""CPU ORACLE (test infrastructure, NOT product code) for the small image kernels of csrc/pxt_image.hip.

Plain numpy restatements of the documented semantics (include/pixtrack_hip.h, the comments above each kernel): the
`uint8(depth * 255) != 0` plane, the iterated 5x5 erosions / dilations of get_mask with OpenCV's default borders, the
uint8 conversion of a render, bilinear resizing with float64 lerps, and the "may be non-zero" plane of a resized image.
tests/test_image_oracle_host.py checks each of them against an independent statement, so that the GPU tests rest on
something verified.  The second half generates the inputs of the mask sweep (tests/test_image_ops_gpu.py); the host
test checks that they are not trivial.

Only tests/ may import this.
"""
from __future__ import annotations

from typing import Iterator, List, Tuple

import numpy as np

_F = np.float32


# ------------------------------------------------------------------------------------------- the operations
def _trunc_u8(v: np.ndarray) -> np.ndarray:
    """float32 -> uint8 as numpy's astype does it for non-negative finite values: truncate, keep the low 8 bits."""
    return (v.astype(np.int64) & 255).astype(np.uint8)


def nonzero_plane(depth_rgba: np.ndarray) -> np.ndarray:
    """`uint8(depth * 255) != 0` of channel 0 of a float32 [..., H, W, 4] depth image (all three colour channels carry
    the same depth).  Negative or non-finite depths are outside the contract: numpy's cast of them is not defined."""
    v = np.asarray(depth_rgba, dtype=_F)[..., 0] * _F(255.0)
    return (_trunc_u8(v) != 0).astype(np.uint8)


def morph5(img: np.ndarray, erode: bool) -> np.ndarray:
    """cv2.erode / cv2.dilate with a 5x5 all-ones kernel and the default border (pixels outside the image never win:
    +inf for the erosion, -inf for the dilation) on a uint8 [..., H, W] plane; leading dimensions are a batch."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape[-2:]
    pad = np.full(img.shape[:-2] + (H + 4, W + 4), 255 if erode else 0, dtype=np.uint8)
    pad[..., 2:-2, 2:-2] = img
    op = np.minimum if erode else np.maximum
    rows = pad[..., :, 0:W]
    for dx in range(1, 5):           # the 5x5 box is a 1x5 box followed by a 5x1 box
        rows = op(rows, pad[..., :, dx:dx + W])
    out = rows[..., 0:H, :]
    for dy in range(1, 5):
        out = op(out, rows[..., dy:dy + H, :])
    return np.ascontiguousarray(out)


def depth_mask(nz: np.ndarray, n_erode: int, n_dilate: int) -> np.ndarray:
    """get_mask's morphology on a 0/1 plane: n_erode erosions, then n_dilate dilations, one 5x5 pass after the other."""
    m = (np.asarray(nz) != 0).astype(np.uint8)
    for _ in range(n_erode):
        m = morph5(m, True)
    for _ in range(n_dilate):
        m = morph5(m, False)
    return m


def rgba_to_u8(rgba: np.ndarray, thresh: float) -> np.ndarray:
    """get_nerf_image's tail: colour zeroed where alpha < thresh (and only there), * 255, astype(uint8)."""
    rgba = np.asarray(rgba, dtype=_F)
    rgb = rgba[..., :3].copy()
    rgb[rgba[..., 3] < _F(thresh)] = 0.0
    return _trunc_u8(rgb * _F(255.0))


def _tap_origin(n_out: int, n_in: int) -> np.ndarray:
    """floor((x + 0.5f) * (float(n_in) / float(n_out)) - 0.5f), every step rounded to float32."""
    s = _F(n_in) / _F(n_out)
    t = (np.arange(n_out, dtype=_F) + _F(0.5)) * s
    return np.floor(t - _F(0.5)).astype(np.int64)


def resize_activity(src_active: np.ndarray, Ho: int, Wo: int, grow: int = 0) -> np.ndarray:
    """Which pixels of an [H, W] -> [Ho, Wo] bilinear resize may be non-zero: the OR of `src_active` over
    [y0 - 1, y0 + 2] x [x0 - 1, x0 + 2] clipped to the image, (y0, x0) the upper-left bilinear tap.  `grow` widens the
    window by that many pixels on every side (the upper bound of the GPU test)."""
    a = (np.asarray(src_active) != 0)
    H, W = a.shape
    y0, x0 = _tap_origin(Ho, H), _tap_origin(Wo, W)
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    ylo, yhi = np.maximum(y0 - 1 - grow, 0), np.minimum(y0 + 2 + grow, H - 1) + 1
    xlo, xhi = np.maximum(x0 - 1 - grow, 0), np.minimum(x0 + 2 + grow, W - 1) + 1
    yhi, xhi = np.maximum(yhi, ylo), np.maximum(xhi, xlo)      # an empty window sums to 0
    cnt = (S[yhi][:, xhi] - S[ylo][:, xhi] - S[yhi][:, xlo] + S[ylo][:, xlo])
    return (cnt > 0).astype(np.uint8)


def resize_linear64(img: np.ndarray, Wo: int, Ho: int) -> np.ndarray:
    """cv2.resize(img, (Wo, Ho), INTER_LINEAR) on float32 HWC with the tap positions and weights computed in float32
    (as unet_oracle.cv2_resize_linear and the kernel do) and the three lerps in float64.  Returns float64."""
    img = np.asarray(img, dtype=_F)
    H, W = img.shape[:2]

    def taps(n_out, n_in):
        s = _F(n_in) / _F(n_out)
        f = (np.arange(n_out, dtype=_F) + _F(0.5)) * s - _F(0.5)
        i0 = np.floor(f).astype(np.int64)
        a = (f - i0.astype(_F)).astype(_F)
        lo, hi = i0 < 0, i0 >= n_in - 1
        a[lo | hi] = 0
        i0[lo] = 0
        i0[hi] = n_in - 1
        return i0, np.minimum(i0 + 1, n_in - 1), a.astype(np.float64)

    x0, x1, ax = taps(Wo, W)
    y0, y1, ay = taps(Ho, H)
    src = img.astype(np.float64)
    ax, ay = ax[None, :, None], ay[:, None, None]
    top = src[y0][:, x0] * (1.0 - ax) + src[y0][:, x1] * ax
    bot = src[y1][:, x0] * (1.0 - ax) + src[y1][:, x1] * ax
    return top * (1.0 - ay) + bot * ay


# ------------------------------------------------------------------------------------------- inputs of the mask sweep
MASK_SHAPES: List[Tuple[int, int]] = [(1, 1), (1, 64), (16, 1), (5, 7), (15, 63), (16, 64), (17, 65), (31, 127),
                                      (33, 129), (48, 130), (20, 200), (32, 256)]
# (n_erode, n_dilate); the single-pass kernels take R = 2 * (n_erode + n_dilate) <= 16, the 5x5 passes run one by one above
MASK_SETTINGS: List[Tuple[int, int]] = [(0, 0), (1, 0), (0, 1), (1, 5), (2, 3),
                                        (0, 8), (8, 0), (4, 4), (3, 5), (1, 7), (7, 1),
                                        (4, 5), (9, 0), (0, 9), (2, 8)]
PROBE_X = (0, 1, 31, 32, 62, 63, 64, 65)   # and W - 1: either side of the 64-column tile seam and of the two 64-bit halves
PROBE_Y = (0, 14, 15, 16, 17)              # and H - 1: either side of the 16-row tile seam


def mask_case_seed(H: int, W: int, n_erode: int, n_dilate: int) -> int:
    return ((H * 1009 + W) * 31 + n_erode) * 31 + n_dilate


def random_mask_plane(H: int, W: int, n_erode: int, n_dilate: int) -> np.ndarray:
    """A 0/1 plane for one case of the sweep: the union of 1 to 4 rectangles that may cross any image border, with 3 %
    of the pixels flipped (speckles outside, pin-holes inside).

    Left like that, most cases erode to nothing (a pin-hole every 33 pixels leaves no (4 n_erode + 1)^2 box intact) or
    dilate to everything.  So, where the image has room for it in at least one direction, one more rectangle with sides
    >= 4 n_erode + 3 is added and kept free of flips: at least 3 x 3 of it survive the erosion.  With n_erode = 0 the
    3 % would hold for the pin-holes only: without erosion every speckle survives
    and grows to a (4 n_dilate + 1)^2 box, so there the speckles (not the pin-holes) are thinned to an expected one
    per two such boxes.  The rectangles are at most about half the image in either direction so that the dilation has
    something left to fill.  A dimension shorter than 4 n_erode + 3 is spanned whole by the kept rectangle (the border
    is neutral for the erosion)."""
    rng = np.random.default_rng(mask_case_seed(H, W, n_erode, n_dilate))
    nz = np.zeros((H, W), np.uint8)
    for _ in range(int(rng.integers(1, 5))):
        h, w = int(rng.integers(1, max(H // 2, 1) + 1)), int(rng.integers(1, max(W // 2, 1) + 1))
        y, x = int(rng.integers(-(h // 2), H)), int(rng.integers(-(w // 2), W))
        nz[max(y, 0):y + h, max(x, 0):x + w] = 1
    flip = rng.uniform(size=(H, W))
    rate = np.full((H, W), 0.03)
    if n_erode == 0:
        rate[nz == 0] = min(0.03, 0.5 / (4 * n_dilate + 1) ** 2)
    side = 4 * n_erode + 3
    keep = None
    if max(H, W) >= side:

        def extent(n):  # pixels outside the image are neutral for the erosion: a full-length run needs no margin
            if n < side:
                return slice(0, n)
            ln = int(rng.integers(side, max(n // 2, side) + 1))
            lo = int(rng.integers(0, n - ln + 1))
            return slice(lo, lo + ln)

        keep = (extent(H), extent(W))
    nz = np.where(flip < rate, 1 - nz, nz).astype(np.uint8)
    if keep is not None:
        nz[keep] = 1
    return nz


def probe_positions(H: int, W: int) -> List[Tuple[int, int]]:
    xs = sorted({x for x in PROBE_X + (W - 1,) if 0 <= x < W})
    ys = sorted({y for y in PROBE_Y + (H - 1,) if 0 <= y < H})
    return [(y, x) for y in ys for x in xs]


def probe_planes(H: int, W: int) -> np.ndarray:
    """uint8 [2 P, H, W]: for each of the P probe positions an all-zero plane with that one pixel lit, then an all-one
    plane with that one pixel cleared.  One probe per plane: the mask of each is one exact box."""
    pos = probe_positions(H, W)
    out = np.zeros((2 * len(pos), H, W), np.uint8)
    out[len(pos):] = 1
    for k, (y, x) in enumerate(pos):
        out[k, y, x] = 1
        out[len(pos) + k, y, x] = 0
    return out


def mask_sweep() -> Iterator[Tuple[int, int, int, int]]:
    for H, W in MASK_SHAPES:
        for ne, nd in MASK_SETTINGS:
            yield H, W, ne, nd
