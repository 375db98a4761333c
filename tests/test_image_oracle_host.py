"""oracle/image_oracle.py against independent statements of the same operations (no GPU): the GPU tests of
tests/test_image_ops_gpu.py compare the kernels with this module, so it is checked first."""
import numpy as np
import pytest

from oracle import image_oracle as IO
from oracle import unet_oracle as UO


def _box(img, r, erode):
    """One (2r+1)^2 box erosion / dilation over the in-image pixels, pixel by pixel."""
    H, W = img.shape
    out = np.empty_like(img)
    for y in range(H):
        for x in range(W):
            win = img[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
            out[y, x] = win.min() if erode else win.max()
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (6, 11), (23, 19)])
def test_iterated_5x5_is_one_box(H, W):
    """n iterated 5x5 erosions (dilations) with OpenCV's default borders = one (4n+1)^2 box over the in-image pixels."""
    rng = np.random.default_rng(H * 100 + W)
    for density in (0.15, 0.5, 0.9):
        img = (rng.uniform(size=(H, W)) < density).astype(np.uint8)
        for n in (1, 2, 4):
            for erode in (True, False):
                it = img
                for _ in range(n):
                    it = IO.morph5(it, erode)
                assert np.array_equal(it, _box(img, 2 * n, erode)), (density, n, erode)
    # ... and depth_mask is the erosion box followed by the dilation box
    img = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
    assert np.array_equal(IO.depth_mask(img, 1, 2), _box(_box(img, 2, True), 4, False))


def test_morph5_takes_a_batch():
    rng = np.random.default_rng(5)
    imgs = (rng.uniform(size=(3, 9, 13)) < 0.6).astype(np.uint8)
    for erode in (True, False):
        both = IO.morph5(imgs, erode)
        for k in range(3):
            assert np.array_equal(both[k], IO.morph5(imgs[k], erode))


def test_depth_mask_hand_written_7x9():
    """A 5x5 block in the top-left corner, a 5x3 block in the bottom-right corner with one more pixel above it, and a
    speckle.  A pixel survives the erosion when every in-image pixel of its 5x5 window is lit (outside counts as lit)."""
    nz = np.array([[1, 1, 1, 1, 1, 0, 0, 0, 0],
                   [1, 1, 1, 1, 1, 0, 0, 0, 1],
                   [1, 1, 1, 1, 1, 0, 1, 1, 1],
                   [1, 1, 1, 1, 1, 0, 1, 1, 1],
                   [1, 1, 1, 1, 1, 0, 1, 1, 1],
                   [0, 0, 0, 0, 0, 0, 1, 1, 1],
                   [0, 1, 0, 0, 0, 0, 1, 1, 1]], np.uint8)
    # left block: x + 2 <= 4 and y + 2 <= 4.  Right block: the window must start at column 6 (x = 8; columns 9, 10 are
    # outside) and at row 2 or below (y >= 4; rows 7, 8 are outside).  The speckle at (6, 1) goes.
    eroded = np.zeros((7, 9), np.uint8)
    eroded[0:3, 0:3] = 1
    eroded[4:7, 8] = 1
    assert np.array_equal(IO.depth_mask(nz, 1, 0), eroded)
    dil = np.zeros((7, 9), np.uint8)
    dil[0:5, 0:5] = 1
    dil[2:7, 6:9] = 1
    assert np.array_equal(IO.depth_mask(nz, 1, 1), dil)
    # without the erosion the dilation fills the image: every pixel has a lit one within 2
    assert IO.depth_mask(nz, 0, 1).all()
    assert np.array_equal(IO.depth_mask(nz, 0, 0), nz)


def test_nonzero_plane_and_rgba_to_u8_wrap():
    vals = np.array([0.0, 0.003, 1 / 255, 0.5 / 255, 1.0, 2.0, 256 / 255, 257 / 255, 511.9 / 255, 254.999 / 255, 300 / 255],
                    np.float32)
    want = np.array([0, 0, 1, 0, 255, 254, 0, 1, 255, 254, 44], np.uint8)   # trunc(v * 255) mod 256
    rgba = np.zeros((1, vals.size, 4), np.float32)
    rgba[0, :, :3] = vals[:, None]
    rgba[0, :, 3] = 0.25
    assert np.array_equal(IO.nonzero_plane(rgba)[0], (want != 0).astype(np.uint8))
    assert np.array_equal(IO.rgba_to_u8(rgba, 0.25)[0, :, 1], want)      # alpha == thresh is kept
    assert not IO.rgba_to_u8(rgba, np.nextafter(np.float32(0.25), np.float32(1))).any()
    assert np.array_equal(IO.rgba_to_u8(rgba, 0.0)[0, :, 2], want)


@pytest.mark.parametrize("H,W,Ho,Wo", [(48, 64, 48, 64), (48, 64, 24, 32), (48, 64, 96, 128), (45, 80, 24, 43), (7, 5, 20, 13),
                                       (1, 9, 1, 4), (9, 1, 4, 1), (30, 40, 1, 1)])
def test_resize_linear64_agrees_with_the_float32_restatement(H, W, Ho, Wo):
    """Same taps and weights, lerps in float64 vs float32: three lerps of values bounded by max|src|, each at most about
    2 ulp at that magnitude."""
    rng = np.random.default_rng(7)
    img = rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32)
    r64 = IO.resize_linear64(img, Wo, Ho)
    assert r64.dtype == np.float64 and r64.shape == (Ho, Wo, 3)
    r32 = UO.cv2_resize_linear(img, Wo, Ho)
    assert np.abs(r32 - r64).max() <= 8 * 2.0 ** -23 * np.abs(img).max()
    if (H, W) == (Ho, Wo):
        assert np.array_equal(r64, img.astype(np.float64))


def test_resize_activity_window():
    """Halving 8 -> 4: output x reads taps 2x, 2x + 1, so the window is source [2x - 1, 2x + 2]; one lit source pixel at
    5 activates outputs 2 (window 3..6) and 3 (window 5..7) and nothing else.  `grow` adds a pixel per side."""
    src = np.zeros((8, 8), np.uint8)
    src[5, 5] = 1
    want = np.zeros((4, 4), np.uint8)
    want[2:4, 2:4] = 1
    assert np.array_equal(IO.resize_activity(src, 4, 4), want)
    want[1:4, 1:4] = 1     # output 1: window 1..4, grown 0..5
    assert np.array_equal(IO.resize_activity(src, 4, 4, grow=1), want)
    # identity: x0 = x, window [x - 1, x + 2]
    ident = np.zeros((8, 8), np.uint8)
    ident[3:7, 3:7] = 1
    assert np.array_equal(IO.resize_activity(src, 8, 8), ident)
    assert not IO.resize_activity(np.zeros((5, 3)), 9, 2).any() and IO.resize_activity(np.ones((1, 1)), 3, 4).all()


def test_mask_sweep_inputs_are_not_trivial():
    """The sweep's random planes, judged on the reference alone: at least 60 % of the cases have a mask that is neither
    empty nor full, and so has every setting and every shape with min(H, W) >= 31."""
    live = {}
    for H, W, ne, nd in IO.mask_sweep():
        nz = IO.random_mask_plane(H, W, ne, nd)
        assert nz.shape == (H, W) and nz.dtype == np.uint8 and nz.max() <= 1
        assert np.array_equal(nz, IO.random_mask_plane(H, W, ne, nd))   # the GPU test sees the same planes
        s = int(IO.depth_mask(nz, ne, nd).sum())
        live[(H, W, ne, nd)] = 0 < s < H * W
    assert len(live) == len(IO.MASK_SHAPES) * len(IO.MASK_SETTINGS) == 180
    assert np.mean(list(live.values())) >= 0.6
    for ne, nd in IO.MASK_SETTINGS:
        assert any(v for k, v in live.items() if k[2:] == (ne, nd)), (ne, nd)
    for H, W in IO.MASK_SHAPES:
        if min(H, W) >= 31:
            assert any(v for k, v in live.items() if k[:2] == (H, W)), (H, W)


def test_probe_planes_hold_one_probe_each():
    for H, W in IO.MASK_SHAPES:
        pos = IO.probe_positions(H, W)
        planes = IO.probe_planes(H, W)
        assert planes.shape == (2 * len(pos), H, W)
        assert (planes[:len(pos)].reshape(len(pos), -1).sum(1) == 1).all()
        assert (planes[len(pos):].reshape(len(pos), -1).sum(1) == H * W - 1).all()
        assert (H - 1, W - 1) in pos and (0, 0) in pos
    assert len(IO.probe_positions(32, 256)) == 6 * 9
    # a lit probe's mask is the (4 n_dilate + 1)^2 box around it, clipped to the image
    m = IO.depth_mask(IO.probe_planes(33, 129)[IO.probe_positions(33, 129).index((16, 64))], 0, 3)
    want = np.zeros((33, 129), np.uint8)
    want[10:23, 58:71] = 1
    assert np.array_equal(m, want)
