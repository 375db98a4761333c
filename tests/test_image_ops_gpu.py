"""Small image kernels (csrc/pxt_image.hip) vs numpy restatements of the cv2/numpy calls they replace
(oracle/image_oracle.py, itself checked on the CPU by tests/test_image_oracle_host.py).

Every output is allocated inside a larger buffer pre-filled with 0xCD: the bytes around it must come back untouched.

Run as a program, this file is the child of test_mask_sweep_byte_version: the single-pass part of the mask sweep
through the float entry, with whatever PXT_MASK_BYTES the environment holds.
"""
import os
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import image_oracle as IO
from oracle import unet_oracle as UO
from pixtrack_amd import _lib
from pixtrack_amd.ops import ops

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

FILL = 0xCD


# ------------------------------------------------------------------------------------------- guarded outputs
class Guarded:
    """`count` payloads of `nbytes` bytes each inside one uint8 device buffer filled with 0xCD, `guard` bytes (at least)
    before, between and after them; every payload starts at a 4-byte-aligned address, or that plus `skew`."""

    def __init__(self, device, nbytes, guard, count=1, skew=0):
        guard = (guard + 3) // 4 * 4
        self.nbytes, self.stride = nbytes, (nbytes + 3) // 4 * 4 + guard
        self.offsets = [guard + skew + k * self.stride for k in range(count)]
        self.buf = torch.full((guard + count * self.stride + 4,), FILL, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 4 == 0

    def ptr(self, k=0):
        return self.buf.data_ptr() + self.offsets[k]

    def tensor(self, k=0):
        return self.buf[self.offsets[k]:self.offsets[k] + self.nbytes]

    def payloads(self):
        """Host copies of the payloads [count, nbytes], after checking that every other byte is still 0xCD."""
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for o in self.offsets:
            inside[o:o + self.nbytes] = True
        touched = np.flatnonzero(~inside & (host != FILL))
        assert touched.size == 0, f"{touched.size} guard bytes written, first at offset {touched[0]} (payloads at {self.offsets[:3]}...)"
        return np.stack([host[o:o + self.nbytes] for o in self.offsets])


# ------------------------------------------------------------------------------------------- depth mask
# float depths for the float entry; which of them count as lit is the oracle's word (trunc(v * 255) mod 256 != 0):
# 0.003 gives 0, 256/255 wraps to 0, 257/255 wraps to 1, 511.9/255 to 255
_DEPTHS = np.array([0.003, 1.0 / 255.0, 1.0, 2.0, 256.0 / 255.0, 257.0 / 255.0, 511.9 / 255.0], np.float32)


def _depth_image(planes):
    """float32 [N, H, W, 4] whose `!= 0` plane is `planes`: the lit and the unlit values above spread over the pixels."""
    lit = IO.nonzero_plane(np.stack([_DEPTHS] * 4, -1)[None])[0].astype(bool)
    lit_v, unlit_v = _DEPTHS[lit], np.concatenate([np.zeros(1, np.float32), _DEPTHS[~lit]])
    assert lit_v.size >= 4 and unlit_v.size >= 3
    idx = np.arange(planes.size).reshape(planes.shape)
    d = np.where(planes != 0, lit_v[idx % lit_v.size], unlit_v[idx % unlit_v.size]).astype(np.float32)
    rgba = np.empty(planes.shape + (4,), np.float32)
    rgba[..., :3] = d[..., None]
    rgba[..., 3] = 0.5
    assert np.array_equal(IO.nonzero_plane(rgba), planes)
    return rgba


def _masks(device, planes, ne, nd, entries=("plane", "float")):
    """Both C entries on every plane of uint8 [N, H, W]; returns {entry: uint8 [N, H, W]} after the hygiene checks: mask
    bytes are 0 or 1, the bytes around each mask and around the 2 * H * W scratch bytes are untouched."""
    L = _lib.lib()
    N, H, W = planes.shape
    n = H * W
    guard = W + 64
    s = _lib.stream_ptr(device)
    iterated = 2 * (ne + nd) > 16
    got = {}
    for entry in entries:
        out = Guarded(device, n, guard, count=N)
        tmp = Guarded(device, 2 * n, guard)
        if entry == "plane":
            src = torch.from_numpy(planes).to(device)
            codes = [L.pxt_depth_mask_plane(src.data_ptr() + k * n, H, W, ne, nd, out.ptr(k), tmp.ptr() if iterated else None, s)
                     for k in range(N)]
        else:
            src = torch.from_numpy(_depth_image(planes)).to(device)
            codes = [L.pxt_depth_mask(src.data_ptr() + k * n * 16, H, W, ne, nd, out.ptr(k), tmp.ptr(), s) for k in range(N)]
        torch.cuda.synchronize()
        assert not any(codes), (entry, codes)
        m = out.payloads().reshape(N, H, W)
        tmp.payloads()
        assert m.max() <= 1, (entry, "mask bytes other than 0 / 1", np.unique(m))
        got[entry] = m
    return got


def _compare(got, ref, what):
    for entry, m in got.items():
        if not np.array_equal(m, ref):
            k, y, x = np.argwhere(m != ref)[0]
            raise AssertionError(f"{what} {entry} entry: {int((m != ref).sum())} wrong mask bytes, first in plane {k} at "
                                 f"(y {y}, x {x}): got {m[k, y, x]}, want {ref[k, y, x]}")


def _sweep_case(device, H, W, ne, nd, entries=("plane", "float")):
    planes = np.concatenate([IO.random_mask_plane(H, W, ne, nd)[None], IO.probe_planes(H, W)])
    _compare(_masks(device, planes, ne, nd, entries), IO.depth_mask(planes, ne, nd), f"{H}x{W} ({ne}, {nd})")


@pytest.mark.parametrize("H,W", IO.MASK_SHAPES)
def test_mask_sweep(device, H, W):
    """pxt_depth_mask_plane and pxt_depth_mask on the same planes, bit for bit the iterated 5x5 reference, at every
    setting of the sweep: R = 2 * (n_erode + n_dilate) of 0, 16 (the single-pass kernel's limit), 18 and 20 (the 5x5
    passes one by one).  The shapes cover partial and exact 64 x 16 tiles both ways, odd W, W % 4 of 0 (dword stores)
    to 3, single rows and columns.  Per case one random union of rectangles with speckles and pin-holes
    (IO.random_mask_plane; its masks are non-trivial, see the host test) and the seam probes: a lone lit pixel, and a
    lone hole, at every combination of x in {0, 1, 31, 32, 62, 63, 64, 65, W-1} and y in {0, 14, 15, 16, 17, H-1}, one
    per plane, whose mask is one exact box.  The float image carries 1/255, 1.0, 2.0, 257/255, 511.9/255 on lit pixels
    and 0, 0.003, 256/255 (wraps to 0) on the others.  Depths stay non-negative and finite: numpy's cast of negative or
    NaN floats to uint8 is not defined, so there is no reference for them."""
    for ne, nd in IO.MASK_SETTINGS:
        _sweep_case(device, H, W, ne, nd)


@pytest.mark.parametrize("H,W,ne,nd,y0,x0", [(60, 84, 1, 5, 15, 20), (60, 84, 1, 5, 0, 44), (97, 150, 2, 3, 67, 0),
                                              (60, 84, 2, 7, 15, 20), (40, 70, 0, 2, 10, 30)])
def test_depth_mask_matches_cv2_semantics(device, H, W, ne, nd, y0, x0):
    """(1, 5) is the tracker's setting (single fused pass); (2, 7) exceeds the fused kernel's halo
    and takes the iterated kernels; blobs touching the border exercise OpenCV's border rule."""
    rng = np.random.default_rng(1)
    depth = np.zeros((H, W, 4), np.float32)
    blob = np.zeros((H, W), np.float32)
    blob[y0:y0 + 30, x0:x0 + 40] = rng.uniform(0.5, 2.0, size=(30, 40))
    blob[rng.uniform(size=(H, W)) > 0.97] = 1.0   # speckles the erosion must remove
    blob[30, 40] = 0.0                            # pin-hole the erosion must widen
    blob[5, 5] = 0.003                            # < 1/255 -> uint8 0
    blob[6, 6] = 256.0 / 255.0                    # wraps to 0 in uint8 (Appendix D.6)
    depth[..., :3] = blob[..., None]
    ref = ((depth[..., 0] * 255.0).astype(np.int64) & 255) != 0
    ref = ref.astype(np.uint8)
    for _ in range(ne):
        ref = IO.morph5(ref, True)
    for _ in range(nd):
        ref = IO.morph5(ref, False)
    d = torch.from_numpy(depth).to(device)
    out = torch.zeros(H, W, dtype=torch.uint8, device=device)
    tmp = torch.zeros(2 * H * W, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().pxt_depth_mask(d.data_ptr(), H, W, ne, nd, out.data_ptr(), tmp.data_ptr(),
                                         _lib.stream_ptr(device)), "pxt_depth_mask")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert 0 < ref.sum() < H * W


@pytest.mark.parametrize("H,W,ne,nd", [(33, 129, 1, 5), (32, 256, 4, 4), (17, 65, 0, 1), (16, 64, 0, 0), (48, 130, 2, 8),
                                       (20, 200, 0, 9)])
def test_mask_ops(device, H, W, ne, nd):
    """The same through ops.depth_mask_plane / ops.depth_mask; above R = 16 the plane op allocates its own scratch."""
    nz = IO.random_mask_plane(H, W, ne, nd)
    ref = IO.depth_mask(nz, ne, nd)
    m1 = torch.full((H, W), FILL, dtype=torch.uint8, device=device)
    ops.depth_mask_plane(torch.from_numpy(nz).to(device), ne, nd, m1)
    m2 = torch.full((H, W), FILL, dtype=torch.uint8, device=device)
    ops.depth_mask(torch.from_numpy(_depth_image(nz)).to(device), ne, nd, m2, torch.empty(2 * H * W, dtype=torch.uint8, device=device))
    _compare({"plane op": m1.cpu().numpy()[None], "float op": m2.cpu().numpy()[None]}, ref[None], f"{H}x{W} ({ne}, {nd})")


def test_mask_output_need_not_be_aligned_when_w_is_not_a_multiple_of_4(device):
    """include/pixtrack_hip.h: mask_out is 4-byte aligned when W % 4 == 0 (dword stores); any address otherwise."""
    H, W, ne, nd = 17, 65, 1, 5
    nz = IO.random_mask_plane(H, W, ne, nd)
    src = torch.from_numpy(nz).to(device)
    for skew in (1, 2, 3):
        out = Guarded(device, H * W, W + 64, skew=skew)
        assert out.ptr() % 4 == skew
        _lib.check(_lib.lib().pxt_depth_mask_plane(src.data_ptr(), H, W, ne, nd, out.ptr(), None, _lib.stream_ptr(device)), "mask")
        ops.depth_mask_plane(src, ne, nd, out.tensor().view(H, W))       # the op accepts it as well
        torch.cuda.synchronize()
        assert np.array_equal(out.payloads().reshape(H, W), IO.depth_mask(nz, ne, nd))


def _single_pass_sweep(device, entries):
    n = 0
    for H, W, ne, nd in IO.mask_sweep():
        if 2 * (ne + nd) <= 16:
            _sweep_case(device, H, W, ne, nd, entries)
            n += 1
    return n


def test_mask_sweep_byte_version(device):
    """PXT_MASK_BYTES=1 selects depth_mask_fused_kernel (byte planes in LDS) for pxt_depth_mask; the knob is read once
    per process, so the single-pass part of the sweep runs in one fresh child."""
    env = dict(os.environ, PXT_MASK_BYTES="1", PYTHONPATH=os.pathsep.join([str(ROOT), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, str(Path(__file__).resolve())], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert f"MASK_SWEEP_OK bytes=1 cases={len(IO.MASK_SHAPES) * 11}" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------------- uint8 conversion
_COLOURS = np.array([0.0, 0.5 / 255, 1 / 255, 254.999 / 255, 1.0, 256 / 255, 300 / 255], np.float32)


def test_rgba_to_u8(device):
    rng = np.random.default_rng(2)
    rgba = rng.uniform(0, 1, size=(33, 47, 4)).astype(np.float32)
    ref = rgba.copy()
    ref[ref[:, :, 3] < 0.25] = 0.0
    ref = (ref[:, :, :3] * 255.0).astype(np.uint8)
    d = torch.from_numpy(rgba).to(device)
    out = torch.zeros(33, 47, 3, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().pxt_rgba_to_u8(d.data_ptr(), 33, 47, 0.25, out.data_ptr(), _lib.stream_ptr(device)), "u8")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("thresh", [0.0, 0.25])
@pytest.mark.parametrize("H,W", [(33, 47), (1, 1)])
def test_rgba_to_u8_edge_values(device, H, W, thresh):
    """Exactly the oracle: colour zeroed only where alpha < thresh (alpha == thresh keeps it), then trunc(v * 255) mod
    256 - on values that sit on the edges (0.5/255, 1/255, 254.999/255, 1.0) and that wrap (256/255, 300/255)."""
    rng = np.random.default_rng(2)
    t = np.float32(thresh)
    alphas = np.array([0.0, np.nextafter(t, np.float32(-1)) if thresh > 0 else 0.0, t, np.nextafter(t, np.float32(1)), 0.6, 1.0],
                      np.float32)
    images = []
    for rep in range(3 if (H, W) == (1, 1) else 1):
        rgba = np.empty((H, W, 4), np.float32)
        pick = rng.integers(0, 2 * _COLOURS.size, size=(H, W, 3))                 # half fixed values, half noise
        rgba[..., :3] = np.where(pick < _COLOURS.size, _COLOURS[pick % _COLOURS.size], rng.uniform(0, 1, size=(H, W, 3)))
        rgba[..., 3] = alphas[(np.arange(H * W).reshape(H, W) + rep) % alphas.size]
        if (H, W) == (1, 1):
            rgba[0, 0] = [(1.0, 256 / 255, 0.5 / 255, t), (1 / 255, 1.0, 300 / 255, alphas[1]), (1.0, 1.0, 1.0, alphas[3])][rep]
        images.append(rgba)
    for rgba in images:
        ref = IO.rgba_to_u8(rgba, thresh)
        d = torch.from_numpy(rgba).to(device)
        out = Guarded(device, H * W * 3, 3 * W + 64)
        _lib.check(_lib.lib().pxt_rgba_to_u8(d.data_ptr(), H, W, float(thresh), out.ptr(), _lib.stream_ptr(device)), "u8")
        torch.cuda.synchronize()
        assert np.array_equal(out.payloads().reshape(H, W, 3), ref)
        kept = rgba[..., 3] == t
        assert (H, W) == (1, 1) or (ref[kept].any() and not ref[rgba[..., 3] < t].any())   # the threshold case is in the data


# ------------------------------------------------------------------------------------------- resize
RESIZE_PAIRS = [(48, 64, 48, 64), (48, 64, 24, 32), (48, 64, 96, 128), (45, 80, 24, 43), (7, 5, 20, 13), (1, 9, 1, 4),
                (9, 1, 4, 1), (30, 40, 1, 1)]


def _resize_gpu(device, img, Ho, Wo):
    H, W, C = img.shape
    d = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(device)
    out = Guarded(device, Ho * Wo * C * 4, 4 * C * Wo + 64)
    _lib.check(_lib.lib().pxt_resize_linear(d.data_ptr(), H, W, C, out.ptr(), Ho, Wo, _lib.stream_ptr(device)), "rs")
    torch.cuda.synchronize()
    return out.payloads()[0].view(np.float32).reshape(Ho, Wo, C), out.tensor().view(torch.float32).view(Ho, Wo, C), d


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H,W,Ho,Wo", RESIZE_PAIRS)
def test_resize_linear_sweep(device, H, W, Ho, Wo, C):
    """pxt_resize_linear vs the same taps with float64 lerps: |out - ref| <= 8 * 2^-23 * max|src| (three float32 lerps
    of values bounded by max|src|, each at most about 2 ulp at that magnitude); the identity is bit-exact (ax = ay = 0,
    a * 1 + b * 0).  The source is a distinct ramp per channel plus noise, so that a channel or row / column swap is off
    by far more than the bound."""
    rng = np.random.default_rng(3)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    img = (10.0 * c + (1 + c) * x + (2.5 - c) * y + rng.uniform(0, 5, size=(H, W, C))).astype(np.float32)
    got, got_dev, src_dev = _resize_gpu(device, img, Ho, Wo)
    if (H, W) == (Ho, Wo):
        assert torch.equal(got_dev, src_dev)
        return
    err = np.abs(got.astype(np.float64) - IO.resize_linear64(img, Wo, Ho)).max()
    bound = 8 * 2.0 ** -23 * np.abs(img).max()
    print(f"resize_linear {H}x{W}x{C} -> {Ho}x{Wo}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("H,W,Ho,Wo", [(480, 640, 192, 256), (100, 75, 33, 25), (48, 64, 96, 128)])
def test_resize_linear(device, H, W, Ho, Wo):
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32)
    ref = UO.cv2_resize_linear(img, Wo, Ho)
    d = torch.from_numpy(img).to(device)
    out = torch.zeros(Ho, Wo, 3, device=device)
    _lib.check(_lib.lib().pxt_resize_linear(d.data_ptr(), H, W, 3, out.data_ptr(), Ho, Wo, _lib.stream_ptr(device)), "rs")
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-3


def _activity_sources(H, W):
    """(name, mask or None, uint8 image or None): blobs and sparse single pixels at corners and edges as a mask; uint8
    images whose only non-zero channel is the first, the second, the third; one with mixed channels."""
    rng = np.random.default_rng(H * 1000 + W)
    blob = IO.random_mask_plane(H, W, 0, 0)
    sparse = np.zeros((H, W), np.uint8)
    for yy, xx in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (0, W // 2), (H - 1, W // 3), (H // 3, W - 1),
                   (H // 2, W // 2)}:
        sparse[yy, xx] = 1
    lone = np.zeros((H, W), np.uint8)
    lone[(2 * H) // 3, (2 * W) // 3] = 1
    yield "mask blobs", blob, None
    yield "mask sparse", sparse, None
    yield "mask lone pixel", lone, None
    yield "mask empty", np.zeros((H, W), np.uint8), None
    for ch in range(3):
        u8 = np.zeros((H, W, 3), np.uint8)
        u8[..., ch] = (sparse if ch != 1 else lone) * rng.integers(1, 256, size=(H, W))
        yield f"u8 channel {ch} only", None, u8
    u8 = (blob[..., None] * rng.integers(0, 256, size=(H, W, 3))).astype(np.uint8)
    yield "u8 blobs", None, u8


@pytest.mark.parametrize("H,W,Ho,Wo", RESIZE_PAIRS + [(54, 96, 29, 52)])
def test_resize_activity(device, H, W, Ho, Wo):
    """pxt_resize_activity, at the C ABI and through ops.resize_activity, from a mask and from a uint8 image.
    Cover: no pixel that pxt_resize_linear makes non-zero (of the uint8 image, or of a nowhere-zero image times the
    mask) has active == 0 - the reason the kernel exists.  Upper bound: active lies inside the reference with a window
    one pixel larger on every side (an always-1 plane fails this).  Exact equality with the reference only where both
    size ratios are multiples of 1/16: there (x + 0.5) * s - 0.5 is exact in float32 whether or not the compiler fuses
    the multiply and the subtraction; elsewhere a fused and an unfused evaluation may legitimately floor differently
    at an integer."""
    L = _lib.lib()
    exact = Fraction(H, Ho).denominator in (1, 2, 4, 8, 16) and Fraction(W, Wo).denominator in (1, 2, 4, 8, 16)
    rng = np.random.default_rng(11)
    dense = rng.uniform(0.5, 2.0, size=(H, W, 3)).astype(np.float32)
    for name, mask, u8 in _activity_sources(H, W):
        src = mask if mask is not None else u8
        d_src = torch.from_numpy(src).to(device)
        out = Guarded(device, Ho * Wo, Wo + 64)
        _lib.check(L.pxt_resize_activity(d_src.data_ptr() if mask is not None else None, d_src.data_ptr() if u8 is not None else None,
                                         H, W, Ho, Wo, out.ptr(), _lib.stream_ptr(device)), "activity")
        via_op = torch.full((Ho, Wo), FILL, dtype=torch.uint8, device=device)
        ops.resize_activity(d_src if mask is not None else None, d_src if u8 is not None else None, H, W, via_op)
        torch.cuda.synchronize()
        active = out.payloads().reshape(Ho, Wo)
        assert active.max() <= 1 and np.array_equal(via_op.cpu().numpy(), active), name
        src_active = mask if mask is not None else u8.any(-1)
        image = dense * mask[..., None] if mask is not None else u8.astype(np.float32)
        resized, _, _ = _resize_gpu(device, image, Ho, Wo)
        uncovered = (resized != 0).any(-1) & (active == 0)
        assert not uncovered.any(), (name, "non-zero resized pixels marked inactive", np.argwhere(uncovered)[:4])
        loose = IO.resize_activity(src_active, Ho, Wo, grow=1)
        assert not (active & (1 - loose)).any(), (name, "active outside the grown window", np.argwhere(active & (1 - loose))[:4])
        if exact:
            ref = IO.resize_activity(src_active, Ho, Wo)
            assert np.array_equal(active, ref), (name, np.argwhere(active != ref)[:4])


if __name__ == "__main__":
    n_cases = _single_pass_sweep(torch.device("cuda:0"), ("float",))
    print(f"MASK_SWEEP_OK bytes={os.environ.get('PXT_MASK_BYTES', '0')} cases={n_cases}")
