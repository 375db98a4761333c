"""Query tiles, the marking rule on the host (pxt_unet_query_tiles_host: the device kernel's own functions, no GPU).

The rule, restated here from the issue and from the LM's loads, not from the kernel's expressions: every point in front
of the camera - valid or not - takes the texels the refine kernel's point evaluation would load around floor(u, v):
columns ix0 - 1 .. ix0 + 2 and rows iy0 - 1 .. iy0 + 2, each clamped into the map; that box grows by the margin on every
side and is clipped to the map; every tile of the last layer it meets is marked.  The layer before takes the tiles under
the marked tiles' up-sampling patches, exactly as for reference tiles (tests/test_reference_tiles_gpu.py restates that).

Points are (x, y, 1) under the identity pose and a camera with f = 1, c = 0: the projection is exact in any arithmetic."""
import ctypes as C
import math

import numpy as np
import pytest

from pixtrack_amd import _lib

IDENTITY = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]
PXT_E_ARG = -1  # (include/pixtrack_hip.h)


def replica_fine(xyz, fine_h, fine_w, margin, window=None, rows=16):
    x0, y0, _full_w, _full_h = window if window is not None else (0, 0, fine_w, fine_h)
    fine = np.zeros((-(-fine_h // rows), -(-fine_w // 16)), np.uint8)
    for x, y, z in np.asarray(xyz, np.float64):
        if not z > 1e-3:
            continue
        iu, iv = int(math.floor(x / z)) - x0, int(math.floor(y / z)) - y0
        xa, xb = (min(max(iu + d, 0), fine_w - 1) for d in (-1, 2))
        ya, yb = (min(max(iv + d, 0), fine_h - 1) for d in (-1, 2))
        xa, xb = max(xa - margin, 0), min(xb + margin, fine_w - 1)
        ya, yb = max(ya - margin, 0), min(yb + margin, fine_h - 1)
        fine[ya // rows:yb // rows + 1, xa // 16:xb // 16 + 1] = 1
    return fine


def replica_low(fine, fine_h, fine_w, fine_rows=16, low_rows=16):
    """The layer before (see the reference-tile test): the low rows / columns behind the one-pixel halo of a needed tile."""
    low_h, low_w = fine_h // 2, fine_w // 2
    low = np.zeros((-(-low_h // low_rows), -(-low_w // 16)), np.uint8)

    def sources(g0, g1, n):
        out = set()
        for g in range(g0 - 1, g1 + 1):
            s = int(math.floor(max((g + 0.5) / 2 - 0.5, 0.0)))
            out |= {min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1)}
        return out

    for r, c in zip(*np.nonzero(fine)):
        for ly in sources(r * fine_rows, (r + 1) * fine_rows, low_h):
            for lx in sources(c * 16, (c + 1) * 16, low_w):
                low[ly // low_rows, lx // 16] = 1
    return low


def record(xyz, margin, full, windowed, pad=4):
    qry = _lib.UnetQueryPoints()
    pts = qry.points
    pts.p3d, pts.n_points = xyz.ctypes.data, len(xyz)
    pts.T[:] = IDENTITY
    pts.cam[:] = [float(full[2]), float(full[3]), 1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0]
    pts.ndist, pts.pad = 0, pad
    pts.x0, pts.y0, pts.full_w, pts.full_h = full if windowed else (0, 0, 0, 0)
    qry.margin = margin
    return qry


def host_flags(pts, fh, fw, rows=(16, 16)):
    fine = np.full((-(-fh // rows[0]), -(-fw // 16)), 9, np.uint8)
    low = np.full((-(-(fh // 2) // rows[1]), -(-(fw // 2) // 16)), 9, np.uint8)
    _lib.check(_lib.lib().pxt_unet_query_tiles_host(C.byref(pts), fh, fw, rows[0], rows[1], fine.ctypes.data,
                                                    low.ctypes.data), "pxt_unet_query_tiles_host")
    return fine, low


def groups(fw, fh, x0=0, y0=0):
    """Named groups of points of an fw x fh map at (x0, y0) of its level; each is checked alone and all together."""
    seams = [(x0 + x, y0 + y, 1.0) for x in (15.999, 16.0, 17.0, 14.0, 31.999, 32.0) for y in (15.999, 16.0, 18.5, 13.2)
             if x < fw and y < fh]
    corners = [(x0 + x, y0 + y, 1.0) for x in (0.0, 0.5, fw - 1.0, fw - 1.5) for y in (0.0, 0.5, fh - 1.0, fh - 1.5)]
    last = [(x0 + fw - 1.0, y0 + 20.3, 1.0), (x0 + fw - 2.2, y0 + 20.3, 1.0), (x0 + 21.7, y0 + fh - 1.0, 1.0),
            (x0 + 21.7, y0 + fh - 2.4, 1.0)]
    # outside the map: invalid for the LM at this pose, but in front of the camera - their clamped boxes count
    outside = [(x0 - 3.0, y0 + 5.0, 1.0), (x0 + fw + 2.0, y0 + 5.0, 1.0), (x0 + 37.0, y0 - 0.25, 1.0),
               (x0 + 5.0, y0 + fh + 40.0, 1.0), (x0 - 5000.0, y0 - 9000.0, 1.0), (x0 + 1e9, y0 + 30.0, 1.0)]
    behind = [(x0 + 8.0, y0 + 8.0, -1.0), (x0 + 40.0, y0 + 9.0, 0.0), (x0 + 40.0, y0 + 40.0, 1e-4)]
    return {"seams": seams, "corners": corners, "last": last, "outside": outside, "behind": behind}


@pytest.mark.parametrize("fine_hw,window", [((64, 96), None), ((48, 64), None), ((64, 96), (32, 16, 240, 160)),
                                            ((48, 64), (176, 112, 240, 160))])
@pytest.mark.parametrize("margin", [0, 4, 12])
def test_marking_rule_on_the_host(fine_hw, window, margin):
    fh, fw = fine_hw
    full = window if window is not None else (0, 0, fw, fh)
    named = groups(fw, fh, full[0], full[1])
    named["all"] = [p for g in named.values() for p in g]
    for name, pts_list in named.items():
        xyz = np.ascontiguousarray(np.asarray(pts_list, np.float32))
        want = replica_fine(xyz, fh, fw, margin, window)
        got_fine, got_low = host_flags(record(xyz, margin, full, window is not None), fh, fw)
        assert np.array_equal(got_fine, want), (name, got_fine, want)
        assert np.array_equal(got_low, replica_low(want, fh, fw)), name
        if name == "behind":
            assert not want.any()
        elif name == "seams" and margin == 0:
            assert 0 < want.sum() < want.size  # (a seam point marks both sides of its seam, and not the whole map)
    # one point, margin 0: exactly the tiles of its 4 x 4 box - (16.0, 22.5) reaches back over the seam at x = 16 ...
    xyz = np.asarray([(full[0] + 16.0, full[1] + 22.5, 1.0)], np.float32)
    got, _ = host_flags(record(xyz, 0, full, window is not None), fh, fw)
    assert got[1, 0] == 1 and got[1, 1] == 1 and got.sum() == 2
    # ... (17.0, 22.5) does not (columns 16 .. 19), and a margin of 4 brings the left tile back (rows 17 .. 28: one row of tiles)
    xyz[0, 0] += 1.0
    got, _ = host_flags(record(xyz, 0, full, window is not None), fh, fw)
    assert got[1, 1] == 1 and got.sum() == 1
    got, _ = host_flags(record(xyz, 4, full, window is not None), fh, fw)
    assert got[1, 0] == 1 and got[1, 1] == 1 and got[0, 1] == 0 and got.sum() == 2


def test_other_tile_heights_and_bad_records():
    fh, fw = 64, 96
    xyz = np.ascontiguousarray(np.asarray(groups(fw, fh)["seams"], np.float32))
    for rows in ((8, 16), (32, 8), (24, 16)):
        want = replica_fine(xyz, fh, fw, 4, None, rows[0])
        got_fine, got_low = host_flags(record(xyz, 4, (0, 0, fw, fh), False), fh, fw, rows)
        assert np.array_equal(got_fine, want)
        assert np.array_equal(got_low, replica_low(want, fh, fw, *rows))
    pts = record(xyz, -1, (0, 0, fw, fh), False)
    fine, low = np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8)
    call = _lib.lib().pxt_unet_query_tiles_host
    assert call(C.byref(pts), fh, fw, 16, 16, fine.ctypes.data, low.ctypes.data) == PXT_E_ARG  # a negative margin
    assert call(None, fh, fw, 16, 16, fine.ctypes.data, low.ctypes.data) == PXT_E_ARG
    pts = record(xyz, 4, (0, 0, fw, fh), False)
    assert call(C.byref(pts), fh, fw + 1, 16, 16, fine.ctypes.data, low.ctypes.data) == PXT_E_ARG  # an odd map
