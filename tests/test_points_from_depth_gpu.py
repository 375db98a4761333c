"""pxt_points_from_depth (torch.ops.pixtrack.points_from_depth) against a numpy / float64 restatement of its selection and
back-projection, on hand-made depth planes (no NeRF): the record and slot_valid exactly, the point order exactly, the
points within 1e-5 x the largest coordinate (the chain is about ten fp32 operations: 1e-6 is expected, the bar is 10 x)."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd.ops import ops

pytestmark = pytest.mark.gpu

DEPTH_SCALE = np.float32(1.0 / 0.33)
FOCAL = np.float32(80.4)
MIN_ALPHA = np.float32(0.5)
# [M | b]: a rotation (about (1, 2, 3)) scaled by 3.03 and a translation, as float32 (what the kernel receives)
_axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
_K = np.array([[0, -_axis[2], _axis[1]], [_axis[2], 0, -_axis[0]], [-_axis[1], _axis[0], 0]])
_R = np.eye(3) + np.sin(0.7) * _K + (1 - np.cos(0.7)) * (_K @ _K)
XFORM = np.concatenate([3.03 * _R, np.array([[0.4], [-1.3], [2.2]])], axis=1).astype(np.float32)


def restate(depth, n_max, erode, min_alpha=MIN_ALPHA, xform=XFORM, focal=FOCAL, depth_scale=DEPTH_SCALE):
    """-> (p3d float64 [n_max, 3], slot_valid uint8 [n_max], record [A, s, n_points, n_candidates])."""
    H, W, _ = depth.shape
    d0, al = depth[..., 0], depth[..., 3]
    base = (al >= np.float32(min_alpha)) & (d0 > np.float32(0))
    acc = np.zeros_like(base)
    e = erode
    inner = np.ones((H - 2 * e, W - 2 * e), bool) if H > 2 * e and W > 2 * e else None
    if inner is not None:
        for dy in range(-e, e + 1):
            for dx in range(-e, e + 1):
                inner &= base[e + dy:H - e + dy, e + dx:W - e + dx]
        acc[e:H - e, e:W - e] = inner
    A = int(acc.sum())
    s = 1
    while s * s * n_max < A:
        s += 1
    ys, xs = np.nonzero(acc)  # row-major
    keep = (xs % s == s // 2) & (ys % s == s // 2)
    xs, ys = xs[keep], ys[keep]
    n_cand = int(xs.size)
    xs, ys = xs[:n_max], ys[:n_max]
    n = int(xs.size)
    M, b = xform.astype(np.float64)[:, :3], xform.astype(np.float64)[:, 3]
    z = d0[ys, xs].astype(np.float64) / (al[ys, xs].astype(np.float64) * float(depth_scale))
    dirs = np.stack([(xs + 0.5 - W / 2.0) / float(focal), (ys + 0.5 - H / 2.0) / float(focal), np.ones(n)], axis=1)
    p3d = np.tile(b, (n_max, 1))
    p3d[:n] = b + z[:, None] * (dirs @ M.T)
    valid = np.zeros(n_max, np.uint8)
    valid[:n] = 1
    return p3d, valid, [A, s, n, n_cand]


def run(device, depth, n_max, erode, min_alpha=MIN_ALPHA, pinned_record=False):
    H, W, _ = depth.shape
    d = torch.from_numpy(depth).to(device)
    p3d = torch.full((n_max, 3), float("nan"), device=device)  # every slot must be written
    valid = torch.full((n_max,), 7, dtype=torch.uint8, device=device)
    record = torch.full((4,), -1, dtype=torch.int32)
    record = record.pin_memory() if pinned_record else record.to(device)
    ws = torch.empty(int(_lib.lib().pxt_points_from_depth_workspace_bytes(W, H)), dtype=torch.uint8, device=device)
    ops.points_from_depth(d, XFORM.reshape(-1).tolist(), float(FOCAL), float(DEPTH_SCALE), float(min_alpha), erode, n_max,
                          p3d, valid, record, ws)
    torch.cuda.synchronize()
    return p3d.cpu().numpy(), valid.cpu().numpy(), record.cpu().numpy().tolist()


def plane(W, H, inside, rng=None):
    """A Depth render's float image: alpha in 0.8 .. 1 and a tilted surface inside, zeros outside."""
    ys, xs = np.mgrid[0:H, 0:W]
    alpha = (0.8 + 0.2 * ((xs * 7 + ys * 13) % 11) / 10.0).astype(np.float32)
    z = (2.0 + 0.004 * xs - 0.003 * ys).astype(np.float32)
    depth = np.zeros((H, W, 4), np.float32)
    depth[..., 3] = np.where(inside, alpha, 0)
    depth[..., 0] = depth[..., 1] = depth[..., 2] = np.where(inside, alpha * z * DEPTH_SCALE, 0)
    return depth


def disc(W, H, r):
    ys, xs = np.mgrid[0:H, 0:W]
    return plane(W, H, (xs - W // 2) ** 2 + (ys - H // 2) ** 2 <= r * r)


def check(device, depth, n_max, erode, min_alpha=MIN_ALPHA, pinned_record=False):
    want_p, want_v, want_rec = restate(depth, n_max, erode, min_alpha)
    got_p, got_v, got_rec = run(device, depth, n_max, erode, min_alpha, pinned_record)
    print("record", got_rec, "expected", want_rec)
    assert got_rec == want_rec
    assert np.array_equal(got_v, want_v)
    tol = 1e-5 * np.abs(want_p).max()
    err = np.abs(got_p.astype(np.float64) - want_p).max()
    print("max |p3d - restated| =", err, "bar", tol)
    # (the order is part of it: a point in another slot is off by at least a lattice step of the surface)
    assert err <= tol
    n = want_rec[2]
    assert np.array_equal(got_p[n:], np.tile(XFORM[:, 3], (n_max - n, 1)))  # unused slots: exactly b
    return want_rec


def test_disc(device):
    rec = check(device, disc(67, 45, 15), 4096, 1)
    assert rec[1] == 1 and rec[2] == rec[0] == rec[3] > 0


def test_disc_small_n_max(device):
    rec = check(device, disc(67, 45, 15), 64, 1, pinned_record=True)
    assert rec[1] > 1 and rec[2] <= 64


def test_full_frame(device):
    rec = check(device, plane(67, 45, np.ones((45, 67), bool)), 50, 1)
    assert rec == [65 * 43, 8, 40, 40]


def test_truncation(device):
    ys, _ = np.mgrid[0:32, 0:64]
    rec = check(device, plane(64, 32, ys % 2 == 1), 300, 0)
    assert rec == [1024, 2, 300, 512]


@pytest.mark.parametrize("erode", [0, 1])
def test_alpha_threshold(device, erode):
    depth = plane(67, 45, np.ones((45, 67), bool))
    below = np.nextafter(MIN_ALPHA, np.float32(0))
    assert below < MIN_ALPHA
    depth[..., 3] = MIN_ALPHA  # exactly the threshold: passes
    depth[::3, 1::4, 3] = below  # one ulp below, next to pixels at the threshold: fails
    depth[5:9, 20:30, 3] = 1.0
    depth[6, 22:25, 0] = 0.0  # alpha 1, depth0 == 0: fails
    depth[40, 3, 0] = -1.0
    want = restate(depth, 4096, erode)[2]
    assert 0 < want[0] < 67 * 45
    check(device, depth, 4096, erode)


def test_empty_plane(device):
    rec = check(device, plane(67, 45, np.zeros((45, 67), bool)), 128, 1)
    assert rec == [0, 1, 0, 0]


def test_single_pixel(device):
    inside = np.zeros((45, 67), bool)
    inside[31, 50] = True
    rec = check(device, plane(67, 45, inside), 16, 0)
    assert rec == [1, 1, 1, 1]
    assert check(device, plane(67, 45, inside), 16, 1) == [0, 1, 0, 0]  # its 3 x 3 square fails


def test_many_workgroups(device):
    rec = check(device, disc(640, 480, 150), 2048, 1)
    assert rec[1] > 1 and rec[3] <= 2048 + 2048 // 2


def test_repeatability(device):
    depth = disc(67, 45, 15)
    first = run(device, depth, 256, 1)
    for _ in range(19):
        again = run(device, depth, 256, 1)
        assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32))
        assert np.array_equal(first[1], again[1]) and first[2] == again[2]


def test_arguments_are_checked(device):
    d = torch.zeros(8, 8, 4, device=device)
    ws = torch.empty(int(_lib.lib().pxt_points_from_depth_workspace_bytes(8, 8)), dtype=torch.uint8, device=device)
    p3d, valid = torch.zeros(4, 3, device=device), torch.zeros(4, dtype=torch.uint8, device=device)
    rec = torch.zeros(4, dtype=torch.int32, device=device)
    xf = XFORM.reshape(-1).tolist()
    with pytest.raises(_lib.PxtError):
        ops.points_from_depth(d, xf, 10.0, 3.0, 0.5, 3, 4, p3d, valid, rec, ws)  # erode out of range
    with pytest.raises(_lib.PxtError):
        ops.points_from_depth(d, xf, 10.0, 3.0, 0.5, 1, 4, p3d, valid, rec, ws[:8])  # workspace too small
    with pytest.raises(_lib.PxtError):
        ops.points_from_depth(d, xf, 10.0, 3.0, 0.5, 1, 4, p3d, valid, torch.zeros(4, dtype=torch.int32), ws)  # pageable record
