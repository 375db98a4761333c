"""Query tiles: how far the LM moves the points, the margin that follows, the tile share, and the guard trips.

    python scripts/query_tile_share.py [frames] [following]

Tracks bench.py's default sequence (seed 1002, 640 x 480) for `frames` (300) frames with the option OFF.  For every pose
the fine level of a steady frame's LM launch evaluated or produced - the level's start pose and the logged pose after each
of its steps - it computes on the host (float64) the largest displacement, in fine pixels, of any reference point from its
projection under the launch's initial pose.  The margin is 2 x that maximum, rounded up to a multiple of 4, at least 8.
With that margin it prints the share of the last two decoder layers' tiles the query pass computes
(pxt_unet_query_tiles_host: the device kernel's own functions, 16-row tiles), and then tracks `frames` + `following` (200)
frames with the option ON and counts the guard trips in both parts."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9  # noqa: E402
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames  # noqa: E402


def project(T12, cam10, xyz):
    """(u, v) [N, 2] and the in-front mask of points under pose T12 and a camera record (pinhole + k1, k2), float64."""
    T = np.asarray(T12, np.float64)
    p = xyz @ T[:9].reshape(3, 3).T + T[9:]
    front = p[:, 2] > 1e-3
    z = np.where(front, p[:, 2], 1.0)
    xn, yn = p[:, 0] / z, p[:, 1] / z
    r2 = xn * xn + yn * yn
    rad = 1.0 + cam10[6] * r2 + cam10[7] * r2 * r2
    return np.stack([xn * rad * cam10[2] + cam10[4], yn * rad * cam10[3] + cam10[5]], 1), front


def track(assets, dev, n, on, margin, spy=None):
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    tr.query_tiles = on
    tr.query_tile_margin = margin
    frames = render_query_frames(assets, tr.testbed)[:n]
    refiner = tr.localizer.refiner
    if spy is not None:
        inner = refiner.lm_finish
        refiner.lm_finish = lambda prob, res: (spy(tr, prob, res), inner(prob, res))[1]
    trips = []
    for i, f in enumerate(frames):
        before = refiner.query_tile_fallbacks
        tr.run_single_frame((f"{i:06d}.png", f))
        trips.append(refiner.query_tile_fallbacks - before)
    return tr, trips


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    more = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dev = torch.device("cuda:0")
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n + more)
    launches = []  # (initial pose, fine camera, points, fine map size, largest displacement)

    def spy(tr, prob, res):
        if 0 not in prob["order"] or tr.localizer.refiner.query_mask is None or res.failed:
            return  # (steady frames only: the option's frames)
        kf = prob["order"].index(0)
        cam10 = np.asarray(prob["packs"][kf].camera.as10().tolist(), np.float64)
        ref = prob["ref"]
        xyz = ref.p3d.detach().cpu().numpy().astype(np.float64)[ref.valid.detach().cpu().numpy() != 0]
        T0 = prob["T_init"].as12().detach().cpu().reshape(-1).numpy()
        log = res.log.numpy()
        start = T0
        for k in range(kf):  # the fine level starts where the levels before it ended
            if res.iters[k] > 0:
                start = log[k, res.iters[k] - 1, 8:20]
        poses = [start] + [log[kf, i, 8:20] for i in range(res.iters[kf])]
        uv0, front0 = project(T0, cam10, xyz)
        worst = 0.0
        for T in poses:
            uv, front = project(T, cam10, xyz)
            both = front & front0
            worst = max(worst, float(np.abs(uv - uv0)[both].max()))  # (the box grows by the margin per axis)
        fmap = prob["packs"][kf].fmap
        launches.append((T0, cam10, ref.p3d.detach().cpu().numpy().astype(np.float32), (int(fmap.shape[0]), int(fmap.shape[1])),
                         worst, len(poses)))

    track(assets, dev, n, False, 8, spy)
    worst = max(l[4] for l in launches)
    margin = max(8, int(math.ceil(2.0 * worst / 4.0)) * 4)
    print(f"{len(launches)} steady launches of {n} frames, {sum(l[5] for l in launches)} fine-level poses; largest displacement "
          f"from the initial pose's projection {worst:.3f} fine pixels (mean of the launches' maxima "
          f"{np.mean([l[4] for l in launches]):.3f}) -> margin {margin}")
    L = _lib.lib()
    shares = []
    for T0, cam10, xyz, (fh, fw), _w, _n in launches:
        xyz = np.ascontiguousarray(xyz)
        q = _lib.UnetQueryPoints()
        q.points.p3d, q.points.n_points = xyz.ctypes.data, len(xyz)
        q.points.T[:] = [float(x) for x in T0]
        q.points.cam[:] = [float(x) for x in cam10]
        q.points.ndist, q.points.pad = (0 if not (cam10[6] or cam10[7]) else 2), 4  # (the rule does not read the pad)
        q.margin = margin
        fine = np.zeros((-(-fh // 16), -(-fw // 16)), np.uint8)
        low = np.zeros((-(-(fh // 2) // 16), -(-(fw // 2) // 16)), np.uint8)
        _lib.check(L.pxt_unet_query_tiles_host(C.byref(q), fh, fw, 16, 16, fine.ctypes.data, low.ctypes.data),
                   "pxt_unet_query_tiles_host")
        shares.append((fine.mean(), low.mean(), fine.size, low.size))
    s = np.asarray(shares)
    print(f"tiles computed with margin {margin}: last layer {100 * s[:, 0].mean():.1f} % of {int(s[0, 2])} (min "
          f"{100 * s[:, 0].min():.1f}, max {100 * s[:, 0].max():.1f}), layer before {100 * s[:, 1].mean():.1f} % of {int(s[0, 3])} "
          f"(min {100 * s[:, 1].min():.1f}, max {100 * s[:, 1].max():.1f})")
    tr, trips = track(assets, dev, n + more, True, margin)
    r = tr.localizer.refiner
    print(f"option on, margin {margin}: {r.query_tile_frames} guarded launches in {n + more} frames; guard trips in the first {n} "
          f"frames: {sum(trips[:n])}, in the {more} that follow: {sum(trips[n:])}; tracked {sum(1 for v in tr.pose_history.values() if v['tracked'])}")


if __name__ == "__main__":
    main()
