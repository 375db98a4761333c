"""Where the rays of the benchmark frame spend their occupancy walk: the share of dt-lattice points that lie in front of a
ray's first occupied point, behind its last one, and on rays that cross the render box without meeting an occupied cell.
CPU only, the repository's own oracle (oracle/ngp_oracle.py: same lattice, same cell test as the HIP march); about a minute.

    python scripts/first_hit_share.py [ROW_STRIDE] [--passes 3 | all] [--frame 5]

The scene is the benchmark's (make_tracking_assets(seed=1002, 640, 480), spp 8), the camera the ground-truth pose of one
frame; every ROW_STRIDE-th image row is walked, every lattice point t' = t + dt(t) from the ray's start to the box exit is
tested (early termination is left out: behind an opaque surface the march stops, so the "behind the last" share is an upper
bound).  With --passes all the 8 passes of a pixel are walked and the share of rays the first-hit kernel finishes itself
is reported as well: it drops a pixel's 8 passes together (ngp_first_hit_body in csrc/pxt_ngp.hip)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from oracle import frame_oracle as FO
from oracle import ngp_oracle as NO
from pixtrack_amd.synthetic import make_tracking_assets

F32 = np.float32


def walk(m, v, rows, spp_pass):
    """Per ray of the given rows that hits the box: (lattice points, index of the first occupied one or -1, of the last)."""
    o, d, _ = NO.generate_rays(v, rows)
    half = F32(m.aabb_scale / 2.0)
    lo = np.maximum(np.asarray(v.aabb_min, np.float32), F32(0.5) - half)
    hi = np.minimum(np.asarray(v.aabb_max, np.float32), F32(0.5) + half)
    tmin, tmax, _ = NO.ray_aabb(o, d, lo, hi)
    hit = tmax > np.maximum(tmin, F32(0.0))
    o, d, tmin, tmax = o[hit], d[hit], tmin[hit], tmax[hit]
    pix = (np.asarray(rows, np.int64)[:, None] * v.width + np.arange(v.width, dtype=np.int64)[None, :]).reshape(-1)[hit]
    dt_lo, dt_hi = NO.MIN_STEP, NO.max_step(m)
    t0 = (np.maximum(tmin, F32(0.0)) + F32(1e-6)).astype(np.float32)
    t = (t0 + NO.start_jitter(pix, spp_pass) * NO.calc_dt(t0, m.cone_angle, dt_lo, dt_hi)).astype(np.float32)
    n = t.shape[0]
    count = np.zeros(n, np.int64)
    first = np.full(n, -1, np.int64)
    last = np.full(n, -1, np.int64)
    live = t < tmax
    while live.any():
        k = np.nonzero(live)[0]
        tk = t[k]
        pos = (o[k] + tk[:, None] * d[k]).astype(np.float32)
        dt = NO.calc_dt(tk, m.cone_angle, dt_lo, dt_hi)
        occ = NO.occupied(m, pos, NO.mip_from_dt(dt, pos, m.cascades))
        ko = k[occ]
        first[ko] = np.where(first[ko] < 0, count[ko], first[ko])
        last[ko] = count[ko]
        count[k] += 1
        t[k] = (tk + dt).astype(np.float32)
        live[k] = t[k] < tmax[k]
    return count, first, last, pix


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("row_stride", nargs="?", type=int, default=6)
    ap.add_argument("--passes", default="3", help="one spp pass (0..7) or 'all'")
    ap.add_argument("--frame", type=int, default=5)
    a = ap.parse_args()
    W, H, SPP = 640, 480, 8
    assets = make_tracking_assets(seed=1002, width=W, height=H, n_frames=a.frame + 1)
    m = FO.ngp_model(assets["snapshot"])
    R, t = assets["gt_poses"][a.frame]
    v = FO.nerf_view(assets["snapshot"], assets["nerf2sfm"], assets["aabb"], R, t,
                     FO.colmap_camera_to_pix(assets["query_camera"]), 0, SPP)
    rows = np.arange(0, H, max(1, a.row_stride))
    passes = list(range(SPP)) if a.passes == "all" else [int(a.passes)]
    tot = dict(rays=0, points=0, empty_rays=0, before=0, after=0, on_empty=0)
    empty_by_pass = []
    for s in passes:
        count, first, last, pix = walk(m, v, rows, s)
        empty = first < 0
        tot["rays"] += count.size
        tot["points"] += int(count.sum())
        tot["empty_rays"] += int(empty.sum())
        tot["on_empty"] += int(count[empty].sum())
        tot["before"] += int(first[~empty].sum())
        tot["after"] += int((count[~empty] - 1 - last[~empty]).sum())
        empty_by_pass.append(empty)
    P = tot["points"]
    pc = lambda x, y: "%.1f %%" % (100.0 * x / max(y, 1))
    print("frame %d, every %d. row, pass(es) %s" % (a.frame, a.row_stride, a.passes))
    print("rays that hit the render box          %d" % tot["rays"])
    print("lattice points crossed                %d (%.1f per ray)" % (P, P / max(tot["rays"], 1)))
    print("rays without an occupied point        %d (%s)" % (tot["empty_rays"], pc(tot["empty_rays"], tot["rays"])))
    print("points on those rays                  %d (%s)" % (tot["on_empty"], pc(tot["on_empty"], P)))
    print("points before a ray's first occupied  %d (%s)" % (tot["before"], pc(tot["before"], P)))
    print("  before the first, or on an empty ray %s" % pc(tot["before"] + tot["on_empty"], P))
    print("points behind a ray's last occupied   %d (%s)" % (tot["after"], pc(tot["after"], P)))
    if len(passes) == SPP:
        all_empty = np.logical_and.reduce(empty_by_pass)  # (the passes of a pixel share the ray: same pixels in every pass)
        some = np.logical_or.reduce(empty_by_pass) & ~all_empty
        n_pix = all_empty.size
        print("pixels whose 8 passes are all empty   %d of %d (%s): finished by the first-hit kernel" %
              (int(all_empty.sum()), n_pix, pc(all_empty.sum(), n_pix)))
        print("pixels with some passes empty         %d (%s): their empty passes stay in the list" %
              (int(some.sum()), pc(some.sum(), n_pix)))
        kept_empty = tot["empty_rays"] - SPP * int(all_empty.sum())
        print("empty rays kept in the second list    %d (%s of the rays)" % (kept_empty, pc(kept_empty, tot["rays"])))


if __name__ == "__main__":
    main()
