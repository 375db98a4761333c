"""Measurements of the opt-in reference points from the render's depth -> profiles/r09_reference_points.json.

  (a) device time of one pxt_points_from_depth call (its three launches) on a real Depth render at 640x480 and 160x120:
      HIP events around batches of calls, host parked ahead of the stream, median of 7; beside it the render with and
      without its float Depth output (what the option adds to the render itself).
  (b) tracked frames/s of the r9 tracker at 640x480 with the option off and on, same process, same frames, alternating
      three times.
  (c) the two documented tracks (bottle, roncelli_blankk of objects8, 65 frames) with the option on: rotation error and
      number of reference points per frame, beside the same run with the option off.
  (d) the six-frame 160x120 sequence of tests/test_reference_points_gpu.py in both modes (the "sfm" figures are the
      test's yardstick).

    python scripts/bench_reference_points.py [--parts abcd] [--frames 200]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import parallel  # noqa: E402
from pixtrack_amd.geometry import Camera, Pose  # noqa: E402
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9  # noqa: E402
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames  # noqa: E402


def _tracker(dev, assets, mode):
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, reference_points=mode)


def _device_us(fn, per=50, reps=7, warm=20):
    """Median / min / max device microseconds per call of ``fn`` (enqueue only), host parked ahead of the stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(4_000_000)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per)
    return {"us_median": float(np.median(out)), "us_min": float(min(out)), "us_max": float(max(out))}


def _rot_err(R, R_gt):
    return float(np.arccos(np.clip((np.trace(np.asarray(R, np.float64) @ np.asarray(R_gt, np.float64).T) - 1) / 2, -1, 1)))


# ------------------------------------------------------------------------------------------------ (a)
def part_a(dev):
    rows = []
    for w, h in ((640, 480), (160, 120)):
        assets = make_tracking_assets(seed=1002, width=w, height=h, n_frames=2)
        tr = _tracker(dev, assets, "render")
        tr.camera = Camera.from_colmap(assets["query_camera"])
        pose = Pose.from_Rt(*assets["gt_poses"][0])
        tr._mask_and_reference(pose, from_slot=False)
        depth, view = tr._own.depth, tr._depth_view(pose)
        refiner = tr.localizer.refiner
        row = {"width": w, "height": h, "points_from_depth": _device_us(lambda: refiner.points_from_render(depth, view), per=20)}
        torch.cuda.synchronize()
        row["record"] = refiner.last_points_record.tolist()  # {accepted pixels, stride, points, candidates}
        row["bytes_read_once"] = 16 * w * h
        tb, spp = tr.testbed, int(tr.spp)
        tb.set_nerf_camera_matrix(np.asarray(tr._nerf_pose(pose))[:3, :])
        tb.fov = tr._frame_views()[0][2]
        row["render_u8_only"] = _device_us(lambda: tb.render_frame_device(w, h, spp, mode=2), per=10, warm=5)
        row["render_with_float_depth"] = _device_us(lambda: tb.render_frame_device(w, h, spp, mode=2, want_float="depth"),
                                                    per=10, warm=5)
        rows.append(row)
        print(row, flush=True)
    return rows


# ------------------------------------------------------------------------------------------------ (b)
def _run(dev, assets, frames, names, mode, warm=10):
    tr = _tracker(dev, assets, mode)
    for i in range(warm):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(warm, len(names)):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    tracked = sum(bool(tr.pose_history[n]["tracked"]) for n in names[warm:])
    return tracked / dt, tracked, tr.renders_ahead_used


def part_b(dev, n_frames):
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n_frames + 10)
    probe = _tracker(dev, assets, "sfm")
    frames = render_query_frames(assets, probe.testbed)
    names = [f"{i:06d}.png" for i in range(n_frames + 10)]
    del probe
    runs = {"off": [], "on": []}
    for _ in range(3):
        for key, mode in (("off", "sfm"), ("on", "render")):
            fps, tracked, ahead = _run(dev, assets, frames, names, mode)
            runs[key].append(fps)
            print("r9", key, fps, tracked, ahead, flush=True)
    return {"r9_640x480": {k: {"fps": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))}
                           for k, v in runs.items()}, "frames": n_frames}


# ------------------------------------------------------------------------------------------------ (c)
def part_c(dev, n=65):
    objs = parallel.load_object_configs()
    out = {}
    for u in (0, 6):
        assets = make_tracking_assets(seed=1002 + u, width=640, height=480, n_frames=n, aabb=objs[u]["aabb"])
        frames = None
        per_mode = {}
        for mode in ("sfm", "render"):
            tr = _tracker(dev, assets, mode)
            if frames is None:
                frames = render_query_frames(assets, tr.testbed)
            rows = []
            for i in range(n):
                name = f"{i:06d}.png"
                tr.run_single_frame((name, frames[i]))
                ret = tr.pose_history[name]
                rows.append({"frame": i, "tracked": bool(ret["tracked"]),
                             "rot_err_rad": _rot_err(tr.pose.R.double().numpy(), assets["gt_poses"][i][0]),
                             "reference_id": int(tr.reference_ids[0]),
                             "n_reference_points": ret.get("n_reference_points"),
                             "reference_point_stride": ret.get("reference_point_stride")})
            per_mode[mode] = rows
        out[objs[u]["name"]] = per_mode
        lo, hi = (10, 20) if u == 0 else (35, 46)
        out[objs[u]["name"] + "_summary"] = {
            "window": [lo, hi],
            **{f"max_rot_err_inside_{m}": float(max(r["rot_err_rad"] for r in per_mode[m][lo:hi + 1])) for m in per_mode},
            **{f"max_rot_err_all_{m}": float(max(r["rot_err_rad"] for r in per_mode[m])) for m in per_mode},
            **{f"tracked_{m}": int(sum(r["tracked"] for r in per_mode[m])) for m in per_mode}}
        print(objs[u]["name"], out[objs[u]["name"] + "_summary"], flush=True)
    return out


# ------------------------------------------------------------------------------------------------ (d)
def part_d(dev, n=6):
    assets = make_tracking_assets(width=160, height=120, n_frames=n)
    frames, out = None, {}
    for mode in ("sfm", "render"):
        tr = _tracker(dev, assets, mode)
        if frames is None:
            frames = render_query_frames(assets, tr.testbed)
        rot, trans, pts = [], [], []
        for i in range(n):
            name = f"{i:06d}.png"
            tr.run_single_frame((name, frames[i]))
            ret = tr.pose_history[name]
            R, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
            rot.append(_rot_err(R, assets["gt_poses"][i][0]))
            trans.append(float(np.linalg.norm(np.asarray(t, np.float64) - assets["gt_poses"][i][1])))
            pts.append(ret.get("n_reference_points"))
        out[mode] = {"rot_err_rad": rot, "trans_err": trans, "max_rot_err_rad": max(rot), "max_trans_err": max(trans),
                     "tracked": [bool(tr.pose_history[f"{i:06d}.png"]["tracked"]) for i in range(n)],
                     "n_reference_points": pts}
        print(mode, out[mode], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09_reference_points.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    for part, fn in (("a", lambda: part_a(dev)), ("b", lambda: part_b(dev, args.frames)), ("c", lambda: part_c(dev)),
                     ("d", lambda: part_d(dev))):
        if part in args.parts:
            result[part] = fn()
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
