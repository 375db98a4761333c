"""Measurements of the GPU pose-error evaluation -> profiles/r11_pose_errors.json.

  (gpu)  time of one pxt_pose_errors call (ADD + ADD-S) for (F, V) = (200, 2620), (1000, 8192), (64, 65536): HIP events
         around 20 calls with the host parked ahead of the stream, median of 7.  Per case: pair evaluations per second
         (F * V^2 per call) and the fraction of the fp32 VALU peak, counting 7 VALU operations per pair against
         MI355X's 157.3 TFLOPS vector fp32 peak taken as 78.65e12 VALU lane-operations per second (the TFLOPS figure
         counts a multiply-add as two).
  (host) wall time of the existing evaluation.adds_distance loop on the same inputs: the first case whole, the others
         on a subset of frames (--host_frames) scaled linearly to F.  Needs no GPU.
  (run)  one evaluate_poses of a 200-frame r9 run at 640 x 480 (synthetic assets, their SfM points as vertices): time,
         auc_add / auc_adds.

    python scripts/bench_pose_errors.py [--parts gpu,host,run] [--host_frames 200,2,1] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import evaluation as E  # noqa: E402

CASES = ((200, 2620), (1000, 8192), (64, 65536))
VALU_OPS_PER_PAIR = 7
PEAK_VALU_OPS = 157.3e12 / 2  # lane-operations per second: the vector fp32 peak counts an FMA as 2 FLOP


def make_case(F, V, seed=11):
    """A Gaussian cloud of diameter ~0.2 away from the origin and F (estimate, ground truth) pose pairs a few degrees and
    millimetres apart."""
    rng = np.random.default_rng(seed + V)
    v = rng.normal(size=(V, 3)) * 0.03 + np.array([0.3, -0.1, 0.5])

    def rot(w):
        th = np.linalg.norm(w)
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)

    T_gt, T_est = np.tile(np.eye(4), (F, 1, 1)), np.tile(np.eye(4), (F, 1, 1))
    for k in range(F):
        T_gt[k, :3, :3], T_gt[k, :3, 3] = rot(rng.normal(size=3)), np.r_[rng.uniform(-0.5, 0.5, 2), rng.uniform(1, 3)]
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = rot(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.005
        T_est[k] = T_gt[k] @ D
    return v, T_est, T_gt


def part_gpu():
    import torch

    from pixtrack_amd import _lib

    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    rows = []
    for F, V in CASES:
        v, T_est, T_gt = make_case(F, V)
        c = v.mean(axis=0)
        verts = torch.from_numpy((v - c).astype(np.float32)).to(dev)
        poses = torch.from_numpy(E.relative_poses(T_est, T_gt, c)).to(dev)
        rec = torch.zeros(F, 8, device=dev)
        ws = torch.empty(int(L.pxt_pose_errors_workspace_bytes(F, V)), dtype=torch.uint8, device=dev)

        def launch(adds=1):
            rc = L.pxt_pose_errors(verts.data_ptr(), V, poses.data_ptr(), F, adds, rec.data_ptr(), ws.data_ptr(), stream)
            assert rc == 0, rc

        per, ms, ms_add = 20, [], []
        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        for which, out in ((1, ms), (0, ms_add)):
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
                e0.record()
                for _ in range(per):
                    launch(which)
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1) / per)
        t = float(np.median(ms)) * 1e-3
        pairs = F * V * V / t
        rows.append({"F": F, "V": V, "ms_per_call_median": t * 1e3, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                     "pairs_per_s": pairs, "valu_ops_per_pair": VALU_OPS_PER_PAIR, "peak_valu_ops_per_s": PEAK_VALU_OPS,
                     "fraction_of_fp32_valu_peak": pairs * VALU_OPS_PER_PAIR / PEAK_VALU_OPS,
                     "add_only_ms_per_call_median": float(np.median(ms_add)),
                     "adds_mean_of_frame_0": float(rec[0, 2])})
        print(rows[-1], flush=True)
    return {"peak": "157.3 TFLOPS vector fp32 (MI355X_MICROARCH) = 78.65e12 VALU lane-operations/s", "cases": rows}


def part_host(host_frames):
    rows = []
    for (F, V), n in zip(CASES, host_frames):
        n = min(n, F)
        v, T_est, T_gt = make_case(F, V)
        t0 = time.perf_counter()
        vals = [E.adds_distance(T_est[k], T_gt[k], v) for k in range(n)]
        dt = time.perf_counter() - t0
        rows.append({"F": F, "V": V, "frames_run": n, "seconds_run": dt, "seconds_for_F_frames": dt * F / n,
                     "scaled_linearly": n != F, "adds_of_frame_0": float(vals[0])})
        print(rows[-1], flush=True)
    return {"what": "evaluation.adds_distance in a Python loop over frames (numpy float64, one process)",
            "cpus": os.cpu_count(), "cases": rows}


def part_run(n_frames=200):
    import torch

    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    dev = torch.device("cuda:0")
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n_frames)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, tr.testbed)
    names = [f"{i:06d}.png" for i in range(n_frames)]
    for name, frame in zip(names, frames):
        tr.run_single_frame((name, frame))
    torch.cuda.synchronize(dev)
    for name, (Rg, tg) in zip(names, assets["gt_poses"]):
        tr.pose_history[name]["gt_pose"] = Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg))
    pts = assets["model3d"].points3D
    v = np.stack([pts[i].xyz for i in sorted(pts)])
    diameter = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))  # (the bounding box's diagonal)
    E.evaluate_poses(tr.pose_history, v, dev, max_distance=0.1 * diameter)  # warm-up: library load, allocator
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = E.evaluate_poses(tr.pose_history, v, dev, max_distance=0.1 * diameter)
    dt = time.perf_counter() - t0
    out = {k: res[k] for k in res if k != "frames"}
    out.update({"frames": n_frames, "V": int(len(v)), "box_diagonal": diameter, "evaluate_poses_seconds": dt,
                "max_distance_rule": "0.1 x bounding-box diagonal"})
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="gpu,host,run")
    ap.add_argument("--host_frames", default="200,2,1")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11_pose_errors.json"))
    args = ap.parse_args()
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    host_frames = [int(x) for x in args.host_frames.split(",")]
    for part, fn in (("gpu", part_gpu), ("host", lambda: part_host(host_frames)), ("run", part_run)):
        if part in args.parts.split(","):
            result[part] = fn()
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
