"""Measurements of the mesh-free pose evaluation -> profiles/r12_depth_agreement.json.

  (gpu)  time of one pxt_depth_agreement call (both launches, 10 taus + the finite-pixel slot) for 640 x 480 x {1, 32, 200}
         pairs and 1024 x 768 x 32 pairs: HIP events around 20 calls with the host parked ahead of the stream, median of
         7.  Per case: bytes read per second (32 B per pixel and pair; the partials and records are left out: < 0.3 %)
         against MI355X's HBM figures of MI355X_MICROARCH.md - 8.0 TB/s peak, 6.29 TB/s measured with a float4 copy.
         The images are synthetic Depth-like frames (a disc of alpha 1 with smooth depth); the kernel's time does not
         depend on their content.
  (run)  wall time of one evaluate_poses_rendered of a 200-frame r9 run at 640 x 480 (synthetic assets), the 400 Depth
         renders included, and its summary.

    python scripts/bench_depth_agreement.py [--parts gpu,run] [--frames 200] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import render_evaluation as RE  # noqa: E402

CASES = ((640, 480, 1), (640, 480, 32), (640, 480, 200), (1024, 768, 32))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
BYTES_PER_PIXEL = 32


def part_gpu():
    import torch

    from pixtrack_amd import _lib

    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    tq = [0.01 * (k + 1) for k in range(10)] + [float("inf")]
    tqs = (ctypes.c_float * len(tq))(*tq)
    rows = []
    for W, H, P in CASES:
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        imgs = []
        for shift in (-0.05, 0.05):
            disc = ((xx - W * (0.5 + shift)) ** 2 + (yy - H * 0.5) ** 2 <= (0.3 * H) ** 2).float()
            one = torch.zeros(H, W, 4, device=dev)
            one[..., 3] = disc
            one[..., 0] = disc * (0.3 + 0.1 * torch.sin(xx * 0.05) * torch.cos(yy * 0.04))
            imgs.append(one.expand(P, H, W, 4).contiguous())
        est, gt = imgs
        rec = torch.zeros(P, RE.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.pxt_depth_agreement_workspace_bytes(P, W, H)), dtype=torch.uint8, device=dev)

        def launch():
            rc = L.pxt_depth_agreement(est.data_ptr(), gt.data_ptr(), P, W, H, 0.5, tqs, len(tq), rec.data_ptr(),
                                       ws.data_ptr(), stream)
            assert rc == 0, rc

        per, ms = 20, []
        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
            e0.record()
            for _ in range(per):
                launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        t = float(np.median(ms)) * 1e-3
        nbytes = P * W * H * BYTES_PER_PIXEL
        r = rec.cpu().numpy().view(np.uint32)
        rows.append({"width": W, "height": H, "pairs": P, "bytes_read_per_call": nbytes, "ms_per_call_median": t * 1e3,
                     "ms_min": float(min(ms)), "ms_max": float(max(ms)), "bytes_per_s": nbytes / t,
                     "fraction_of_hbm_peak_8.0TBs": nbytes / t / HBM_PEAK,
                     "fraction_of_measured_copy_6.29TBs": nbytes / t / HBM_COPY,
                     "input_MB": 2 * P * W * H * 16 / 1e6, "fits_infinity_cache_256MiB": 2 * P * W * H * 16 <= (256 << 20),
                     "n_both_of_pair_0": int(r[0, 2]), "n_union_of_pair_0": int(r[0, 3])})
        print(rows[-1], flush=True)
        del est, gt, imgs
    return {"hbm": "8.0 TB/s peak, 6.29 TB/s measured float4 copy (MI355X_MICROARCH)", "bytes_per_pixel_and_pair": 32,
            "calls_per_window": 20, "windows": 7, "cases": rows}


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
    diameter = RE.bounding_box_diagonal(assets["model3d"])
    warm = {n: tr.pose_history[n] for n in names[:2]}
    RE.evaluate_poses_rendered(warm, tr.testbed, tr.nerf2sfm, diameter)  # warm-up: allocator, first launches
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = RE.evaluate_poses_rendered(tr.pose_history, tr.testbed, tr.nerf2sfm, diameter)
    dt = time.perf_counter() - t0
    out = {k: res[k] for k in res if k != "frames"}
    out.update({"frames": n_frames, "width": 640, "height": 480, "spp": 8, "depth_renders": 2 * res["n_evaluated"],
                "evaluate_poses_rendered_seconds": dt, "diameter_rule": "diagonal of the SfM points' bounding box"})
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="gpu,run")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_depth_agreement.json"))
    args = ap.parse_args()
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    for part, fn in (("gpu", part_gpu), ("run", lambda: part_run(args.frames))):
        if part in args.parts.split(","):
            result[part] = fn()
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
