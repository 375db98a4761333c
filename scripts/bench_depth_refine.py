"""Measurements of the opt-in sensor-depth refinement -> profiles/depth_refine.json.

  (a) device time per pxt_depth_refine call: N = 600 and 2048 points, 10 iterations with the stop thresholds at 0 (so
      all ten run), a 640 x 480 sensor image, 1 and 8 problems per launch: HIP events around batches of 50 launches
      with the host parked ahead of the stream, median of 7.  The scene is the analytic one of
      pixtrack_amd/depth_scene.py (two ellipsoids before a plane) at 640 x 480.
  (b) tracked frames/s of the r9 tracker (640 x 480, reference_points="render") with the option on against off, same
      process, same scene, alternating; "on" includes the loss of render-ahead.  The sensor frames are Depth renders at
      the ground-truth poses, quantised to uint16.  Also the mean translation error of both runs.

    python scripts/bench_depth_refine.py [--parts ab] [--frames 100] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import depth_refinement as DR  # noqa: E402


def _time_launches(dev, launch, per=50, reps=7):
    for _ in range(20):
        launch()
    torch.cuda.synchronize(dev)
    us, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
        e0.record()
        t0 = time.perf_counter()
        for _ in range(per):
            launch()
        host.append((time.perf_counter() - t0) * 1e6 / per)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / per)
    return {"us_per_launch_median": float(np.median(us)), "us_min": float(min(us)), "us_max": float(max(us)),
            "host_us_per_call": float(np.median(host))}


# ------------------------------------------------------------------------------------------------ (a)
def part_a(dev):
    from pixtrack_amd.depth_scene import SCALE, make_scene, pose12, rodrigues

    sc = make_scene(640, 480, n_per=40000, seed=5)
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    sensor = torch.from_numpy(sc["sensor"].view(np.int16)).to(dev)
    T0 = pose12(rodrigues(np.radians(0.5) * np.array([0.6, 0.0, 0.8])) @ sc["R"], sc["t"] + np.array([0.001, 0.0, 0.002]))
    pose = torch.zeros(16, device=dev)
    pose[:12] = torch.from_numpy(T0.astype(np.float32)).to(dev)
    conf = _lib.DepthConf()
    conf.num_iters, conf.pad, conf.loss, conf.loss_scale, conf.min_valid = 10, 2, 1, 0.004, 10
    conf.lambda_[:] = [1e-2] * 6
    conf.max_residual, conf.max_edge = 0.02, 0.01
    conf.grad_stop = conf.dt_stop = conf.dR_stop = 0.0
    rows = []
    for N in (600, 2048):
        assert len(sc["points"]) >= N, len(sc["points"])
        p3d = torch.from_numpy(sc["points"][:N].astype(np.float32)).to(dev).contiguous()
        for K in (1, 8):
            recs = [torch.zeros(32, device=dev) for _ in range(K)]
            probs = (_lib.DepthProblem * K)()
            for k in range(K):
                q = probs[k]
                q.p3d, q.point_mask, q.n_points = p3d.data_ptr(), None, N
                q.sensor, q.width, q.height, q.sensor_scale = sensor.data_ptr(), 640, 480, float(np.float32(SCALE))
                q.cam[:] = [float(x) for x in sc["cam10"]]
                q.ndist, q.pose, q.pose_is_lm_record = 0, pose.data_ptr(), 0
                q.out, q.log, q.codes = recs[k].data_ptr(), None, None
            ws = torch.zeros(int(L.pxt_depth_refine_workspace_bytes(K)), dtype=torch.uint8, device=dev)

            def launch():
                rc = L.pxt_depth_refine(probs, K, C.byref(conf), ws.data_ptr(), stream)
                assert rc == 0, rc

            row = {"N": N, "problems": K, "iterations": 10, "sensor": "640x480", **_time_launches(dev, launch)}
            torch.cuda.synchronize(dev)
            r = recs[-1].cpu().numpy()
            row.update(status=float(r[31]), iterations_run=int(r[13]), n_valid=int(r[17]), cost_before=float(r[14]),
                       cost_after=float(r[16]))
            row["us_per_iteration"] = row["us_per_launch_median"] / 11.0  # ten updates and the final evaluation
            rows.append(row)
            print(row, flush=True)
    return rows


# ------------------------------------------------------------------------------------------------ (b)
def _sensor_frames(dev, assets, tr, n):
    from pixtrack_amd import render_evaluation as RE
    from pixtrack_amd import sensor_evaluation as SE
    from pixtrack_amd.geometry import Camera

    camera = Camera.from_colmap(assets["query_camera"])
    W, H = (int(x) for x in camera.size)
    zs = RE.z_scale(tr.testbed, tr.nerf2sfm)
    out = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
    zmaps = []
    for k in range(n):
        Rg, tg = assets["gt_poses"][k]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rg, tg
        RE._render_depth(tr.testbed, tr.nerf2sfm, T, camera, 8, out)
        g = out.cpu().numpy()
        on = (g[..., 3] >= 0.5) & (g[..., 0] > 0)
        with np.errstate(all="ignore"):
            zmaps.append(np.where(on, g[..., 0] / np.where(on, g[..., 3], 1) * zs, 0.0))
    z = np.stack(zmaps)
    scale = float(z.max() / 20000)
    counts = np.where(z > 0, np.rint(z / scale), 60000).astype(np.uint16)
    sx, sy, _ = SE.sensor_alignment(camera)
    return SE.shifted_sensor(counts, (-sx, -sy)), scale


def _run_r9(dev, assets, frames, names, option):
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, reference_points="render",
                             depth_refine=option)
    warm = 10
    for i in range(warm):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(warm, len(names)):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    hist = tr.pose_history
    tracked = sum(bool(hist[n]["tracked"]) for n in names[warm:])
    err = [float(np.linalg.norm(np.asarray(hist[n]["T_refined"].numpy()[1], np.float64) - assets["gt_poses"][i][1]))
           for i, n in enumerate(names) if i >= warm and hist[n].get("success")]
    refined = sum(bool(hist[n].get("depth_refined")) for n in names[warm:])
    return {"fps": tracked / dt, "tracked": tracked, "mean_translation_error": float(np.mean(err)) if err else None,
            "depth_refined_frames": refined, "renders_ahead_used": int(tr.renders_ahead_used)}


def part_b(dev, n_frames):
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    n = n_frames + 10
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n)
    probe = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, probe.testbed)
    names = [f"{i:06d}.png" for i in range(n)]
    images, scale = _sensor_frames(dev, assets, probe, n)
    del probe
    table = {name: images[k] for k, name in enumerate(names)}
    option = DR.DepthRefine(lookup=table.get, sensor_depth_scale=scale)
    runs = {"off": [], "on": []}
    for _ in range(2):
        for key, opt in (("off", None), ("on", option)):
            runs[key].append(_run_r9(dev, assets, frames, names, opt))
            print("r9", key, runs[key][-1], flush=True)
    return {"r9_640x480_render_points": {k: {"fps": [r["fps"] for r in v], "median_fps": float(np.median([r["fps"] for r in v])),
                                             **{m: v[-1][m] for m in v[-1] if m != "fps"}} for k, v in runs.items()},
            "frames": n_frames, "sfm_units_per_count": scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_refine.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    for part, fn in (("a", lambda: part_a(dev)), ("b", lambda: part_b(dev, args.frames))):
        if part in args.parts:
            result[part] = fn()
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
