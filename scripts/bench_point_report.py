"""Measurements of the opt-in per-point residual report -> profiles/r10_point_report.json.

  (a) launch time of pxt_lm_point_report, one problem of N = 2048 points, at both lane-group widths (C = 32: 8 lanes per
      point, C = 128: 32), with and without the [N, 8] point records, beside pxt_lm_information on the same problem in
      the same run: HIP events around batches of 50 launches with the host parked ahead of the stream, median of 7.
  (b) tracked frames/s of the r9 tracker (640x480) with the option off / "summary" / "full", same process, same
      scene, alternating three times.

    python scripts/bench_point_report.py [--parts ab] [--frames 200] [--out FILE]
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
from pixtrack_amd.optimizer import cstride_for  # noqa: E402
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9  # noqa: E402
from pixtrack_amd.synthetic import make_lm_scene, make_tracking_assets, render_query_frames  # noqa: E402


def pack_level(scene, level, dev):
    fq = scene.feats_query[level]
    Cc = fq.shape[0] - 1
    cs = cstride_for(Cc)
    h, w = fq.shape[1:]
    fmap = torch.zeros(h, w, cs)
    d = fq[:-1]
    fmap[..., :Cc] = (d / d.norm(dim=0, keepdim=True).clamp_min(1e-12)).permute(1, 2, 0)
    fmap[..., Cc] = fq[-1]
    fr = scene.feats_ref[level]
    fref = torch.zeros(fr.shape[0], cs)
    fref[:, :Cc] = fr[:, :-1] / fr[:, :-1].norm(dim=1, keepdim=True).clamp_min(1e-12)
    fref[:, Cc] = fr[:, -1]
    return fmap.to(dev).contiguous(), fref.to(dev).contiguous(), Cc, scene.camera.scale(scene.scales[level])


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
    rows = []
    N = 2048
    sc = make_lm_scene(seed=1401, width=640, height=480, n_points=N)
    p3d = torch.from_numpy(sc.p3d).float().to(dev).contiguous()
    pose = torch.from_numpy(np.concatenate([sc.R_init.reshape(-1), sc.t_init]).astype(np.float32)).to(dev)
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    conf = _lib.LmConf()
    conf.pad, conf.loss, conf.loss_alpha, conf.loss_scale, conf.min_valid = 1, 2, 0.0, 0.1, 10
    conf_ref = C.byref(conf)
    for level, Cc in ((0, 32), (1, 128)):
        fmap, fref, C_, cam = pack_level(sc, level, dev)
        assert C_ == Cc
        h, w, cs = (int(x) for x in fmap.shape)

        def fill(q):
            q.p3d, q.point_mask, q.n_points = p3d.data_ptr(), None, N
            q.level.fmap, q.level.fref = fmap.data_ptr(), fref.data_ptr()
            q.level.h, q.level.w, q.level.C, q.level.cstride = h, w, Cc, cs
            q.level.cam[:] = [float(x) for x in cam.as10().tolist()]
            q.level.ndist = int(cam._data.shape[-1] - 6)
            q.pose, q.pose_is_lm_record = pose.data_ptr(), 0

        # (the native entries called directly on problem arrays built once: a timed call costs the host microseconds)
        info = (_lib.LmInfoProblem * 1)()
        fill(info[0])
        rec = torch.zeros(48, device=dev)
        info[0].out = rec.data_ptr()
        info_ws = torch.zeros(int(L.pxt_lm_information_workspace_bytes(1)), dtype=torch.uint8, device=dev)

        def launch_info():
            rc = L.pxt_lm_information(info, 1, conf_ref, info_ws.data_ptr(), stream)
            assert rc == 0, rc

        row = {"N": N, "C": Cc, "lanes_per_point": 8 if Cc <= 32 else 32, "information": _time_launches(dev, launch_info)}
        rep_ws = torch.zeros(int(L.pxt_lm_point_report_workspace_bytes(1)), dtype=torch.uint8, device=dev)
        for key, with_points in (("report_summary_only", False), ("report_with_points", True)):
            prob = (_lib.LmReportProblem * 1)()
            fill(prob[0])
            summ = torch.zeros(16, device=dev)
            pts = torch.zeros(N, 8, device=dev)
            prob[0].inlier_weight = 0.5
            prob[0].points, prob[0].summary = (pts.data_ptr() if with_points else None), summ.data_ptr()

            def launch_report():
                rc = L.pxt_lm_point_report(prob, 1, conf_ref, rep_ws.data_ptr(), stream)
                assert rc == 0, rc

            row[key] = _time_launches(dev, launch_report)
            row["n_valid"] = float(summ[1])
        rows.append(row)
        print(row, flush=True)
    return rows


# ------------------------------------------------------------------------------------------------ (b)
def _run_r9(dev, assets, frames, names, mode):
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, point_report=mode)
    warm = 10
    for i in range(warm):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(warm, len(names)):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    tracked = sum(bool(tr.pose_history[n]["tracked"]) for n in names[warm:])
    ratios = [tr.pose_history[n].get("inlier_ratio") for n in names[warm:]]
    ratios = [r for r in ratios if r is not None]
    return tracked / dt, tracked, (float(np.median(ratios)) if ratios else None)


def part_b(dev, n_frames):
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n_frames + 10)
    probe = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, probe.testbed)
    names = [f"{i:06d}.png" for i in range(n_frames + 10)]
    del probe
    modes = (("off", False), ("summary", "summary"), ("full", "full"))
    fps = {k: [] for k, _ in modes}
    extra = {}
    for _ in range(3):
        for key, mode in modes:
            f, tracked, ratio = _run_r9(dev, assets, frames, names, mode)
            fps[key].append(f)
            extra[key] = {"tracked": tracked, "median_inlier_ratio": ratio}
            print("r9", key, f, tracked, ratio, flush=True)
    return {"r9_640x480": {k: {"fps": v, "median": float(np.median(v)), "spread": float(max(v) - min(v)), **extra[k]}
                           for k, v in fps.items()}, "frames": n_frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10_point_report.json"))
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
