"""Measurements of the sensor-depth VSD comparison -> profiles/sensor_vsd.json.

Time of one pxt_sensor_vsd call (both launches, 10 taus + the finite-pixel slot, a ray plane) for 640 x 480 x {1, 32, 200}
pairs and 1024 x 768 x 32 pairs, without a shift and with YCB-Video's (-7, 1): HIP events around 20 calls with the host
parked ahead of the stream, median of 7.  Bytes read per call: 34 per pixel and pair (two float4 images and the 2-byte
sensor counts; the ray plane, shared by every pair and cache-resident, the partials and the records are left out).

Yardsticks, timed in the same process on the same buffers: pxt_depth_agreement (32 B per pixel and pair) and a float4
device-to-device copy of one image stack (16 B read + 16 B written per pixel and pair).  The aim of DESIGN 3.11 -
bytes/s within 10 % of pxt_depth_agreement's on the two HBM-sized cases - is reported as met or missed per case.

    python scripts/bench_sensor_vsd.py [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import render_evaluation as RE  # noqa: E402
from pixtrack_amd import sensor_evaluation as SE  # noqa: E402

CASES = ((640, 480, 1), (640, 480, 32), (640, 480, 200), (1024, 768, 32))
HBM_SIZED = {(640, 480, 200), (1024, 768, 32)}  # inputs beyond the 256 MiB Infinity Cache
HBM_PEAK = 8.0e12
SHIFT_YCB = (-7, 1)
PER, WINDOWS = 20, 7


def _time(torch, dev, launch):
    """Median, min and max seconds per call: PER calls between two events, the host parked ahead, WINDOWS windows."""
    for _ in range(3):
        launch()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
        e0.record()
        for _ in range(PER):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / PER)
    return float(np.median(ms)) * 1e-3, float(min(ms)) * 1e-3, float(max(ms)) * 1e-3


def measure():
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
        for off in (-0.05, 0.05):
            disc = ((xx - W * (0.5 + off)) ** 2 + (yy - H * 0.5) ** 2 <= (0.3 * H) ** 2).float()
            one = torch.zeros(H, W, 4, device=dev)
            one[..., 3] = disc
            one[..., 0] = disc * (0.3 + 0.1 * torch.sin(xx * 0.05) * torch.cos(yy * 0.04))
            imgs.append(one.expand(P, H, W, 4).contiguous())
        est, gt = imgs
        # the sensor sees the ground truth (1e-4 per count), a far background and a slab over the left third
        counts = torch.where(gt[0, ..., 3] > 0, gt[0, ..., 0] * 1e4, torch.full_like(gt[0, ..., 0], 20000.0))
        counts[:, :W // 3] = 1000.0
        sensor = counts.round().to(torch.int32).to(torch.int16).expand(P, H, W).contiguous()
        ray = torch.from_numpy(np.sqrt(1.0 + ((np.arange(W) + 0.5 - W / 2)[None, :] / (1.6 * W)) ** 2
                                       + ((np.arange(H) + 0.5 - H / 2)[:, None] / (1.6 * W)) ** 2).astype(np.float32)).to(dev)
        dst = torch.empty_like(est)
        rec = torch.zeros(P, SE.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.pxt_sensor_vsd_workspace_bytes(P, W, H)), dtype=torch.uint8, device=dev)
        rec_da = torch.zeros(P, RE.RECORD, dtype=torch.int32, device=dev)
        ws_da = torch.empty(int(L.pxt_depth_agreement_workspace_bytes(P, W, H)), dtype=torch.uint8, device=dev)

        def vsd(shift):
            def launch():
                rc = L.pxt_sensor_vsd(est.data_ptr(), gt.data_ptr(), sensor.data_ptr(), ray.data_ptr(), P, W, H, shift[0],
                                      shift[1], 0.5, 1e-4, 0.0015, tqs, len(tq), rec.data_ptr(), ws.data_ptr(), stream)
                assert rc == 0, rc
            return launch

        def agreement():
            rc = L.pxt_depth_agreement(est.data_ptr(), gt.data_ptr(), P, W, H, 0.5, tqs, len(tq), rec_da.data_ptr(),
                                       ws_da.data_ptr(), stream)
            assert rc == 0, rc

        npix = P * W * H
        row = {"width": W, "height": H, "pairs": P, "input_MB": npix * 34 / 1e6, "hbm_sized": (W, H, P) in HBM_SIZED}
        for name, launch, nbytes in (("sensor_vsd", vsd((0, 0)), npix * 34), ("sensor_vsd_shifted", vsd(SHIFT_YCB), npix * 34),
                                     ("depth_agreement", agreement, npix * 32),
                                     ("float4_copy", lambda: dst.copy_(est), npix * 32)):
            t, lo, hi = _time(torch, dev, launch)
            row[name] = {"bytes_per_call": nbytes, "us_per_call_median": t * 1e6, "us_min": lo * 1e6, "us_max": hi * 1e6,
                         "bytes_per_s": nbytes / t, "fraction_of_hbm_peak_8.0TBs": nbytes / t / HBM_PEAK}
        for name in ("sensor_vsd", "sensor_vsd_shifted"):
            ratio = row[name]["bytes_per_s"] / row["depth_agreement"]["bytes_per_s"]
            row[name]["bytes_per_s_over_depth_agreement"] = ratio
            row[name]["aim_within_10_percent"] = ("met" if ratio >= 0.9 else "missed") if row["hbm_sized"] else "not an HBM case"
        r = rec.cpu().numpy().view(np.uint32)
        row["record_of_pair_0"] = {"n_vis_est": int(r[0, 0]), "n_vis_gt": int(r[0, 1]), "n_inter": int(r[0, 2]),
                                   "n_union": int(r[0, 3]), "n_sil_gt": int(r[0, 9])}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del est, gt, imgs, dst, sensor
    return {"hbm": "8.0 TB/s peak (MI355X_MICROARCH)", "bytes_per_pixel_and_pair": {"sensor_vsd": 34, "depth_agreement": 32,
                                                                                     "float4_copy": "16 read + 16 written"},
            "calls_per_window": PER, "windows": WINDOWS, "thresholds": len(tq), "shifted": list(SHIFT_YCB), "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sensor_vsd.json"))
    args = ap.parse_args()
    result = measure()
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(result, indent=1))
    print(json.dumps({"written": str(path)}))


if __name__ == "__main__":
    main()
