"""Measurements of the opt-in occlusion handling -> profiles/occlusion_mask.json.

  (a) device time per pxt_occlusion_mask call (both launches) at 640 x 480 and 1024 x 768, default radii (1, 3) and the
      largest (8, 8), and per pxt_points_visible call at N = 600 and 2048: HIP events around batches of 50 calls with
      the host parked ahead of the stream, median of 7.  In the same process, on the same image: pxt_depth_mask_plane
      (erode 1, dilate 5: the frame's plain mask) and a plain copy of the 16 + 2 bytes per pixel the pass reads (two
      device-to-device copies, which also write what they read).  The image is a disc silhouette with a slab occluder
      over its left third.
  (b) tracked frames/s of the r9 tracker (640 x 480, SfM points) with the option on against off, same process, same
      scene, alternating; render-ahead stays on in both.  The sensor frames are Depth renders at the ground-truth
      poses, quantised to uint16 (no occluder: the pass runs on every steady frame and removes nothing).

    python scripts/bench_occlusion_mask.py [--parts ab] [--frames 100] [--out FILE]
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
from pixtrack_amd import occlusion as OC  # noqa: E402


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
    return {"us_per_call_median": float(np.median(us)), "us_min": float(min(us)), "us_max": float(max(us)),
            "host_us_per_call": float(np.median(host))}


# ------------------------------------------------------------------------------------------------ (a)
def _image(W, H, seed=3):
    """A disc silhouette 2.0 deep (alpha 1), the sensor on it except over its left third, where a slab stands at 1.0;
    far background elsewhere; one raw count is 1e-3."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (xx - W / 2) ** 2 + (yy - H / 2) ** 2 <= (0.35 * H) ** 2
    img = np.zeros((H, W, 4), np.float32)
    img[..., 3] = disc
    img[..., 0] = np.where(disc, 2.0 + 0.05 * rng.random((H, W)), 0.0)
    sensor = np.where(disc, 2000, 6000).astype(np.uint16)
    sensor[:, int(W / 2 - 0.35 * H):int(W / 2 - 0.35 * H / 3)] = 1000
    sensor[rng.random((H, W)) < 0.02] = 0
    nz = (disc | (rng.random((H, W)) < 0.001)).astype(np.uint8)
    return img, sensor, nz


def part_a(dev):
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    out = {"occlusion_mask": [], "points_visible": []}
    for W, H in ((640, 480), (1024, 768)):
        img, sensor, nz = _image(W, H)
        d_img = torch.from_numpy(img).to(dev)
        d_sensor = torch.from_numpy(sensor.view(np.int16)).to(dev)
        d_nz = torch.from_numpy(nz).to(dev)
        plain = torch.empty(H, W, dtype=torch.uint8, device=dev)
        mask, occ = torch.empty_like(plain), torch.empty_like(plain)
        rec = torch.zeros(OC.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.pxt_occlusion_mask_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
        img2, sensor2 = torch.empty_like(d_img), torch.empty_like(d_sensor)

        def plane():
            rc = L.pxt_depth_mask_plane(d_nz.data_ptr(), H, W, 1, 5, plain.data_ptr(), None, stream)
            assert rc == 0, rc

        def copy():
            img2.copy_(d_img)
            sensor2.copy_(d_sensor)

        plane()
        row = {"size": f"{W}x{H}", "depth_mask_plane": _time_launches(dev, plane), "copy_18B_per_pixel": _time_launches(dev, copy)}
        for radii in ((1, 3), (8, 8)):
            def launch():
                rc = L.pxt_occlusion_mask(d_img.data_ptr(), d_sensor.data_ptr(), plain.data_ptr(), W, H, 0, 0, 0.5, 1e-3,
                                          0.2, radii[0], radii[1], mask.data_ptr(), occ.data_ptr(), rec.data_ptr(),
                                          ws.data_ptr(), stream)
                assert rc == 0, rc

            t = _time_launches(dev, launch)
            torch.cuda.synchronize(dev)
            ref = OC.occlusion_mask_reference(img, sensor, plain.cpu().numpy(), (0, 0), 0.5, 1e-3, 0.2, *radii)
            assert np.array_equal(rec.cpu().numpy(), ref["record"]) and np.array_equal(mask.cpu().numpy(), ref["mask"])
            key = f"occlusion_mask_r{radii[0]}_{radii[1]}"
            row[key] = {**t, "record": OC.decode_record(rec)}
            row[key]["ratio_to_depth_mask_plane"] = t["us_per_call_median"] / row["depth_mask_plane"]["us_per_call_median"]
            row[key]["ratio_to_copy"] = t["us_per_call_median"] / row["copy_18B_per_pixel"]["us_per_call_median"]
        out["occlusion_mask"].append(row)
        print(row, flush=True)
        if (W, H) != (640, 480):
            continue
        cam10 = [float(W), float(H), 768.0, 768.0, W / 2 - 0.5, H / 2 - 0.5, -0.05, 0.0, 0.0, 0.0]
        T = (C.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2.0)
        cam = (C.c_float * 10)(*cam10)
        rng = np.random.default_rng(9)
        for N in (600, 2048):
            pts = np.stack([rng.uniform(-0.9, 0.9, N), rng.uniform(-0.7, 0.7, N), rng.uniform(-0.2, 0.2, N)], 1).astype(np.float32)
            d_pts = torch.from_numpy(pts).to(dev)
            valid = torch.empty(N, dtype=torch.uint8, device=dev)

            def launch():
                rc = L.pxt_points_visible(d_pts.data_ptr(), None, N, T, cam, 2, occ.data_ptr(), W, H, valid.data_ptr(),
                                          rec.data_ptr(), stream)
                assert rc == 0, rc

            t = _time_launches(dev, launch)
            torch.cuda.synchronize(dev)
            r = {"N": N, "size": f"{W}x{H}", **t, "record": OC.decode_record(rec)}
            out["points_visible"].append(r)
            print(r, flush=True)
    return out


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

    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, occlusion=option)
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
    applied = sum(bool(hist[n].get("occlusion_applied")) for n in names[warm:])
    return {"fps": tracked / dt, "tracked": tracked, "occlusion_applied_frames": applied,
            "occluder_pixels": sum(int(hist[n].get("n_occluder_pixels") or 0) for n in names[warm:]),
            "renders_ahead_used": int(tr.renders_ahead_used)}


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
    option = OC.OcclusionMask(lookup=table.get, sensor_depth_scale=scale)
    runs = {"off": [], "on": []}
    for _ in range(3):
        for key, opt in (("off", None), ("on", option)):
            runs[key].append(_run_r9(dev, assets, frames, names, opt))
            print("r9", key, runs[key][-1], flush=True)
    return {"r9_640x480": {k: {"fps": [r["fps"] for r in v], "median_fps": float(np.median([r["fps"] for r in v])),
                               **{m: v[-1][m] for m in v[-1] if m != "fps"}} for k, v in runs.items()},
            "frames": n_frames, "sfm_units_per_count": scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occlusion_mask.json"))
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
