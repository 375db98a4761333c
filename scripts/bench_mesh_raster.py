"""Measurements of the mesh rasteriser -> profiles/mesh_raster.json.

  (a) device time per view of pxt_mesh_raster at 640 x 480 for the 128^3 mesh of the synthetic NeRF (about a pixel per
      triangle), a 12-triangle box that fills the image (the list path) and an icosphere of 81 920 triangles: HIP events
      around batches of calls with the host parked ahead of the stream, median of 7; calls of 1 and of 8 views.  In the
      same process: a device-to-device copy that moves the bytes the design must move per view - the key plane cleared
      (8 B per pixel), read back (8 B), the float4 image written (16 B), the vertices (12 B each) and indices (12 B per
      triangle) read once - a copy of half that size, since a copy reads and writes its size.
  (b) 200 frames of evaluate_poses_mesh against evaluate_poses_rendered (two spp-8 NeRF Depth renders per frame) on the
      same poses: host clock around a call that ends with the records on the host, best of 3.

    python scripts/bench_mesh_raster.py [--parts ab] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import mesh as M  # noqa: E402
from pixtrack_amd import mesh_evaluation as ME  # noqa: E402
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402

W, H = 640, 480


def _time_launches(dev, launch, per=20, reps=7, warm=3):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize(dev)
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
        e0.record()
        for _ in range(per):
            launch()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / per)
    return {"us_per_call_median": float(np.median(us)), "us_min": float(min(us)), "us_max": float(max(us))}


def _object(dev, tmp, n_frames):
    """The synthetic object on disk and loaded: (assets, testbed, nerf2sfm)."""
    from pixtrack_amd.synthetic import make_tracking_assets, write_object_dir
    from pixtrack_amd.utils.ingp_utils import initialize_ingp, load_nerf2sfm

    assets = make_tracking_assets(width=W, height=H, n_frames=n_frames)
    obj = Path(tmp) / "object"
    write_object_dir(assets, obj)
    testbed = initialize_ingp(str(obj / "pixtrack/instant-ngp/snapshots/weights.msgpack"),
                              [[float(x) for x in c] for c in assets["aabb"]], device=str(dev))
    return assets, testbed, load_nerf2sfm(str(obj / "pixtrack/pixsfm/dataset/nerf2sfm.pkl"))


def _box():
    V = np.asarray([(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
    F = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2),
         (1, 3, 7), (1, 7, 5)]
    return V, np.asarray(F)


def _raster_row(dev, name, V, F, views):
    r = R.MeshRenderer(V, F, dev)
    row = {"mesh": name, "vertices": r.n_vertices, "triangles": r.n_triangles, "width": W, "height": H}
    _, _, rec = r.render_depth(views[:1], W, H)
    row["record_of_view_0"] = [int(x) for x in rec[0]]
    row["covered_fraction"] = float(rec[0, R.W_COVERED]) / (W * H)
    for P in (1, 8):
        v = torch.from_numpy(np.ascontiguousarray(views[:P])).to(dev)
        depth = torch.empty(P, H, W, 4, dtype=torch.float32, device=dev)
        records = torch.empty(P, R.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, r.n_triangles, W, H)), dtype=torch.uint8, device=dev)
        t = _time_launches(dev, lambda: ops.mesh_raster(r.vertices, r.triangles, v, depth, None, records, ws))
        row[f"views_{P}"] = {**t, "us_per_view": t["us_per_call_median"] / P, "workspace_bytes": ws.numel()}
    moved = W * H * (8 + 8 + 16) + r.n_vertices * 12 + r.n_triangles * 12
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    row["bytes_moved_per_view"] = moved
    row["copy_of_those_bytes"] = _time_launches(dev, lambda: dst.copy_(src))
    row["ratio_to_copy_1_view"] = row["views_1"]["us_per_view"] / row["copy_of_those_bytes"]["us_per_call_median"]
    row["ratio_to_copy_8_views"] = row["views_8"]["us_per_view"] / row["copy_of_those_bytes"]["us_per_call_median"]
    print(row, flush=True)
    return row


def part_a(dev):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        _, testbed, _ = _object(dev, tmp, 2)
        mesh = M.extract_mesh(testbed, 128, colors=False)
        lo, hi = np.asarray(testbed.render_aabb.min), np.asarray(testbed.render_aabb.max)
        centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
        focal = 0.5 * W / np.tan(np.radians(20.0))
        cams = ME.look_at_cameras(centre, 1.05 * radius / np.sin(np.arctan(0.5 * H / focal)), 8)
        views = np.stack([R.ngp_view_record(C, focal, W, H) for C in cams])
        rows.append(_raster_row(dev, "synthetic NeRF at 128^3", mesh["V"], mesh["F"], views))
    V, F = _box()
    eye = np.eye(3)
    outside = np.stack([R.pack_view(eye, (0.01 * k, 0.0, 2.2), 500.0, 500.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_raster_row(dev, "12-triangle box whose front face fills the image", V, F, outside))
    V, F = R.icosphere(6)
    sphere = np.stack([R.pack_view(eye, (0.0, 0.0, 2.6 + 0.01 * k), 600.0, 600.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_raster_row(dev, "icosphere of 81920 triangles", V, F, sphere))
    return rows


def part_b(dev, n_frames=200):
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.render_evaluation import evaluate_poses_rendered
    from pixtrack_amd.synthetic import perturb_pose

    with tempfile.TemporaryDirectory() as tmp:
        assets, testbed, nerf2sfm = _object(dev, tmp, n_frames)
        mesh = M.extract_mesh(testbed, 128, colors=False, nerf2sfm=nerf2sfm)
        cam = Camera.from_colmap(assets["query_camera"])
        rng = np.random.default_rng(0)
        poses = {}
        for k, (Rg, tg) in enumerate(assets["gt_poses"]):
            Re, te = perturb_pose(Rg, tg, rng, 1.0, 0.01 * mesh["diameter"], assets["center"])
            poses[f"{k:06d}.png"] = {"success": True, "camera": cam,
                                     "gt_pose": Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg)),
                                     "T_refined": Pose.from_Rt(torch.from_numpy(Re), torch.from_numpy(te))}
        renderer = R.MeshRenderer(mesh["V"], mesh["F"], dev)

        def clock(fn):
            ts, last = [], None
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                last = fn()
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t0)
            return ts, last

        t_mesh, res_mesh = clock(lambda: ME.evaluate_poses_mesh(poses, renderer, mesh["diameter"]))
        t_nerf, res_nerf = clock(lambda: evaluate_poses_rendered(poses, testbed, nerf2sfm, mesh["diameter"]))
        brief = lambda r: {k: r[k] for k in ("n_evaluated", "ar_vsd", "iou_mean", "mean_abs_dz_mean", "vsd_mean")}
        row = {"frames": n_frames, "width": W, "height": H, "triangles": int(len(mesh["F"])),
               "evaluate_poses_mesh_seconds": t_mesh, "evaluate_poses_rendered_seconds": t_nerf,
               "mesh_ms_per_frame_best": 1e3 * min(t_mesh) / n_frames, "nerf_ms_per_frame_best": 1e3 * min(t_nerf) / n_frames,
               "speedup_best": min(t_nerf) / min(t_mesh), "mesh": brief(res_mesh), "nerf": brief(res_nerf)}
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_raster.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts:
        result["raster"] = part_a(dev)
        save()
    if "b" in args.parts:
        result["evaluation_200_frames"] = part_b(dev)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
