"""Measurements of reference_points="template"  -> profiles/mesh_points.json.

  (a) device time of ONE pxt_points_from_depth_views call on K in {1, 2, 4, 8} real 640 x 480 depth planes of a mesh
      template's frame call, against K calls of pxt_points_from_depth (the one-view kernel it generalises) on the same
      planes, same bytes; beside both a float4 copy of the planes.  The recipe of 3.6: HIP events around 20 queued
      calls, host parked ahead of the stream, median of 7, the sides alternating.
  (b) tracked frames/s and error maxima of the solo r9 tracker on the synthetic mesh object at 640 x 480 with "template"
      against "sfm", alternated three times in one process (3.6(b)'s method).
  (c) eight synthetic mesh objects in lock-step (one group) with "template" against "sfm": bench_mesh_lockstep.py's set-up.

    python scripts/bench_mesh_points.py [--parts abc] [--frames 100] [--objects 8] [--out FILE]
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
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402

QW, QH, N_MAX, ERODE, MIN_ALPHA = 640, 480, 2048, 1, 0.5


def _alternate(dev, sides, per=20, reps=7, warm=3):
    """{name: [microseconds per call] x reps} of the callables in ``sides``, alternating, host parked ahead of the stream."""
    for fn in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize(dev)
    out = {k: [] for k in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(4_000_000)
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / per)
    return out


def _rot_err(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T) - 1) / 2, -1, 1)))


# ------------------------------------------------------------------------------------------------ (a)
def part_a(dev):
    from pixtrack_amd.synthetic import make_bumpy_mesh

    f_q = 1.2 * QW
    planes, views = [], []
    for k in range(8):
        V, F, UV, FUV, tex = make_bumpy_mesh(1012 + k, 4)
        radius = float(np.linalg.norm(V, axis=1).max())
        z = f_q * radius / ((0.75 - 0.03 * k) * QH / 2)  # the silhouette fills that share of the image height
        view = R.pack_view(np.eye(3), [0.0, 0.0, z], f_q, f_q, QW / 2 - 0.5, QH / 2 - 0.5, 1e-6, 1.0 / (z + radius))
        renderer = R.MeshRenderer(V, F, dev, uvs=UV, triangle_uvs=FUV, texture=tex)
        planes.append(renderer.render_frame([(view, QW, QH, 1, ("depth",))], download_records=False)[0]["depth"].clone())
        views.append(view)
    L, C = _lib.lib(), _lib.C
    ws1 = torch.empty(int(L.pxt_points_from_depth_workspace_bytes(QW, QH)), dtype=torch.uint8, device=dev)
    xform = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    rows = []
    for K in (1, 2, 4, 8):
        need = int(L.pxt_points_from_depth_views_workspace_bytes(K, (C.c_int32 * (2 * K))(*([QW, QH] * K))))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        p3d = torch.empty(K, N_MAX, 3, dtype=torch.float32, device=dev)
        valid = torch.empty(K, N_MAX, dtype=torch.uint8, device=dev)
        rec = torch.zeros(K, 4, dtype=torch.int32).pin_memory()
        rec1 = [torch.zeros(4, dtype=torch.int32).pin_memory() for _ in range(K)]
        flat = [float(x) for v in views[:K] for x in v]
        src = torch.stack(planes[:K])
        dst = torch.empty_like(src)

        def batched():
            ops.points_from_depth_views(planes[:K], flat, MIN_ALPHA, ERODE, N_MAX, p3d, valid, rec, ws)

        def one_by_one():
            for k in range(K):
                ops.points_from_depth(planes[k], xform, f_q, 1.0, MIN_ALPHA, ERODE, N_MAX, p3d[k], valid[k], rec1[k], ws1)

        sides = {"views_call": batched, "one_view_calls": one_by_one, "float4_copy": lambda: dst.copy_(src)}
        us = _alternate(dev, sides)
        torch.cuda.synchronize(dev)
        med = {k: float(np.median(v)) for k, v in us.items()}
        nbytes = 16 * QW * QH * K
        row = {"views": K, "size": [QW, QH], "n_max": N_MAX, "erode": ERODE, "us": us, "us_median": med,
               "ratio_views_call_to_one_view_calls": med["views_call"] / med["one_view_calls"],
               "plane_bytes": nbytes, "views_call_GBps": nbytes / med["views_call"] * 1e-3,
               "one_view_calls_GBps": nbytes / med["one_view_calls"] * 1e-3,
               "float4_copy_GBps_read": nbytes / med["float4_copy"] * 1e-3,
               "records": rec.tolist(), "records_equal_one_view": rec.tolist() == [r.tolist() for r in rec1]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


# ------------------------------------------------------------------------------------------------ (b), (c)
def _objects(dev, tmp, n_objects, n_frames):
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames

    objs = []
    for k in range(n_objects):
        out = Path(tmp) / f"object{k}"
        out.mkdir()
        assets = make_mesh_tracking_assets(seed=1031 + k, width=QW, height=QH, n_frames=n_frames, out_dir=out, device=dev)
        V, F = assets["mesh"][:2]
        renderer = R.MeshRenderer(V, F, dev, **assets["mesh_shading"])
        objs.append((assets, renderer, render_mesh_query_frames(assets, renderer)))
    return objs


def _tracker(dev, tmp, obj, mode):
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    assets, renderer, _ = obj
    return PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, template=MeshTemplate(renderer, supersample=2),
                               assets={k: assets[k] for k in ("model3d", "weights", "covis", "upright_ref_img")},
                               reference_points=mode)


def _quality(tr, assets, names):
    rot, trans = [], []
    for i, n in enumerate(names):
        ret = tr.pose_history[n]
        Rt, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
        rot.append(_rot_err(Rt, assets["gt_poses"][i][0]))
        trans.append(float(np.linalg.norm(np.asarray(t, np.float64) - assets["gt_poses"][i][1])))
    return {"max_rot_err_rad": max(rot), "max_trans_err": max(trans),
            "tracked": int(sum(bool(tr.pose_history[n]["tracked"]) for n in names))}


def part_b(dev, n_frames, warm=10):
    names = [f"{i:06d}.png" for i in range(n_frames)]
    with tempfile.TemporaryDirectory() as tmp:
        obj = _objects(dev, tmp, 1, n_frames)[0]
        runs = {"sfm": [], "template": []}
        quality = {}
        for _ in range(3):
            for mode in ("sfm", "template"):
                tr = _tracker(dev, tmp, obj, mode)
                for i in range(warm):
                    tr.run_single_frame((names[i], obj[2][i]))
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for i in range(warm, n_frames):
                    tr.run_single_frame((names[i], obj[2][i]))
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                tracked = sum(bool(tr.pose_history[n]["tracked"]) for n in names[warm:])
                runs[mode].append(tracked / dt)
                quality[mode] = _quality(tr, obj[0], names)
                if mode == "template":
                    quality[mode]["n_reference_points"] = [tr.pose_history[n]["n_reference_points"] for n in names[::10]]
                    quality[mode]["reference_point_stride"] = [tr.pose_history[n]["reference_point_stride"] for n in names[::10]]
                print(json.dumps({"r9": mode, "fps": runs[mode][-1], **quality[mode]}), flush=True)
    return {"frames": n_frames, "size": [QW, QH],
            "fps": {k: {"runs": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))} for k, v in runs.items()},
            "ratio_template_to_sfm": float(np.median(runs["template"]) / np.median(runs["sfm"])), "quality": quality}


def part_c(dev, n_frames, n_objects, warm=10):
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker

    names = [f"{i:06d}.png" for i in range(n_frames)]
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        objs = _objects(dev, tmp, n_objects, n_frames)
        for rep in range(2):
            for mode in ("sfm", "template"):
                trs = [_tracker(dev, tmp, obj, mode) for obj in objs]
                multi = MultiObjectTracker(trs, n_groups=1)
                for i in range(warm):
                    multi.run_single_frames([(names[i], frames[i]) for _, _, frames in objs])
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for i in range(warm, n_frames):
                    multi.run_single_frames([(names[i], frames[i]) for _, _, frames in objs])
                torch.cuda.synchronize(dev)
                seconds = time.perf_counter() - t0
                q = [_quality(tr, obj[0], names) for tr, obj in zip(trs, objs)]
                row = rows.setdefault(mode, {"frames_per_second": [], "objects": n_objects, "frames": n_frames})
                row["frames_per_second"].append(n_objects * (n_frames - warm) / seconds)
                row.update(tracked=[x["tracked"] for x in q], max_rot_err_rad=max(x["max_rot_err_rad"] for x in q),
                           max_trans_err=max(x["max_trans_err"] for x in q), points_calls=multi.points_calls,
                           solo_frames=multi.solo_frames, lockstep_frames=multi.lockstep_frames)
                print(json.dumps({"lock-step": mode, **row}), flush=True)
    for row in rows.values():
        row["frames_per_second_median"] = float(np.median(row["frames_per_second"]))
    rows["ratio_template_to_sfm"] = rows["template"]["frames_per_second_median"] / rows["sfm"]["frames_per_second_median"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_points.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_points.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    for part, key, fn in (("a", "points_call", lambda: part_a(dev)), ("b", "r9_640x480", lambda: part_b(dev, args.frames)),
                          ("c", "lockstep_640x480", lambda: part_c(dev, args.frames, args.objects))):
        if part in args.parts:
            result[key] = fn()
            save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
