"""Measurements of the sensor options for mesh templates -> profiles/occlusion_views.json.

  (a) device time of ONE pxt_occlusion_mask_views call for K = 1 / 2 / 4 / 8 views against K pxt_occlusion_mask calls
      queued back to back, same process, same image pairs (640 x 480, radii (1, 3), the disc-and-slab scene of
      scripts/bench_occlusion_mask.py; every view has planes of its own, all name ONE sensor image): HIP events around 50
      queued calls with the host parked ahead of the stream, median of 7 with min and max.  Criterion for K >= 2: the
      batched call is faster than the K calls by more than the two sides' min-max ranges taken together.
      With --parent_lib: the single call of another build of the library (the parent commit's), alternating with this
      one's, so that a change of the single call's code shows up.
  (b) tracked frames/s of the mesh tracker with reference_points="template" at 640 x 480: options off / occlusion on /
      depth refinement on, same process, alternating, 100 timed frames after 10; and the mean translation error.
  (c) the same three settings for eight mesh trackers in lock-step that share one sensor image per step - eight
      instances of ONE object and sequence, so that the one image is every tracker's true depth: medians of five with
      the spread (every run is reported).

    python scripts/bench_occlusion_views.py [--parts abc] [--frames 100] [--parent_lib FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_occlusion_mask import _image, _time_launches  # noqa: E402
from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import depth_refinement as DR  # noqa: E402
from pixtrack_amd import occlusion as OC  # noqa: E402

W, H = 640, 480
RADII = (1, 3)


# ------------------------------------------------------------------------------------------------ (a)
def _single_prototype(L):
    res, args = _lib.PROTOTYPES["pxt_occlusion_mask"]
    L.pxt_occlusion_mask.restype, L.pxt_occlusion_mask.argtypes = res, args
    res, args = _lib.PROTOTYPES["pxt_occlusion_mask_workspace_bytes"]
    L.pxt_occlusion_mask_workspace_bytes.restype, L.pxt_occlusion_mask_workspace_bytes.argtypes = res, args
    return L


def part_a(dev, parent_lib):
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    img, sensor, nz = _image(W, H)
    d_sensor = torch.from_numpy(sensor.view(np.int16)).to(dev)
    plain = torch.empty(H, W, dtype=torch.uint8, device=dev)
    d_nz = torch.from_numpy(nz).to(dev)
    assert L.pxt_depth_mask_plane(d_nz.data_ptr(), H, W, 1, 5, plain.data_ptr(), None, stream) == 0
    kmax = 8
    imgs = [torch.from_numpy(img).to(dev) for _ in range(kmax)]
    plains = [plain.clone() for _ in range(kmax)]
    masks = [torch.empty_like(plain) for _ in range(kmax)]
    occs = [torch.empty_like(plain) for _ in range(kmax)]
    recs = torch.zeros(kmax, OC.RECORD, dtype=torch.int32, device=dev)
    ws1 = [torch.empty(int(L.pxt_occlusion_mask_workspace_bytes(W, H)), dtype=torch.uint8, device=dev) for _ in range(kmax)]
    ref = OC.occlusion_mask_reference(img, sensor, plain.cpu().numpy(), (0, 0), 0.5, 1e-3, 0.2, *RADII)

    def single(lib, k):
        rc = lib.pxt_occlusion_mask(imgs[k].data_ptr(), d_sensor.data_ptr(), plains[k].data_ptr(), W, H, 0, 0, 0.5, 1e-3, 0.2,
                                    RADII[0], RADII[1], masks[k].data_ptr(), occs[k].data_ptr(), recs[k].data_ptr(),
                                    ws1[k].data_ptr(), stream)
        assert rc == 0, rc

    def check(K):
        torch.cuda.synchronize(dev)
        got = recs.cpu().numpy()
        for k in range(K):
            assert np.array_equal(got[k], ref["record"]) and np.array_equal(masks[k].cpu().numpy(), ref["mask"])
            assert np.array_equal(occs[k].cpu().numpy(), ref["occluder"])

    out = {"size": f"{W}x{H}", "radii": list(RADII), "record": OC.decode_record(ref["record"]), "views": []}
    for K in (1, 2, 4, 8):
        table = (_lib.OcclusionView * K)()
        for k in range(K):
            v = table[k]
            v.depth, v.sensor, v.mask_in = imgs[k].data_ptr(), d_sensor.data_ptr(), plains[k].data_ptr()
            v.mask_out, v.occluder = masks[k].data_ptr(), occs[k].data_ptr()
            v.width, v.height, v.shift_x, v.shift_y, v.sensor_q, v.delta_q = W, H, 0, 0, 1e-3, 0.2
        need = int(L.pxt_occlusion_mask_views_workspace_bytes(K, (C.c_int32 * (2 * K))(*([W, H] * K))))
        wsK = torch.empty(need, dtype=torch.uint8, device=dev)

        def batched():
            rc = L.pxt_occlusion_mask_views(table, K, 0.5, RADII[0], RADII[1], recs.data_ptr(), wsK.data_ptr(), stream)
            assert rc == 0, rc

        def singles():
            for k in range(K):
                single(L, k)

        recs.zero_()
        tb = _time_launches(dev, batched)
        check(K)
        recs.zero_()
        ts = _time_launches(dev, singles)
        check(K)
        gain = ts["us_per_call_median"] - tb["us_per_call_median"]
        ranges = (tb["us_max"] - tb["us_min"]) + (ts["us_max"] - ts["us_min"])
        row = {"K": K, "batched": tb, "k_single_calls": ts, "gain_us": gain, "ranges_us": ranges,
               "criterion_met": bool(gain > ranges) if K >= 2 else None}
        out["views"].append(row)
        print(row, flush=True)
    if parent_lib:
        P = _single_prototype(C.CDLL(str(parent_lib), mode=C.RTLD_LOCAL))
        runs = {"this": [], "parent": []}
        for _ in range(3):
            for name, lib in (("this", L), ("parent", P)):
                runs[name].append(_time_launches(dev, lambda lib=lib: single(lib, 0)))
                check(1)
        out["single_call_against_parent"] = {name: {"us_medians": [r["us_per_call_median"] for r in rs],
                                                    "us_min": min(r["us_min"] for r in rs),
                                                    "us_max": max(r["us_max"] for r in rs)} for name, rs in runs.items()}
        print(out["single_call_against_parent"], flush=True)
    return out


# ------------------------------------------------------------------------------------------------ (b), (c)
def _mesh_object(dev, seed, n, out_dir):
    from pixtrack_amd import mesh_render as R
    from pixtrack_amd.geometry import Camera
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames

    assets = make_mesh_tracking_assets(seed=seed, width=W, height=H, n_frames=n, out_dir=out_dir, device=dev)
    V, F = assets["mesh"][:2]
    renderer = R.MeshRenderer(V, F, dev, **assets["mesh_shading"])
    frames = render_mesh_query_frames(assets, renderer)
    camera = Camera.from_colmap(assets["query_camera"])
    z = np.zeros((n, H, W))
    for k, (Rg, tg) in enumerate(assets["gt_poses"]):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rg, tg
        g = renderer.render_frame([(R.view_record(camera, T), W, H, 1, ("depth",))], download_records=False)[0]["depth"].cpu().numpy()
        z[k] = np.where(g[..., 3] > 0, g[..., 0], 0.0)
    return assets, renderer, frames, z


TRACKER_KEYS = ("model3d", "weights", "covis", "upright_ref_img")


def _tracker(dev, obj, **kw):
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    assets, renderer = obj[0], obj[1]
    return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets={k: assets[k] for k in TRACKER_KEYS if k in assets},
                               template=MeshTemplate(renderer, supersample=2), reference_points="template", **kw)


def _trans_error(tr, gt, names):
    out = []
    for n, (_Rg, tg) in zip(names, gt):
        ret = tr.pose_history[n]
        T = ret["T_refined"] if ret.get("success") else ret["T_init"]
        out.append(float(np.linalg.norm(np.asarray(T.numpy()[1], np.float64) - tg)))
    return float(np.mean(out))


def _settings(table, scale):
    return {"off": lambda: {}, "occlusion": lambda: {"occlusion": OC.OcclusionMask(lookup=table.get, sensor_depth_scale=scale)},
            "depth_refine": lambda: {"depth_refine": DR.DepthRefine(lookup=table.get, sensor_depth_scale=scale)}}


def part_b(dev, n_frames, tmp):
    warm = 10
    n = n_frames + warm
    names = [f"{i:06d}.png" for i in range(n)]
    obj = _mesh_object(dev, 1031, n, tmp / "solo")
    scale = float(obj[3].max() / 20000)
    counts = np.where(obj[3] > 0, np.rint(obj[3] / scale), 60000).astype(np.uint16)
    table = {name: counts[k] for k, name in enumerate(names)}
    runs = {}
    for _ in range(3):
        for key, make in _settings(table, scale).items():
            tr = _tracker(dev, obj, **make())
            for i in range(warm):
                tr.run_single_frame((names[i], obj[2][i]))
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n):
                tr.run_single_frame((names[i], obj[2][i]))
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            tracked = sum(bool(tr.pose_history[m]["tracked"]) for m in names[warm:])
            r = {"fps": tracked / dt, "tracked": tracked, "mean_translation_error": _trans_error(tr, obj[0]["gt_poses"], names),
                 "sensor_uploads": int(tr.sensor_uploads)}
            runs.setdefault(key, []).append(r)
            print("solo", key, r, flush=True)
    return {"frames": n_frames, "runs": runs,
            "median_fps": {k: float(np.median([r["fps"] for r in v])) for k, v in runs.items()}}


def part_c(dev, n_frames, tmp, n_objects=8, reps=5):
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker

    warm = 10
    n = n_frames + warm
    names = [f"{i:06d}.png" for i in range(n)]
    # ONE image per step that is right for all eight: eight trackers of one object (eight DIFFERENT objects drawn into
    # one image overlap at its centre, where the nearest surface is mostly another object's - DESIGN 3.23 has that run)
    objs = [_mesh_object(dev, 1031, n, tmp / "obj")] * n_objects
    z = objs[0][3]
    scale = float(z.max() / 20000)
    counts = np.where(z > 0, np.rint(z / scale), 60000).astype(np.uint16)
    table = {name: counts[k] for k, name in enumerate(names)}
    runs = {}
    for _ in range(reps):
        for key, make in _settings(table, scale).items():
            opts = make()  # one lookup for the eight
            trackers = [_tracker(dev, o, **opts) for o in objs]
            multi = MultiObjectTracker(trackers, n_groups=1)
            for i in range(warm):
                multi.run_single_frames([(names[i], o[2][i]) for o in objs])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n):
                multi.run_single_frames([(names[i], o[2][i]) for o in objs])
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            tracked = sum(bool(tr.pose_history[m]["tracked"]) for tr in trackers for m in names[warm:])
            r = {"fps": tracked / dt, "tracked": tracked, "sensor_uploads": int(multi.sensor_uploads),
                 "occlusion_view_calls": int(multi.occlusion_view_calls), "depth_refine_calls": int(multi.depth_refine_calls),
                 "mean_translation_error": float(np.mean([_trans_error(tr, o[0]["gt_poses"], names) for tr, o in zip(trackers, objs)]))}
            runs.setdefault(key, []).append(r)
            print("lock-step", key, r, flush=True)
    return {"frames": n_frames, "objects": n_objects, "runs": runs,
            "median_fps": {k: float(np.median([r["fps"] for r in v])) for k, v in runs.items()},
            "fps_min_max": {k: [min(r["fps"] for r in v), max(r["fps"] for r in v)] for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occlusion_views.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for part, fn in (("a", lambda: part_a(dev, args.parent_lib)), ("b", lambda: part_b(dev, args.frames, tmp)),
                         ("c", lambda: part_c(dev, args.frames, tmp, reps=args.reps))):
            if part in args.parts:
                result[part] = fn()
                path.parent.mkdir(parents=True, exist_ok=True)
                path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
