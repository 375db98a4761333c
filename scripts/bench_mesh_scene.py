"""Measurements of mutual occlusion in lock-step mesh tracking -> profiles/mesh_scene.json.

  (a) device time of ONE pxt_mesh_render_scene_batch call against ONE pxt_mesh_render_frame_batch call on the same views
      (that entry point's launches are the parent's, unchanged): K in {2, 4, 8} objects in one scene, each with a
      tracker frame's two views - a 640 x 480 depth_nz plane (the scene view) and a 640 x 480 rgb_u8 image at supersample
      2 - at 5120 and 81 920 triangles, the objects side by side and partly behind each other.  bench_mesh_template.py's
      method: HIP events around 20 queued calls with the host parked ahead of the stream, the two sides alternating, five
      repeats, medians.  The planes and record words 0..9 of the two sides are compared byte for byte inside the run.
      The extra launch is not timed alone: the difference of the two medians stands for it, next to the time of a
      device-to-device copy of the key bytes it reads (K x 640 x 480 x 8), taken the same way.
  (b) two synthetic mesh objects in ONE 640 x 480 image, the second partly behind the first, tracked in lock-step with
      the option off and on in one process: frames per second by the host clock around the frame loops (each ends in
      a device synchronise), frames tracked, rotation / translation errors against ground truth, hidden pixels and
      gated points per frame.  No ratio and no accuracy threshold is fixed: "it does not help on this scene" is a
      result.

    python scripts/bench_mesh_scene.py [--parts ab] [--frames 60] [--out FILE]
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
sys.path.insert(0, str(ROOT / "scripts"))

from bench_mesh_lockstep import _Batch  # noqa: E402
from bench_mesh_template import QH, QW, _alternate, _pose  # noqa: E402
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402


class _SceneBatch(_Batch):
    """The scene call on a _Batch's views: every item's first view is a member of scene 0."""

    def __init__(self, items, r_grow):
        super().__init__(items)
        shapes = tuple((r.n_triangles, tuple((W, H, S, tuple(want)) for _, W, H, S, want in q)) for r, q in items)
        scenes = [[0] + [None] * (len(q) - 1) for _, q in items]
        (self.view_scene, self.occ_offsets, occ_bytes, need), = R._scene_plan(shapes, R._batch_plan(shapes), scenes)
        self.occluder = torch.empty(occ_bytes, dtype=torch.uint8, device=items[0][0].device)
        self.ws = torch.empty(need, dtype=torch.uint8, device=items[0][0].device)
        self.r_grow = int(r_grow)

    def __call__(self):
        ops.mesh_render_scene_batch(*self.meshes, self.view_mesh, self.views, self.geometry, self.offsets, self.view_scene,
                                    self.r_grow, self.occ_offsets, *self.bufs, self.occluder, self.records, self.ws)


def part_a(dev, r_grow):
    from pixtrack_amd.synthetic import make_bumpy_mesh

    rows = []
    f_q = 1.2 * QW
    for subdivisions in (4, 6):
        renderers, requests = [], []
        for k in range(8):
            V, F, UV, FUV, tex = make_bumpy_mesh(1012 + k, subdivisions)
            Rm, t = _pose(V, f_q, (0.6 - 0.03 * k) * QH)
            t = t + np.asarray([(k - 3.5) * 0.35, 0.0, 0.0])  # side by side, neighbours overlap
            v = R.pack_view(Rm, t, f_q, f_q, QW / 2 - 0.5, QH / 2 - 0.5, 1e-6, 1.0 / (2.0 * t[2]))
            renderers.append(R.MeshRenderer(V, F, dev, uvs=UV, triangle_uvs=FUV, texture=tex))
            requests.append([(v, QW, QH, 1, ("depth_nz",)), (v, QW, QH, 2, ("rgb_u8",))])
        for K in (2, 4, 8):
            lo = (8 - K) // 2  # the middle K: neighbours
            items = list(zip(renderers[lo:lo + K], requests[lo:lo + K]))
            plain, scene = _Batch(items), _SceneBatch(items, r_grow)
            keys_src = torch.empty(K * QW * QH * 8, dtype=torch.uint8, device=dev)
            keys_dst = torch.empty_like(keys_src)
            sides = {"batch": plain, "scene": scene, "key_copy": lambda: keys_dst.copy_(keys_src)}
            for side in sides.values():
                side()
            torch.cuda.synchronize(dev)
            equal = all(bool(torch.equal(a, b)) for a, b in zip(plain.bufs, scene.bufs) if a is not None) and \
                bool(torch.equal(plain.records[:, :10], scene.records[:, :10]))
            us = _alternate(dev, sides)
            med = {n: float(np.median(v)) for n, v in us.items()}
            rec = scene.records.cpu().numpy()
            row = {"objects": K, "triangles": renderers[0].n_triangles, "views": 2 * K, "query": [QW, QH], "r_grow": scene.r_grow,
                   "batch_us": us["batch"], "scene_us": us["scene"], "key_copy_us": us["key_copy"],
                   "batch_us_median": med["batch"], "scene_us_median": med["scene"], "key_copy_us_median": med["key_copy"],
                   "extra_us": med["scene"] - med["batch"], "ratio": med["scene"] / med["batch"],
                   "batch_spread_us": float(max(us["batch"]) - min(us["batch"])), "key_bytes": int(keys_src.numel()),
                   "planes_and_records_equal": equal, "covered": [int(rec[2 * k, 0]) for k in range(K)],
                   "hidden": [int(rec[2 * k, 10]) for k in range(K)], "occluder": [int(rec[2 * k, 11]) for k in range(K)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def _composite(objs, poses, i, cam, g, sigma=2.0):
    """Frame i: each object at its pose, 4 x 4 samples per pixel; where both are seen, the nearer one on top."""
    rgba, z = [], []
    for (_, renderer), T in zip(objs, poses):
        v = R.view_record(cam, T[i])
        out = renderer.render_frame([(v, QW, QH, 4, ("rgba",)), (v, QW, QH, 1, ("depth",))], download_records=False)
        rgba.append(out[0]["rgba"])
        d = out[1]["depth"]
        z.append(torch.where(d[..., 3] > 0, d[..., 0], torch.full_like(d[..., 0], 1e30)))
    first = (z[0] <= z[1])[..., None]
    top, below = torch.where(first, rgba[0], rgba[1]), torch.where(first, rgba[1], rgba[0])
    img = (top[..., :3] + (1.0 - top[..., 3:]) * below[..., :3]) * 255.0
    return (img + (torch.randn(img.shape, generator=g) * sigma).to(img.device)).clamp_(0, 255).round_().contiguous()


def part_b(dev, n_frames, r_grow):
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker, MutualOcclusion
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets
    from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

    warm = 10
    names = [f"{i:06d}.png" for i in range(n_frames)]
    shifts = ((-0.20, 0.0, 0.0), (0.75, 0.0, 1.3))  # the second object 1.3 behind, its left third behind the first
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for k in range(2):
            out = Path(tmp) / f"object{k}"
            out.mkdir()
            assets = make_mesh_tracking_assets(seed=1041 + k, width=QW, height=QH, n_frames=n_frames, out_dir=out, device=dev)
            V, F = assets["mesh"][:2]
            objs.append((assets, R.MeshRenderer(V, F, dev, **assets["mesh_shading"])))
        poses = []
        for (assets, _), s in zip(objs, shifts):
            Ts = []
            for Rg, tg in assets["gt_poses"]:
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = Rg, tg + np.asarray(s)
                Ts.append(T)
            poses.append(Ts)
        cam = Camera.from_colmap(objs[0][0]["query_camera"])
        g = torch.Generator(device="cpu").manual_seed(5)
        frames = [_composite(objs, poses, i, cam, g) for i in range(n_frames)]
        for label, option in (("off", None), ("on", MutualOcclusion(scenes=[0, 0], r_grow=r_grow)), ("off again", None)):
            trs = []
            for (assets, renderer), Ts in zip(objs, poses):
                tr = PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, template=MeshTemplate(renderer, supersample=2),
                                         assets={k: assets[k] for k in ("model3d", "weights", "covis", "upright_ref_img")})
                tr.pose = Pose.from_Rt(Ts[0][:3, :3], Ts[0][:3, 3])
                trs.append(tr)
            multi = MultiObjectTracker(trs, n_groups=1, mutual_occlusion=option)
            for i in range(warm):
                multi.run_single_frames([(names[i], frames[i])] * 2)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n_frames):
                multi.run_single_frames([(names[i], frames[i])] * 2)
            torch.cuda.synchronize(dev)
            seconds = time.perf_counter() - t0
            row = {"option": label, "r_grow": r_grow, "frames": n_frames, "frames_timed": 2 * (n_frames - warm),
                   "frames_per_second": 2 * (n_frames - warm) / seconds, "solo_frames": multi.solo_frames,
                   "lockstep_frames": multi.lockstep_frames, "objects": []}
            for tr, Ts in zip(trs, poses):
                rot, tra = [], []
                for i, n in enumerate(names):
                    ret = tr.pose_history[n]
                    Rt, t = (ret["T_refined"] if ret.get("success") else ret["T_init"]).numpy()
                    rot.append(float(np.degrees(geodesic_distance_for_rotations(Rt, Ts[i][:3, :3]))))
                    tra.append(float(np.linalg.norm(t - Ts[i][:3, 3])))
                obj = {"tracked": sum(bool(tr.pose_history[n]["tracked"]) for n in names),
                       "rotation_error_deg_mean": float(np.mean(rot)), "rotation_error_deg_max": float(np.max(rot)),
                       "translation_error_mean": float(np.mean(tra)), "translation_error_max": float(np.max(tra))}
                if option is not None:
                    hist = [tr.pose_history[n] for n in names]
                    obj.update(applied=sum(bool(h["mutual_occlusion_applied"]) for h in hist),
                               hidden_pixels_mean=float(np.mean([h["n_mutually_hidden_pixels"] for h in hist])),
                               hidden_fraction_mean=float(np.mean([h["mutually_hidden_fraction"] or 0.0 for h in hist])),
                               occluder_pixels_mean=float(np.mean([h["n_mutual_occluder_pixels"] for h in hist])),
                               points_gated_mean=float(np.mean([h["n_points_gated_mutual"] for h in hist])))
                row["objects"].append(obj)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--r_grow", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_scene.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_scene.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts:
        result["scene_call"] = part_a(dev, args.r_grow)
        save()
    if "b" in args.parts:
        result["two_objects_640x480"] = part_b(dev, args.frames, args.r_grow)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
