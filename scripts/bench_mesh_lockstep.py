"""Measurements of lock-step tracking from mesh templates -> profiles/mesh_lockstep.json.

  (a) device time of ONE pxt_mesh_render_frame_batch call for K in {2, 4, 8} objects, each with a tracker frame's two
      views - a 640 x 480 depth_nz plane and a 640 x 480 rgb_u8 image at supersample 2 - against the way to the same
      planes without it: K consecutive pxt_mesh_render_frame calls.  The synthetic tracking object at 5120 and at
      81 920 triangles (K different seeds of it), textured.  bench_mesh_template.py's method: HIP events around 20 queued
      calls with the host parked ahead of the stream, the two sides alternating, five repeats, medians.  The criterion:
      the batched call's median is not above the K-call side's median plus that side's own max - min over its five
      repeats.  The planes of the two sides are compared byte for byte inside the run.
  (b) eight synthetic mesh objects at 640 x 480 tracked in lock-step (one group and two) against the same eight
      trackers run one after the other in the same process: total frames per second by the host clock around the
      frame loops (each ends in a device synchronise), the device time of a step's render calls, every frame tracked.
      Recorded without a bar.

    python scripts/bench_mesh_lockstep.py [--parts ab] [--frames 100] [--objects 8] [--out FILE]
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

from bench_mesh_template import QH, QW, _alternate, _Frame, _pose  # noqa: E402
from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402


class _Batch:
    """One batched call with its buffers allocated once (what mesh_render.render_frame_batch does per call, without the
    allocations and the plan lookup)."""

    def __init__(self, items):
        self.items = items
        shapes = tuple((r.n_triangles, tuple((W, H, S, tuple(want)) for _, W, H, S, want in q)) for r, q in items)
        (_, _, self.view_mesh, self.geometry, self.offsets, sizes, need), = R._batch_plan(shapes)
        dev = items[0][0].device
        self.bufs = [None if n == 0 else torch.empty(n // (4 if k in (0, 2) else 1), dtype=torch.float32 if k in (0, 2) else torch.uint8,
                                                     device=dev) for k, n in enumerate(sizes)]
        self.views = torch.from_numpy(np.ascontiguousarray(np.stack([v[0] for _, q in items for v in q]).astype(np.float32)))
        self.records = torch.empty(len(self.view_mesh), R.RECORD, dtype=torch.int32, device=dev)
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rs = [r for r, _ in items]
        self.meshes = ([r.vertices for r in rs], [r.triangles for r in rs], [r.colors for r in rs], [r.uvs for r in rs],
                       [r.triangle_uvs for r in rs], [r.texture for r in rs])

    def __call__(self):
        ops.mesh_render_frame_batch(*self.meshes, self.view_mesh, self.views, self.geometry, self.offsets, *self.bufs,
                                    self.records, self.ws)

    def plane(self, p, name):
        k = R.FRAME_OUTPUTS.index(name)
        W, H = self.geometry[3 * p:3 * p + 2]
        ch, o = (4, 3, 4, 1)[k], self.offsets[4 * p + k]
        e = (16, 3, 16, 1)[k] // ch
        return self.bufs[k][o // e:o // e + W * H * ch].view(H, W, ch)


class _Calls:
    """K one-mesh frame calls, one after the other."""

    def __init__(self, frames):
        self.frames = frames

    def __call__(self):
        for f in self.frames:
            f()


def _sides_equal(batch, frames):
    """Every plane and record of the batched call equals the one-mesh calls', byte for byte."""
    p, ok = 0, True
    for f in frames:
        for q, (_, _, _, _, want) in enumerate(f.requests):
            for name in want:
                ok = ok and bool(torch.equal(batch.plane(p, name), f.plane(q, name)))
            ok = ok and bool(torch.equal(batch.records[p], f.records[q]))
            p += 1
    return ok


def part_a(dev):
    from pixtrack_amd.synthetic import make_bumpy_mesh

    rows = []
    f_q = 1.2 * QW
    for subdivisions in (4, 6):
        renderers, requests = [], []
        for k in range(8):
            V, F, UV, FUV, tex = make_bumpy_mesh(1012 + k, subdivisions)
            Rm, t = _pose(V, f_q, (0.75 - 0.03 * k) * QH)
            v = R.pack_view(Rm, t, f_q, f_q, QW / 2 - 0.5, QH / 2 - 0.5, 1e-6, 1.0 / (2.0 * t[2]))
            renderers.append(R.MeshRenderer(V, F, dev, uvs=UV, triangle_uvs=FUV, texture=tex))
            requests.append([(v, QW, QH, 1, ("depth_nz",)), (v, QW, QH, 2, ("rgb_u8",))])
        for K in (2, 4, 8):
            frames = [_Frame(r, q) for r, q in zip(renderers[:K], requests[:K])]
            batch = _Batch(list(zip(renderers[:K], requests[:K])))
            sides = {"batch": batch, "calls": _Calls(frames)}
            for side in sides.values():
                side()
            torch.cuda.synchronize(dev)
            equal = _sides_equal(batch, frames)
            us = _alternate(dev, sides)
            bm, cm = float(np.median(us["batch"])), float(np.median(us["calls"]))
            spread = float(max(us["calls"]) - min(us["calls"]))
            row = {"objects": K, "triangles": renderers[0].n_triangles, "views": 2 * K, "query": [QW, QH], "reference": [QW, QH],
                   "supersample": 2, "batch_us": us["batch"], "calls_us": us["calls"], "batch_us_median": bm,
                   "calls_us_median": cm, "calls_spread_us": spread, "criterion_met": bool(bm <= cm + spread),
                   "ratio": bm / cm, "planes_and_records_equal": equal,
                   "covered_fraction_query": [float(batch.records[2 * k, R.W_COVERED].item()) / (QW * QH) for k in range(K)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def part_b(dev, n_frames, n_objects):
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames

    warm = 10
    names = [f"{i:06d}.png" for i in range(n_frames)]
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for k in range(n_objects):
            out = Path(tmp) / f"object{k}"
            out.mkdir()
            assets = make_mesh_tracking_assets(seed=1031 + k, width=QW, height=QH, n_frames=n_frames, out_dir=out, device=dev)
            V, F = assets["mesh"][:2]
            renderer = R.MeshRenderer(V, F, dev, **assets["mesh_shading"])
            objs.append((assets, renderer, render_mesh_query_frames(assets, renderer)))
            print(json.dumps({"object": k, "triangles": int(len(F))}), flush=True)

        def trackers():
            return [PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, template=MeshTemplate(r, supersample=2),
                                        assets={k: a[k] for k in ("model3d", "weights", "covis", "upright_ref_img")})
                    for a, r, _ in objs]

        def tracked(trs):
            return [sum(bool(tr.pose_history[n]["tracked"]) for n in names) for tr in trs]

        rows = []
        # one after the other: tracker by tracker, each over its own sequence
        trs = trackers()
        seconds = 0.0
        for tr, (_, _, frames) in zip(trs, objs):
            for i in range(warm):
                tr.run_single_frame((names[i], frames[i]))
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n_frames):
                tr.run_single_frame((names[i], frames[i]))
            torch.cuda.synchronize(dev)
            seconds += time.perf_counter() - t0
        timed = n_objects * (n_frames - warm)
        solo_fps = timed / seconds
        calls = _Calls([_Frame(tr.template.renderer, tr.template.requests(tr.pose, tr.camera, tr._reference_camera())) for tr in trs])
        us = _alternate(dev, {"calls": calls})["calls"]
        rows.append({"mode": "one after the other", "objects": n_objects, "frames_timed": timed, "frames_per_second": solo_fps,
                     "tracked": tracked(trs), "frames": n_frames, "render_calls_us_per_step": us,
                     "render_calls_us_per_step_median": float(np.median(us)), "render_calls_per_step": n_objects})
        print(json.dumps(rows[-1]), flush=True)
        for n_groups in (1, 2):
            trs = trackers()
            multi = MultiObjectTracker(trs, n_groups=n_groups)
            for i in range(warm):
                multi.run_single_frames([(names[i], frames[i]) for _, _, frames in objs])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n_frames):
                multi.run_single_frames([(names[i], frames[i]) for _, _, frames in objs])
            torch.cuda.synchronize(dev)
            seconds = time.perf_counter() - t0
            groups = [[trs[k] for k in g.members] for g in multi.groups]
            batches = [_Batch([(tr.template.renderer, tr.template.requests(tr.pose, tr.camera, tr._reference_camera())) for tr in g])
                       for g in groups]
            us = _alternate(dev, {"batch": _Calls(batches)})["batch"]  # (the groups' calls one after the other, on one stream)
            rows.append({"mode": f"lock-step, {n_groups} group(s)", "objects": n_objects, "frames_timed": timed,
                         "frames_per_second": timed / seconds, "ratio_to_one_after_the_other": (timed / seconds) / solo_fps,
                         "tracked": tracked(trs), "frames": n_frames, "solo_frames": multi.solo_frames,
                         "lockstep_frames": multi.lockstep_frames,
                         "template_frames_batched": [tr.template_frames_batched for tr in trs],
                         "render_calls_us_per_step": us, "render_calls_us_per_step_median": float(np.median(us)),
                         "render_calls_per_step": n_groups})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_lockstep.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_lockstep.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts:
        result["batch_call"] = part_a(dev)
        save()
    if "b" in args.parts:
        result["tracker_640x480"] = part_b(dev, args.frames, args.objects)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
