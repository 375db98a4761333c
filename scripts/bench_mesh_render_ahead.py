"""Measurements of render-ahead for mesh templates -> profiles/mesh_render_ahead.json.

  (a) device time of ONE pxt_mesh_render_frame_batch_posed call against ONE pxt_mesh_render_frame_batch call on the same
      views: 1, 4 and 8 synthetic mesh objects, each with a tracker frame's two views - a 640 x 480 depth_nz plane and a
      640 x 480 rgb_u8 image at supersample 2.  bench_mesh_template.py's method: HIP events around 20 queued calls with
      the host parked ahead of the stream, the two sides alternating, five repeats, medians.  The posed side's planes
      are compared with the plain side's inside the run (the plain side is given the floats posed_view_reference forms).
      Reported: the difference of the medians beside the plain call's own max - min over its five repeats.
  (b) the r9 tracker on the synthetic mesh object at 640 x 480, 100 frames of which 90 are timed, supersample 1, 2 and 4:
      MeshTemplate(render_ahead=True) against render_ahead=False in the same process, the sides alternating, five
      repeats each (a fresh tracker per repeat).  Frames per second by the host clock around the frame loop, which ends
      in a device synchronise.  The criterion: the on median exceeds the off median by more than the off side's
      max - min.  Beside it: the host time a frame spends queueing the posed call and verifying it, and the device time
      of the frame's render call.
  (c) eight synthetic mesh objects in lock-step (one group), the same way.

    python scripts/bench_mesh_render_ahead.py [--parts abc] [--frames 100] [--objects 8] [--out FILE]
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

TRACKER_KEYS = ("model3d", "weights", "covis", "upright_ref_img")


class _PosedBatch(_Batch):
    """The same call with every view's pose read on the device from a pinned record that holds it."""

    def __init__(self, items, radii):
        super().__init__(items)
        full = self.views.numpy()
        self.records_lm = []
        for v in full:
            rec = np.zeros(16, np.float32)
            rec[:12], rec[15] = v[:12], 1.0
            self.records_lm.append(torch.from_numpy(rec).pin_memory())
        self.radii = [float(radii[m]) for m in self.view_mesh]
        host = full.copy()
        host[:, :12], host[:, 17] = 0.0, 0.0
        self.views = torch.from_numpy(host)
        self.views_out = torch.zeros(len(full), R.VIEW_OUT, dtype=torch.float32).pin_memory()
        self.drawn = np.stack([R.posed_view_reference(rec, v, radius)[0]
                               for rec, v, radius in zip(self.records_lm, host, self.radii)])

    def __call__(self):
        ops.mesh_render_frame_batch_posed(*self.meshes, self.view_mesh, self.views, self.geometry, self.offsets,
                                          self.records_lm, self.radii, *self.bufs, self.records, self.ws, self.views_out)


def part_a(dev):
    from pixtrack_amd.synthetic import make_bumpy_mesh

    rows = []
    f_q = 1.2 * QW
    renderers, requests, radii = [], [], []
    for k in range(8):
        V, F, UV, FUV, tex = make_bumpy_mesh(1012 + k, 4)
        Rm, t = _pose(V, f_q, (0.75 - 0.03 * k) * QH)
        v = R.pack_view(Rm, t, f_q, f_q, QW / 2 - 0.5, QH / 2 - 0.5, 1e-6, 1.0)
        renderers.append(R.MeshRenderer(V, F, dev, uvs=UV, triangle_uvs=FUV, texture=tex))
        requests.append([(v, QW, QH, 1, ("depth_nz",)), (v, QW, QH, 2, ("rgb_u8",))])
        radii.append(float(np.linalg.norm(V.astype(np.float64), axis=1).max()))
    for K in (1, 4, 8):
        items = list(zip(renderers[:K], requests[:K]))
        posed = _PosedBatch(items, radii[:K])
        plain = _Batch([(r, [(posed.drawn[2 * k + j], *q[1:]) for j, q in enumerate(qs)]) for k, (r, qs) in enumerate(items)])
        sides = {"plain": plain, "posed": posed}
        for side in sides.values():
            side()
        torch.cuda.synchronize(dev)
        equal = all(bool(torch.equal(plain.plane(p, name), posed.plane(p, name)))
                    for p in range(2 * K) for name in (("depth_nz",) if p % 2 == 0 else ("rgb_u8",)))
        equal = equal and bool(torch.equal(plain.records, posed.records))
        rows_out = posed.views_out.numpy()
        floats_equal = bool(np.array_equal(rows_out[:, :20].view(np.uint32), posed.drawn.view(np.uint32)) and (rows_out[:, 20] == 1.0).all())
        us = _alternate(dev, sides)
        pm, qm = float(np.median(us["plain"])), float(np.median(us["posed"]))
        row = {"objects": K, "triangles": renderers[0].n_triangles, "views": 2 * K, "query": [QW, QH], "reference": [QW, QH],
               "supersample": 2, "plain_us": us["plain"], "posed_us": us["posed"], "plain_us_median": pm, "posed_us_median": qm,
               "difference_us": qm - pm, "plain_spread_us": float(max(us["plain"]) - min(us["plain"])),
               "planes_and_records_equal": equal, "views_out_equal_reference": floats_equal}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def _timed(fn):
    """Wraps a bound method so that the host seconds spent in it add up in ``fn.seconds``."""
    def wrapper(*args, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*args, **kw)
        finally:
            wrapper.seconds += time.perf_counter() - t0
    wrapper.seconds = 0.0
    return wrapper


def _summary(fps):
    """{side: [frames per second] x repeats} -> medians, spreads and the criterion."""
    on, off = fps["on"], fps["off"]
    on_m, off_m, spread = float(np.median(on)), float(np.median(off)), float(max(off) - min(off))
    return {"on_fps": on, "off_fps": off, "on_fps_median": on_m, "off_fps_median": off_m, "off_spread_fps": spread,
            "gain_fps": on_m - off_m, "ratio": on_m / off_m, "criterion_met": bool(on_m - off_m > spread)}


def part_b(dev, n_frames, repeats=5, warm=10):
    from bench_mesh_template import _Frame
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames

    rows = []
    names = [f"{i:06d}.png" for i in range(n_frames)]
    with tempfile.TemporaryDirectory() as tmp:
        assets = make_mesh_tracking_assets(width=QW, height=QH, n_frames=n_frames, out_dir=tmp, device=dev)
        V, F = assets["mesh"][:2]
        renderer = R.MeshRenderer(V, F, dev, **assets["mesh_shading"])
        frames = render_mesh_query_frames(assets, renderer)
        for S in (1, 2, 4):
            fps = {"on": [], "off": []}
            poses, host_ms, counters, tr = {}, [], None, None
            for _ in range(repeats):
                for side in ("off", "on"):
                    tr = PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, assets={k: assets[k] for k in TRACKER_KEYS},
                                             template=MeshTemplate(renderer, supersample=S, render_ahead=side == "on"))
                    tr._render_ahead_mesh = _timed(tr._render_ahead_mesh)
                    tr._verify_render_ahead = _timed(tr._verify_render_ahead)
                    for i in range(warm):
                        tr.run_single_frame((names[i], frames[i]))
                    torch.cuda.synchronize(dev)
                    tr._render_ahead_mesh.seconds = tr._verify_render_ahead.seconds = 0.0
                    t0 = time.perf_counter()
                    for i in range(warm, n_frames):
                        tr.run_single_frame((names[i], frames[i]))
                    torch.cuda.synchronize(dev)
                    fps[side].append((n_frames - warm) / (time.perf_counter() - t0))
                    poses[side] = np.stack([tr.pose_history[n]["T_refined"].as12().double().numpy().reshape(-1) for n in names])
                    if side == "on":
                        host_ms.append((1e3 * tr._render_ahead_mesh.seconds / (n_frames - warm),
                                        1e3 * tr._verify_render_ahead.seconds / (n_frames - warm)))
                        counters = dict(used=tr.renders_ahead_used, rejected=tr.renders_ahead_rejected,
                                        dropped=tr.renders_ahead_dropped, stale=tr.renders_ahead_stale)
            call = _Frame(renderer, tr.template.requests(tr.pose, tr.camera, tr._reference_camera()))
            us = _alternate(dev, {"frame": call})["frame"]
            row = {"supersample": S, "frames": n_frames, "frames_timed": n_frames - warm, **_summary(fps),
                   "poses_bit_identical": bool(np.array_equal(poses["on"], poses["off"])), "counters_on": counters,
                   "tracked_on": sum(bool(h["tracked"]) for h in tr.pose_history.values()),
                   "host_ms_per_frame_queueing_the_posed_call": float(np.median([h[0] for h in host_ms])),
                   "host_ms_per_frame_verifying": float(np.median([h[1] for h in host_ms])),
                   "render_call_us_median": float(np.median(us)), "render_views": len(call.requests)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def part_c(dev, n_frames, n_objects, repeats=5, warm=10):
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames

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
        fps = {"on": [], "off": []}
        poses, multi, trs = {}, None, None
        timed = n_objects * (n_frames - warm)
        for _ in range(repeats):
            for side in ("off", "on"):
                trs = [PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, assets={k: a[k] for k in TRACKER_KEYS},
                                           template=MeshTemplate(r, supersample=2, render_ahead=side == "on"))
                       for a, r, _ in objs]
                multi = MultiObjectTracker(trs, n_groups=1)
                for i in range(warm):
                    multi.run_single_frames([(names[i], f[i]) for _, _, f in objs])
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for i in range(warm, n_frames):
                    multi.run_single_frames([(names[i], f[i]) for _, _, f in objs])
                torch.cuda.synchronize(dev)
                fps[side].append(timed / (time.perf_counter() - t0))
                poses[side] = np.stack([tr.pose_history[n]["T_refined"].as12().double().numpy().reshape(-1)
                                        for tr in trs for n in names])
        row = {"objects": n_objects, "groups": 1, "supersample": 2, "frames": n_frames, "frames_timed": timed, **_summary(fps),
               "poses_bit_identical": bool(np.array_equal(poses["on"], poses["off"])),
               "posed_calls_on": multi.mesh_ahead_calls, "head_of_step_calls_on": multi.mesh_prime_calls,
               "renders_ahead_used_on": [tr.renders_ahead_used for tr in trs],
               "renders_ahead_rejected_on": [tr.renders_ahead_rejected for tr in trs],
               "tracked_on": [sum(bool(tr.pose_history[n]["tracked"]) for n in names) for tr in trs]}
        print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_render_ahead.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_render_ahead.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts:
        result["posed_call"] = part_a(dev)
        save()
    if "b" in args.parts:
        result["tracker_640x480"] = part_b(dev, args.frames)
        save()
    if "c" in args.parts:
        result["lockstep_640x480"] = part_c(dev, args.frames, args.objects)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
