"""Measurements of the mesh template -> profiles/mesh_template.json.

  (a) device time of one pxt_mesh_render_frame call at the tracker's shapes - a 640 x 480 depth_nz plane at the query
      camera plus a 640 x 480 or a 960 x 720 rgb_u8 image at the reference camera, supersample 1, 2 and 4, vertex
      colours and a 2048 x 2048 texture map, the synthetic mesh object at 81 920 triangles - against what the same
      planes cost without the call, in the same process: one pxt_mesh_render(_textured) call for depth_nz, one for the
      float colour image at the fine size, avg_pool2d, and the 8-bit conversion (pxt_rgba_to_u8).  HIP events around
      batches of calls with the host parked ahead of the stream; the sides alternate, five repeats each.  The
      criterion: the frame call's median is not above the composition's median plus the composition's own spread
      (max - min) over its five repeats.  The outputs of the two sides are compared first.  Where supersample is 1 and
      the two cameras agree the existing call can write both planes at once; that single call is timed beside the two
      (``single_call_*``: recorded, the harder comparison, with the same allowance rule).
  (b) the r9 tracker with the template on the synthetic mesh object at 640 x 480: frames per second by the host clock
      around the frame loop (ends in a device synchronise), and the device time of the frame's render call at the
      tracker's own requests.  Recorded only: the NeRF tracker's scene is another one.

    python scripts/bench_mesh_template.py [--parts ab] [--frames 100] [--out FILE]
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

QW, QH = 640, 480


def _batch_us(dev, launch, per=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
    e0.record()
    for _ in range(per):
        launch()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / per


def _alternate(dev, sides, repeats=5, warm=3):
    """{name: launch} -> {name: [us per call] x repeats}, the sides taking turns."""
    for launch in sides.values():
        for _ in range(warm):
            launch()
    torch.cuda.synchronize(dev)
    us = {name: [] for name in sides}
    for _ in range(repeats):
        for name, launch in sides.items():
            us[name].append(_batch_us(dev, launch))
    return us


class _Frame:
    """One frame call with its buffers allocated once (what MeshRenderer.render_frame does per call, without the
    allocations)."""

    def __init__(self, r, requests):
        self.r = r
        self.geometry, self.offsets, sizes = [], [], [0, 0, 0, 0]
        for _, W, H, S, want in requests:
            self.geometry += [W, H, S]
            for k, (name, px) in enumerate(zip(R.FRAME_OUTPUTS, (16, 3, 16, 1))):
                self.offsets.append(sizes[k] if name in want else -1)
                sizes[k] += (W * H * px + 15) // 16 * 16 if name in want else 0
        dev = r.device
        self.bufs = [None if n == 0 else torch.empty(n // (4 if k in (0, 2) else 1), dtype=torch.float32 if k in (0, 2) else torch.uint8,
                                                     device=dev) for k, n in enumerate(sizes)]
        self.views = torch.from_numpy(np.stack([q[0] for q in requests])).to(dev)
        self.records = torch.empty(len(requests), R.RECORD, dtype=torch.int32, device=dev)
        need = int(_lib.lib().pxt_mesh_render_frame_workspace_bytes(len(requests), r.n_triangles,
                                                                    (_lib.C.c_int32 * len(self.geometry))(*self.geometry)))
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.requests = requests

    def __call__(self):
        r = self.r
        ops.mesh_render_frame(r.vertices, r.triangles, r.colors, r.uvs, r.triangle_uvs, r.texture, self.views, self.geometry,
                              self.offsets, *self.bufs, self.records, self.ws)

    def plane(self, p, name):
        k = R.FRAME_OUTPUTS.index(name)
        _, W, H, _, _ = self.requests[p]
        ch, o = (4, 3, 4, 1)[k], self.offsets[4 * p + k]
        e = (16, 3, 16, 1)[k] // ch
        return self.bufs[k][o // e:o // e + W * H * ch].view(H, W, ch)


class _Composition:
    """The same planes from the existing calls: depth_nz from one call; the colour image from one call at the fine size,
    avg_pool2d and pxt_rgba_to_u8 - or, with ``fused``, one existing call for both planes (supersample 1, one camera)."""

    def __init__(self, r, vq, vr, RW, RH, S, fused):
        dev = r.device
        self.r, self.S, self.fused, self.RW, self.RH = r, S, fused, RW, RH
        self.vq = torch.from_numpy(vq[None]).to(dev)
        self.vf = torch.from_numpy(R.supersampled_view(vr, S)[None]).to(dev)
        self.nz = torch.empty(1, QH, QW, dtype=torch.uint8, device=dev)
        self.u8 = torch.empty(RH, RW, 3, dtype=torch.uint8, device=dev)
        self.rgba = torch.empty(1, RH * S, RW * S, 4, dtype=torch.float32, device=dev)
        self.rec = torch.empty(1, R.RECORD, dtype=torch.int32, device=dev)
        L = _lib.lib()
        self.ws_q = torch.empty(int(L.pxt_mesh_raster_workspace_bytes(1, r.n_triangles, QW, QH)), dtype=torch.uint8, device=dev)
        self.ws_f = torch.empty(int(L.pxt_mesh_raster_workspace_bytes(1, r.n_triangles, RW * S, RH * S)), dtype=torch.uint8, device=dev)

    def _render(self, views, W, H, rgba, u8, nz, ws):
        r = self.r
        if r.texture is None:
            ops.mesh_render(r.vertices, r.triangles, r.colors, views, W, H, rgba, u8, None, nz, None, self.rec, ws)
        else:
            ops.mesh_render_textured(r.vertices, r.triangles, r.uvs, r.triangle_uvs, r.texture, views, W, H, rgba, u8, None, nz,
                                     None, self.rec, ws)

    def __call__(self):
        if self.fused:
            self._render(self.vq, QW, QH, None, self.u8.view(1, QH, QW, 3), self.nz, self.ws_q)
            return
        self._render(self.vq, QW, QH, None, None, self.nz, self.ws_q)
        self._render(self.vf, self.RW * self.S, self.RH * self.S, self.rgba, None, None, self.ws_f)
        img = self.rgba[0]
        if self.S > 1:
            img = torch.nn.functional.avg_pool2d(img.permute(2, 0, 1)[None], self.S)[0].permute(1, 2, 0).contiguous()
        ops.rgba_to_u8(img, 0.0, self.u8)


def _bench_mesh(subdivisions=6):
    from pixtrack_amd.synthetic import make_bumpy_mesh

    V, F, UV, FUV, tex = make_bumpy_mesh(1012, subdivisions, texture_size=(2048, 2048), texture_sigma=12.0)
    C = np.clip(0.5 + 0.5 * V / np.abs(V).max(), 0.0, 1.0).astype(np.float32)
    return V, F, C, dict(uvs=UV, triangle_uvs=FUV, texture=tex)


def _pose(V, f, size_px):
    """The object in front of the camera, its largest extent ``size_px`` pixels: (R, t)."""
    lo, hi = V.min(0), V.max(0)
    a = np.deg2rad(25.0)
    Rm = np.asarray([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
    return Rm, -Rm @ (0.5 * (lo + hi)) + np.asarray([0.0, 0.0, f * float((hi - lo).max()) / size_px])


def part_a(dev):
    V, F, C, textured = _bench_mesh()
    rows = []
    f_q = 1.2 * QW
    Rm, t = _pose(V, f_q, 0.75 * QH)
    for shading, kw in (("vertex colours", dict(colors=C)), ("texture 2048 x 2048", textured)):
        r = R.MeshRenderer(V, F, dev, **kw)
        for RW, RH in ((640, 480), (960, 720)):
            f_r = f_q * RW / QW
            vq = R.pack_view(Rm, t, f_q, f_q, QW / 2 - 0.5, QH / 2 - 0.5, 1e-6, 1.0 / (2.0 * t[2]))
            vr = R.pack_view(Rm, t, f_r, f_r, RW / 2 - 0.5, RH / 2 - 0.5, 1e-6, 1.0 / (2.0 * t[2]))
            for S in (1, 2, 4):
                fused = S == 1 and (RW, RH) == (QW, QH)
                requests = [(vq, QW, QH, 1, ("depth_nz", "rgb_u8"))] if fused else \
                    [(vq, QW, QH, 1, ("depth_nz",)), (vr, RW, RH, S, ("rgb_u8",))]
                frame, comp = _Frame(r, requests), _Composition(r, vq, vr, RW, RH, S, False)
                sides = {"frame": frame, "composition": comp}
                if fused:
                    sides["single_call"] = _Composition(r, vq, vr, RW, RH, S, True)
                for side in sides.values():
                    side()
                torch.cuda.synchronize(dev)
                du8 = (frame.plane(len(requests) - 1, "rgb_u8").int() - comp.u8.int()).abs()
                nz_equal = bool(torch.equal(frame.plane(0, "depth_nz")[..., 0], comp.nz[0]))
                us = _alternate(dev, sides)
                fm, cm = float(np.median(us["frame"])), float(np.median(us["composition"]))
                spread = float(max(us["composition"]) - min(us["composition"]))
                row = {"shading": shading, "triangles": r.n_triangles, "query": [QW, QH], "reference": [RW, RH], "supersample": S,
                       "views": len(requests), "frame_us": us["frame"], "composition_us": us["composition"],
                       "frame_us_median": fm, "composition_us_median": cm, "composition_spread_us": spread,
                       "criterion_met": bool(fm <= cm + spread), "ratio": fm / cm, "depth_nz_equal": nz_equal,
                       "rgb_u8_max_abs_difference": int(du8.max()), "rgb_u8_pixels_differing": int((du8.amax(-1) > 0).sum()),
                       "covered_fraction_query": float(frame.records[0, R.W_COVERED].item()) / (QW * QH)}
                if fused:
                    one = sides["single_call"]
                    sm, ss = float(np.median(us["single_call"])), float(max(us["single_call"]) - min(us["single_call"]))
                    row.update({"single_call_us": us["single_call"], "single_call_us_median": sm, "single_call_spread_us": ss,
                                "single_call_not_slower": bool(fm <= sm + ss),
                                "single_call_outputs_equal": bool(torch.equal(one.u8, comp.u8) and torch.equal(one.nz, comp.nz))})
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def part_b(dev, n_frames):
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, render_mesh_query_frames
    from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        assets = make_mesh_tracking_assets(width=QW, height=QH, n_frames=n_frames, out_dir=tmp, device=dev)
        V, F = assets["mesh"][:2]
        frames = render_mesh_query_frames(assets, R.MeshRenderer(V, F, dev, **assets["mesh_shading"]))
        for S in (1, 2, 4):
            template = MeshTemplate(R.MeshRenderer(V, F, dev, **assets["mesh_shading"]), supersample=S)
            tr = PixLocPoseTrackerR9("", "", "", tmp, debug=0, device=dev, template=template,
                                     assets={k: assets[k] for k in ("model3d", "weights", "covis", "upright_ref_img")})
            warm = 10
            for i in range(warm):
                tr.run_single_frame((f"{i:06d}.png", frames[i]))
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n_frames):
                tr.run_single_frame((f"{i:06d}.png", frames[i]))
            torch.cuda.synchronize(dev)
            seconds = time.perf_counter() - t0
            errs = []
            for i in range(n_frames):
                Rt, tt = tr.pose_history[f"{i:06d}.png"]["T_refined"].numpy()
                Rg, tg = assets["gt_poses"][i]
                errs.append((float(geodesic_distance_for_rotations(Rt, Rg)), float(np.linalg.norm(tt - tg))))
            tracked = sum(bool(h["tracked"]) for h in tr.pose_history.values())
            call = _Frame(template.renderer, template.requests(tr.pose, tr.camera, tr._reference_camera()))
            us = _alternate(dev, {"frame": call})["frame"]
            row = {"supersample": S, "frames_timed": n_frames - warm, "frames_per_second": (n_frames - warm) / seconds,
                   "ms_per_frame": 1e3 * seconds / (n_frames - warm), "tracked": tracked, "frames": n_frames,
                   "rotation_error_max_rad": max(e[0] for e in errs), "translation_error_max": max(e[1] for e in errs),
                   "cost_mean": float(np.mean([h["cost"] for h in tr.pose_history.values()])),
                   "render_call_us": us, "render_call_us_median": float(np.median(us)), "render_views": len(call.requests),
                   "triangles": int(len(F)), "nerf_render_ms_documented": 0.68}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_template.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_template.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts:
        result["frame_call"] = part_a(dev)
        save()
    if "b" in args.parts:
        result["tracker_640x480"] = part_b(dev, args.frames)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
