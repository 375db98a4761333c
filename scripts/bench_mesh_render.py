"""Measurements of the colour render (pxt_mesh_render) -> profiles/mesh_render.json.

640 x 480, calls of 8 views and of 1 view, the meshes of scripts/bench_mesh_raster.py (the 128^3 mesh of the synthetic
NeRF, the 12-triangle box that fills the image, the icosphere of 81 920 triangles) with seeded vertex colours.  In one
process, HIP events around batches of 20 calls with the host parked ahead of the stream
(bench_mesh_raster._time_launches), median of 7:

  depth       pxt_mesh_raster, depth only (the parent's four launches, unchanged)
  tracker     pxt_mesh_render -> rgb_u8 + depth_nz (what the tracker takes from a renderer per frame)
  tracker+d   ... + the float depth image
  all         rgba, rgb_u8, depth, depth_nz, ids

and for each a device-to-device copy of the bytes the variant must move per call: the key plane cleared (8 B per pixel
and view) and read back (8 B), the outputs written, vertices (12 B each; 24 B with colours) and indices (12 B per
triangle) read once per view - a copy of half that size, since a copy reads and writes its size.

    python scripts/bench_mesh_render.py [--out FILE] [--skip_nerf]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import bench_mesh_raster as B  # noqa: E402
from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import mesh as M  # noqa: E402
from pixtrack_amd import mesh_evaluation as ME  # noqa: E402
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402

W, H = B.W, B.H
OUT_BYTES = {"rgba": 16, "rgb_u8": 3, "depth": 16, "depth_nz": 1, "ids": 4}
VARIANTS = {"depth": ("depth",), "tracker": ("rgb_u8", "depth_nz"), "tracker+d": ("rgb_u8", "depth_nz", "depth"),
            "all": ("rgba", "rgb_u8", "depth", "depth_nz", "ids")}


def _row(dev, name, V, F, views):
    C = np.random.default_rng(0).uniform(0.0, 1.0, size=(len(V), 3)).astype(np.float32)
    r = R.MeshRenderer(V, F, dev, colors=C)
    row = {"mesh": name, "vertices": r.n_vertices, "triangles": r.n_triangles, "width": W, "height": H}
    rec = r.render(views[:1], W, H)["records"]
    row["covered_fraction"] = float(rec[0, R.W_COVERED]) / (W * H)
    for P in (8, 1):
        v = torch.from_numpy(np.ascontiguousarray(views[:P])).to(dev)
        bufs = {"rgba": torch.empty(P, H, W, 4, device=dev), "rgb_u8": torch.empty(P, H, W, 3, dtype=torch.uint8, device=dev),
                "depth": torch.empty(P, H, W, 4, device=dev), "depth_nz": torch.empty(P, H, W, dtype=torch.uint8, device=dev),
                "ids": torch.empty(P, H, W, dtype=torch.int32, device=dev)}
        records = torch.empty(P, R.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, r.n_triangles, W, H)), dtype=torch.uint8, device=dev)

        def launch(names):
            if names == ("depth",):
                return lambda: ops.mesh_raster(r.vertices, r.triangles, v, bufs["depth"], None, records, ws)
            a = [bufs[k] if k in names else None for k in ("rgba", "rgb_u8", "depth", "depth_nz", "ids")]
            return lambda: ops.mesh_render(r.vertices, r.triangles, r.colors, v, W, H, *a, records, ws)

        res = {}
        for key, names in VARIANTS.items():
            moved = P * (W * H * (16 + sum(OUT_BYTES[k] for k in names)) + r.n_triangles * 12
                         + r.n_vertices * (12 if key == "depth" else 24))
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            t = B._time_launches(dev, launch(names))
            c = B._time_launches(dev, lambda: dst.copy_(src))
            res[key] = {**t, "us_per_view": t["us_per_call_median"] / P, "bytes_moved_per_call": moved,
                        "copy_us_per_call_median": c["us_per_call_median"],
                        "ratio_to_copy": t["us_per_call_median"] / c["us_per_call_median"]}
        for key in res:
            res[key]["ratio_to_depth"] = res[key]["us_per_call_median"] / res["depth"]["us_per_call_median"]
        row[f"views_{P}"] = res
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_render.json"))
    ap.add_argument("--skip_nerf", action="store_true", help="leave out the mesh extracted from the synthetic NeRF")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.PxtError("the measurement needs a ROCm device")
    dev = torch.device("cuda:0")
    rows = []
    if not args.skip_nerf:
        with tempfile.TemporaryDirectory() as tmp:
            _, testbed, _ = B._object(dev, tmp, 2)
            mesh = M.extract_mesh(testbed, 128, colors=False)
            lo, hi = np.asarray(testbed.render_aabb.min), np.asarray(testbed.render_aabb.max)
            centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
            focal = 0.5 * W / np.tan(np.radians(20.0))
            cams = ME.look_at_cameras(centre, 1.05 * radius / np.sin(np.arctan(0.5 * H / focal)), 8)
            views = np.stack([R.ngp_view_record(C, focal, W, H) for C in cams])
            rows.append(_row(dev, "synthetic NeRF at 128^3", mesh["V"], mesh["F"], views))
    eye = np.eye(3)
    V, F = B._box()
    outside = np.stack([R.pack_view(eye, (0.01 * k, 0.0, 2.2), 500.0, 500.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_row(dev, "12-triangle box whose front face fills the image", V, F, outside))
    V, F = R.icosphere(6)
    sphere = np.stack([R.pack_view(eye, (0.0, 0.0, 2.6 + 0.01 * k), 600.0, 600.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_row(dev, "icosphere of 81920 triangles", V, F, sphere))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({"render": rows}, indent=1))
    print(json.dumps({"rows": len(rows), "out": str(path)}))


if __name__ == "__main__":
    main()
