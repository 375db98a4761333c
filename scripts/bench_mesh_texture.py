"""Measurements of the textured render (pxt_mesh_render_textured) -> profiles/mesh_texture.json.

640 x 480, calls of 8 views and of 1 view, writing rgb_u8 + depth_nz (what the tracker takes from a renderer per frame),
on two meshes of scripts/bench_mesh_render.py with the same views: the 12-triangle box that fills the image and the
icosphere of 81 920 triangles.  In one process, HIP events around batches of 20 calls with the host parked ahead of the
stream (bench_mesh_raster._time_launches), median of 7:

  colour          pxt_mesh_render with seeded vertex colours (the call of profiles/mesh_render.json's "tracker" rows)
  textured_2048   pxt_mesh_render_textured, a 2048 x 2048 map (16 MiB of texels: the gathers leave the caches)
  textured_64     the same UVs on a 64 x 64 map (16 KiB: the gathers stay in cache; what is left is the arithmetic)

UVs: one per vertex, the vertex's x, y over the bounding box (a planar projection: neighbouring pixels read neighbouring
texels, as on a model with a sensible atlas).  For each variant a device-to-device copy of the bytes the call must move:
the key plane cleared and read back (16 B per pixel and view), the outputs, vertices, indices and, for the textured
calls, the UVs, UV indices and four texels per covered pixel at most once per texel of the map - a copy of half that
size, since a copy reads and writes its size.  The colour rows carry the parent's figure from profiles/mesh_render.json
beside them when that file is there.

    python scripts/bench_mesh_texture.py [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import bench_mesh_raster as B  # noqa: E402
from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import mesh_render as R  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402

W, H = B.W, B.H
TEXTURES = {"textured_2048": 2048, "textured_64": 64}


def _parent_rows():
    path = ROOT / "profiles" / "mesh_render.json"
    if not path.is_file():
        return {}
    return {r["mesh"]: r for r in json.loads(path.read_text())["render"]}


def _row(dev, name, V, F, views, parent):
    rng = np.random.default_rng(0)
    C = rng.uniform(0.0, 1.0, size=(len(V), 3)).astype(np.float32)
    lo, hi = V.min(0), V.max(0)
    UV = ((V[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    colour = R.MeshRenderer(V, F, dev, colors=C)
    textured = {k: R.MeshRenderer(V, F, dev, uvs=UV, texture=rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8))
                for k, n in TEXTURES.items()}
    row = {"mesh": name, "vertices": colour.n_vertices, "triangles": colour.n_triangles, "width": W, "height": H}
    rec = colour.render(views[:1], W, H)["records"]
    covered = int(rec[0, R.W_COVERED])
    row["covered_fraction"] = covered / (W * H)
    for P in (8, 1):
        v = torch.from_numpy(np.ascontiguousarray(views[:P])).to(dev)
        u8 = torch.empty(P, H, W, 3, dtype=torch.uint8, device=dev)
        nz = torch.empty(P, H, W, dtype=torch.uint8, device=dev)
        records = torch.empty(P, R.RECORD, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, colour.n_triangles, W, H)), dtype=torch.uint8,
                         device=dev)
        r = colour
        launches = {"colour": lambda: ops.mesh_render(r.vertices, r.triangles, r.colors, v, W, H, None, u8, None, nz, None,
                                                      records, ws)}
        base = P * (W * H * (16 + 4) + r.n_triangles * 12 + r.n_vertices * 12)
        moved = {"colour": base + P * r.n_vertices * 12}
        for k, t in textured.items():
            launches[k] = (lambda t: lambda: ops.mesh_render_textured(t.vertices, t.triangles, t.uvs, t.triangle_uvs, t.texture,
                                                                      v, W, H, None, u8, None, nz, None, records, ws))(t)
            texels = min(4 * covered, TEXTURES[k] ** 2)
            moved[k] = base + P * (r.n_vertices * 8 + r.n_triangles * 12 + texels * 4)
        res = {}
        for key, launch in launches.items():
            src = torch.empty(moved[key] // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            t = B._time_launches(dev, launch)
            c = B._time_launches(dev, lambda: dst.copy_(src))
            res[key] = {**t, "us_per_view": t["us_per_call_median"] / P, "bytes_moved_per_call": moved[key],
                        "copy_us_per_call_median": c["us_per_call_median"],
                        "ratio_to_copy": t["us_per_call_median"] / c["us_per_call_median"]}
        for key in res:
            res[key]["ratio_to_colour"] = res[key]["us_per_call_median"] / res["colour"]["us_per_call_median"]
        res["textured_2048_over_64"] = res["textured_2048"]["us_per_call_median"] / res["textured_64"]["us_per_call_median"]
        was = parent.get(name, {}).get(f"views_{P}", {}).get("tracker")
        if was:
            res["colour"]["parent_us_per_call_median"] = was["us_per_call_median"]
            res["colour"]["parent_us_min_max"] = [was["us_min"], was["us_max"]]
            res["colour"]["ratio_to_parent"] = res["colour"]["us_per_call_median"] / was["us_per_call_median"]
        row[f"views_{P}"] = res
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_texture.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.PxtError("the measurement needs a ROCm device")
    dev = torch.device("cuda:0")
    parent = _parent_rows()
    eye = np.eye(3)
    rows = []
    V, F = B._box()
    outside = np.stack([R.pack_view(eye, (0.01 * k, 0.0, 2.2), 500.0, 500.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_row(dev, "12-triangle box whose front face fills the image", V, F, outside, parent))
    V, F = R.icosphere(6)
    sphere = np.stack([R.pack_view(eye, (0.0, 0.0, 2.6 + 0.01 * k), 600.0, 600.0, 319.5, 239.5, 1e-6, 1.0) for k in range(8)])
    rows.append(_row(dev, "icosphere of 81920 triangles", V, F, sphere, parent))
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({"texture": rows}, indent=1))
    print(json.dumps({"rows": len(rows), "out": str(path)}))


if __name__ == "__main__":
    main()
