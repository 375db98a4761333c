"""Measurements of NeRF mesh extraction -> profiles/iso_surface.json.

  (a) device time of pxt_iso_surface_count (both launches) and pxt_iso_surface_emit (with normals) at 128^3 and 256^3, on
      a sphere lattice and on the synthetic NeRF's density lattice: HIP events around batches of calls with the host
      parked ahead of the stream, median of 7.  In the same process: a device-to-device float copy of the lattice's bytes.
  (b) density_lattice (pxt_ngp_query over the whole lattice, torch making the positions) at the same sizes: host clock
      around a call that ends in a synchronise, median of 5.
  (c) pxt_max_pairwise_distance at 16 k and 128 k points: pairs evaluated per second, and 9 lane-operations per pair
      (3 subtractions, 1 product, 2 multiply-adds, 1 compare, 2 selects) against the 78.65e12 lane-operations/s of the
      fp32 VALU.
  (d) extract_mesh end to end at 128^3 (lattice, border, extraction, components on the host, colours, diameter).

    python scripts/bench_iso_surface.py [--parts abcd] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd import mesh as M  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402

VALU_PEAK = 78.65e12  # lane-operations/s: the 157.3 TFLOPS vector fp32 peak with an FMA counted once
LANE_OPS_PER_PAIR = 9


def _time_launches(dev, launch, per=20, reps=7, warm=5):
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


def _testbed(dev):
    from pixtrack_amd.ngp import Testbed
    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, make_synthetic_nerf

    tb = Testbed(device=dev)
    tb.load_snapshot(make_synthetic_nerf())
    tb.snap_to_pixel_centers = True
    tb.render_aabb.min, tb.render_aabb.max = PREMIER_PROTEIN_AABB
    return tb


def _sphere(n, dev):
    ax = torch.arange(n, dtype=torch.float32, device=dev) - (n - 1) / 2
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.35 * n - torch.sqrt(x * x + y * y + z * z)).contiguous()


def _extract_times(dev, values, iso, origin, spacing):
    nz, ny, nx = (int(s) for s in values.shape)
    grid = M._grid7(iso, origin, spacing)
    ws = torch.empty(int(_lib.lib().pxt_iso_surface_workspace_bytes(nx, ny, nz)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.iso_surface_count(values, grid, ws, counts)
    n, m = counts.cpu().tolist()
    V = torch.empty(n, 3, dtype=torch.float32, device=dev)
    N = torch.empty(n, 3, dtype=torch.float32, device=dev)
    F = torch.empty(m, 3, dtype=torch.int32, device=dev)
    other = torch.empty_like(values)
    row = {"points": values.numel(), "lattice_bytes": values.numel() * 4, "vertices": n, "triangles": m,
           "workspace_bytes": ws.numel(),
           "count": _time_launches(dev, lambda: ops.iso_surface_count(values, grid, ws, counts)),
           "emit_with_normals": _time_launches(dev, lambda: ops.iso_surface_emit(values, grid, ws, V, N, F)),
           "emit": _time_launches(dev, lambda: ops.iso_surface_emit(values, grid, ws, V, None, F)),
           "float_copy_of_the_lattice": _time_launches(dev, lambda: other.copy_(values))}
    row["count_plus_emit_us"] = row["count"]["us_per_call_median"] + row["emit_with_normals"]["us_per_call_median"]
    row["ratio_to_copy"] = row["count_plus_emit_us"] / row["float_copy_of_the_lattice"]["us_per_call_median"]
    inv = M.mesh_invariants(V.cpu().numpy(), F.cpu().numpy())
    row["closed_and_oriented"] = inv["directed_edges_repeated"] == 0 and inv["directed_edges_unpaired"] == 0
    row["euler"] = inv["euler"]
    return row


def part_ab(dev, parts):
    tb = _testbed(dev)
    out = {"extract": [], "density_lattice": []}
    for n in (128, 256):
        if "b" in parts or "a" in parts:
            ts = []
            for _ in range(5):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                values, origin, spacing = M.density_lattice(tb, n)
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t0)
            row = {"resolution": n, "points": n ** 3, "seconds_median": float(np.median(ts[1:])), "seconds_first": ts[0],
                   "points_per_second": n ** 3 / float(np.median(ts[1:]))}
            out["density_lattice"].append(row)
            print(row, flush=True)
        if "a" in parts:
            closed = M.close_lattice_border(values, 2.5)
            for name, v, iso, o, s in (("sphere", _sphere(n, dev), 0.0, (0, 0, 0), (1, 1, 1)),
                                       ("synthetic_nerf", closed, 2.5, origin, spacing)):
                row = {"lattice": name, "resolution": n, **_extract_times(dev, v, iso, o, s)}
                out["extract"].append(row)
                print(row, flush=True)
    return out


def part_c(dev):
    rows = []
    rng = np.random.default_rng(0)
    for n in (16 * 1024, 128 * 1024):
        p = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).to(dev)
        ws = torch.empty(int(_lib.lib().pxt_max_pairwise_distance_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        rec = torch.zeros(4, dtype=torch.int32, device=dev)
        t = _time_launches(dev, lambda: ops.max_pairwise_distance(p, rec, ws), per=5 if n > 50000 else 20)
        tiles = (n + 1023) // 1024
        evaluated = 1024 * 1024 * tiles * (tiles + 1) // 2  # every workgroup walks its own tile and the later ones
        rate = evaluated / (t["us_per_call_median"] * 1e-6)
        row = {"n": n, "pairs": n * (n - 1) // 2, "pairs_evaluated": evaluated, **t, "pairs_evaluated_per_second": rate,
               "lane_ops_per_second": rate * LANE_OPS_PER_PAIR, "of_fp32_valu_peak": rate * LANE_OPS_PER_PAIR / VALU_PEAK,
               "result": M.max_pairwise_distance(p)}
        rows.append(row)
        print(row, flush=True)
    return rows


def part_d(dev):
    tb = _testbed(dev)
    ts, last = [], None
    for _ in range(4):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        last = M.extract_mesh(tb, 128)
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    row = {"resolution": 128, "seconds_first": ts[0], "seconds_median": float(np.median(ts[1:])), "times_last": last["times"],
           "vertices": int(len(last["V"])), "triangles": int(len(last["F"])), "n_components": last["n_components"],
           "diameter": last["diameter"], "invariants": last["invariants"]}
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "iso_surface.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1))

    if "a" in args.parts or "b" in args.parts:
        result.update(part_ab(dev, args.parts))
        save()
    if "c" in args.parts:
        result["max_pairwise_distance"] = part_c(dev)
        save()
    if "d" in args.parts:
        result["extract_mesh"] = part_d(dev)
        save()
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
