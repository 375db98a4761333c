"""The relocaliser's depth stage, measured (pixtrack_amd/relocalizer.py): one JSON line.

    python scripts/bench_relocalize_depth.py [--width 640 --height 480 --trials 12 --rolls 24 --seed 1]

One process, a mesh-template tracker with relocalizer="mesh" and the default RelocDepth on make_mesh_tracking_assets'
object:
* per distance factor (0.5 .. 2 times the mapping distance): seeded trials - a random mapping view, a random roll, up to
  5 degrees / 1 cm of perturbation, the object's centre moved to a random pixel of the middle half of the image and to
  the factor's depth; the sensor frame is the mesh's own depth there, 0 off the object.  Reported: the recall of the
  right bank ENTRY (the one nearest to the ground truth by rotation) among the depth stage's best n_geometric, the rank
  of its best placement, and the end-to-end recovery (2e-2 rad, 0.05 units) with the stage and without it;
* the depth launch alone on the full placement grid: median, minimum and maximum of ``--runs`` launches between device
  events after 5 warm-ups; the feature scorer on a SAMPLE of the same hypotheses (``--sample`` of them, evenly spaced),
  timed the same way and scaled to all of them - it is not run on all: that is the point of the stage;
* the whole localize with the stage, split by device events.
Numbers at a toy size measure overheads: the defaults are the sizes a user would run."""
from __future__ import annotations

import argparse
import json
import math
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SENSOR_SCALE = 2e-4  # SfM units per count: the object sits up to ~8 units away at factor 2


def timed(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": runs}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--trials", type=int, default=12, help="trials per distance factor")
    ap.add_argument("--rolls", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=20, help="timed launches per kernel (>= 5)")
    ap.add_argument("--sample", type=int, default=4096, help="hypotheses the feature scorer is timed on")
    ap.add_argument("--factors", type=float, nargs="+", default=[0.5, 0.71, 1.0, 1.41, 2.0])
    args = ap.parse_args(argv)
    if args.runs < 5:
        ap.error("--runs >= 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_relocalize_depth needs a ROCm device: nothing is measured without one")

    from pixtrack_amd import mesh_render as R
    from pixtrack_amd import relocalizer as RL
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.ops import ops
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_mesh_tracking_assets, perturb_pose, render_mesh_query_frames
    from pixtrack_amd.unet import OUTPUT_DIMS
    from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

    dev = torch.device("cuda:0")
    W, H = args.width, args.height
    tmp = tempfile.TemporaryDirectory()  # (the reference model's directory: removed when the process ends)
    assets = make_mesh_tracking_assets(seed=1030 + args.seed, width=W, height=H, n_frames=2, out_dir=tmp.name, device=dev)
    V, F = assets["mesh"][:2]
    renderer = R.MeshRenderer(V, F, dev, **assets["mesh_shading"])
    sensors = {}
    depth = RL.RelocDepth(lookup=sensors.get, sensor_depth_scale=SENSOR_SCALE)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, template=MeshTemplate(renderer, supersample=2),
                             assets={k: assets[k] for k in ("model3d", "weights", "covis", "upright_ref_img")},
                             relocalizer="mesh", reloc_depth=depth, reloc_options=dict(rolls=args.rolls))
    reloc = tr.relocalizer
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    bank_bytes = reloc.build_bank()
    torch.cuda.synchronize(dev)
    bank_s = time.perf_counter() - t0

    dbs = tr.localizer.model3d.dbs
    camera = Camera.from_colmap(assets["query_camera"])
    cam10 = [float(x) for x in camera.as10().tolist()]
    fx, fy, cx, cy = cam10[2:6]
    rng = np.random.default_rng(args.seed)

    def rolled(Rv, tv, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        return Rz @ Rv, Rz @ tv

    def sensor_at(pose):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = pose
        g = renderer.render_frame([(R.view_record(camera, T), W, H, 1, ("depth",))], download_records=False)[0]["depth"].cpu().numpy()
        z = np.where(g[..., 3] > 0, g[..., 0], 0.0)
        return np.rint(np.minimum(z / SENSOR_SCALE, 65535)).astype(np.uint16)

    def close(pose, Rg, tg):
        if pose is None:
            return False
        Rp, tp = pose.numpy()
        return bool(geodesic_distance_for_rotations(Rp, Rg) < 2e-2 and float(np.linalg.norm(np.asarray(tp) - tg)) < 0.05)

    per = 1 + len(depth.distances) * depth.grid[0] * depth.grid[1]
    by_factor = {}
    views = sorted(dbs)
    for s in args.factors:
        gts = []
        for _ in range(args.trials):
            v = int(rng.choice(views))
            Rg, tg = rolled(dbs[v].qvec2rotmat(), dbs[v].tvec, float(rng.uniform(0, 360)))
            Rg, tg = perturb_pose(Rg, tg, rng, float(rng.uniform(0, 5)), float(rng.uniform(0, 0.01)), assets["center"])
            c = Rg @ assets["center"] + tg
            px, py = rng.uniform(0.25 * W, 0.75 * W), rng.uniform(0.25 * H, 0.75 * H)
            z = s * c[2]
            gts.append((Rg, tg + np.array([z * (px - cx) / fx, z * (py - cy) / fy, z]) - c))
        a = dict(assets)
        a["gt_poses"] = gts
        frames = render_mesh_query_frames(a, renderer, seed=args.seed + 100, cold_start_indices=())
        hit, ranks, ok_depth, ok_plain = 0, [], 0, 0
        for (Rg, tg), fr in zip(gts, frames):
            plane = torch.from_numpy(sensor_at((Rg, tg)).view(np.int16)).to(dev)
            res = reloc.localize(fr, camera, sensor=plane)
            kept_entries = (reloc.last_geometric.cpu().numpy() // per)
            where = np.nonzero(kept_entries == reloc.nearest_view(Rg))[0]
            hit += len(where) > 0
            ranks.append(int(where[0]) if len(where) else None)
            ok_depth += close(res.pose, Rg, tg)
            ok_plain += close(reloc.localize(fr, camera).pose, Rg, tg)
        by_factor[f"{s:g}"] = {"entry_recall": round(hit / len(gts), 3), "entry_best_rank": ranks,
                               "recovered_with_depth": round(ok_depth / len(gts), 3),
                               "recovered_without": round(ok_plain / len(gts), 3), "trials": len(gts)}

    # ---- the two scoring kernels on the placement grid
    reloc._placements(cam10)
    Mp = reloc.n_placed
    p3d_d, valid_d = reloc.depth_bank
    depth_launch = lambda: RL.score_hypotheses_depth(p3d_d, valid_d, reloc._place_poses_dev, reloc._place_depth_ranges, plane,
                                                     SENSOR_SCALE, reloc.depth_tolerance, camera, out=reloc._place_out)
    t_depth = timed(depth_launch, args.runs)
    n_depth_points = int(reloc._place_depth_ranges[:, 1].sum().item())
    lvl = reloc.score_level
    maps_q, scales_q = tr.localizer.refiner.dense_feature_extraction(frames[0], "bench", 1, None, True)
    cam_l = camera.scale(scales_q[lvl])
    p3d, fref, valid = reloc.bank
    n_sample = min(args.sample, Mp)
    pick = torch.linspace(0, Mp - 1, n_sample, device=dev).long()
    s_poses = reloc._place_poses_dev.index_select(0, pick).contiguous()
    s_ranges = reloc._place_feat_ranges.index_select(0, pick).contiguous()
    s_out = torch.empty(n_sample, 4, device=dev)
    feature_launch = lambda: ops.score_pose_hypotheses(
        maps_q[lvl], int(OUTPUT_DIMS[lvl]), [float(x) for x in cam_l.as10().tolist()], int(cam_l._data.shape[-1] - 6), p3d, fref,
        valid, s_poses, s_ranges, int(reloc.conf.pad), int(reloc.conf.loss), float(reloc.conf.loss_alpha),
        float(reloc.conf.loss_scale), s_out)
    t_feat = timed(feature_launch, args.runs)
    n_feat_points = int(s_ranges[:, 1].sum().item())
    feat_scaled_ms = t_feat["median_ms"] * Mp / n_sample

    # ---- the whole localize with the stage
    reloc.timing = True
    split = []
    for i in range(5 + args.runs):
        reloc.localize(frames[i % len(frames)], camera, sensor=plane)
        if i >= 5:
            split.append(reloc.timings_ms())
    reloc.timing = False
    med = {k: round(float(np.median([t[k] for t in split])), 4) for k in split[0]}

    print(json.dumps({
        "workload": "relocalize_depth", "width": W, "height": H, "views": reloc.n_views, "bank_entries": len(reloc.views),
        "rolls": reloc.rolls, "grid": list(depth.grid), "distances": list(depth.distances), "placements": Mp,
        "n_geometric": reloc.n_geometric, "depth_points_per_entry": depth.depth_points, "bank_build_s": round(bank_s, 3),
        "bank_bytes": bank_bytes, "by_distance_factor": by_factor,
        "depth_kernel": {**t_depth, "points": n_depth_points, "bytes_per_point": 14,
                         "GBps": round(n_depth_points * 14 / (t_depth["median_ms"] * 1e-3) / 1e9, 1)},
        "feature_kernel_sample": {**t_feat, "hypotheses": n_sample, "points": n_feat_points,
                                  "scaled_to_all_placements_ms": round(feat_scaled_ms, 2)},
        "feature_over_depth": round(feat_scaled_ms / t_depth["median_ms"], 1),
        "per_hypothesis_us": {"depth": round(1e3 * t_depth["median_ms"] / Mp, 5), "feature": round(1e3 * t_feat["median_ms"] / n_sample, 4)},
        "localize_with_depth_ms_median": med,
    }))


if __name__ == "__main__":
    main()
