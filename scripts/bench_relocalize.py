"""Relocaliser measurement (pixtrack_amd/relocalizer.py): one JSON line.

    python scripts/bench_relocalize.py [--width 640 --height 480 --trials 50 --seed 1]

* bank build: wall time (ends in a device synchronise) and bytes;
* per relocalisation: median of 20 after 5 warm-ups, from device events, split into the UNet pass, the scoring launch
  (+ device ranking) and the batched LM;
* the scoring kernel alone: median of 50 launches between device events, M, points, the algorithmic gather bytes
  (M x N x 4 taps x cstride x 4 B; the map is L2-resident) and their rate as a share of the 34.5 TB/s aggregate L2;
* the LM's recovery rate as a function of the initial in-plane error: share of seeded trials that converge (2e-2 rad,
  0.05 units) when the initial pose is the ground truth rolled by that error - with the nearest bank entry's features
  (what localize refines with; sets the roll spacing) and with the same view's upright features (one entry per view);
* recovery rate of ``localize`` over seeded lost-frame trials (a random mapping view, a random roll, up to 5 degrees /
  1 cm of perturbation).
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

L2_AGGREGATE_TBPS = 34.5  # MI355X: 8 XCDs x 4.3 TB/s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rolls", type=int, default=24)
    ap.add_argument("--top_k", type=int, default=8)
    ap.add_argument("--basin_trials", type=int, default=24, help="trials per initial error of the LM basin measurement")
    args = ap.parse_args(argv)

    from pixtrack_amd import _lib
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.ops import ops
    from pixtrack_amd.optimizer import PixTrackOptimizer
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.relocalizer import Relocalizer
    from pixtrack_amd.synthetic import make_tracking_assets, perturb_pose, render_query_frames
    from pixtrack_amd.unet import OUTPUT_DIMS
    from pixtrack_amd.utils.pose_utils import geodesic_distance_for_rotations

    dev = torch.device("cuda:0")
    assets = make_tracking_assets(seed=1300 + args.seed, width=args.width, height=args.height, n_frames=2)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    reloc = Relocalizer(tr.localizer, rolls=args.rolls, top_k=args.top_k, render=tr.get_reference_image)
    tr.relocalizer = reloc
    dbs = tr.localizer.model3d.dbs

    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    bank_bytes = reloc.build_bank()
    torch.cuda.synchronize(dev)
    bank_s = time.perf_counter() - t0

    rng = np.random.default_rng(args.seed)

    def rolled(R, t, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        return Rz @ R, Rz @ t

    def frames_at(poses, seed):
        a = dict(assets)
        a["gt_poses"] = poses
        return render_query_frames(a, tr.testbed, seed=seed, cold_start_indices=())

    def close(pose, R, t):
        Rp, tp = pose.numpy()
        rot = geodesic_distance_for_rotations(Rp, R)
        return rot < 2e-2 and float(np.linalg.norm(np.asarray(tp) - t)) < 0.05, rot

    # ---- lost-frame trials: a random view, a random roll, a small perturbation
    views = sorted(dbs)
    gts = []
    for _ in range(args.trials):
        v = int(rng.choice(views))
        R, t = rolled(dbs[v].qvec2rotmat(), dbs[v].tvec, float(rng.uniform(0, 360)))
        gts.append(perturb_pose(R, t, rng, float(rng.uniform(0, 5)), float(rng.uniform(0, 0.01)), assets["center"]))
    frames = frames_at(gts, seed=args.seed + 100)
    camera = tr.get_query_camera(frames[0])

    # ---- timing: 5 warm-ups, 20 timed (device events)
    reloc.timing = True
    times = []
    for i in range(25):
        reloc.localize(frames[i % len(frames)], camera)
        if i >= 5:
            times.append(reloc.timings_ms())
    med = {k: float(np.median([t[k] for t in times])) for k in times[0]}

    # ---- the scoring kernel alone
    reloc.timing = False
    lvl = reloc.score_level
    maps_q, scales_q = tr.localizer.refiner.dense_feature_extraction(frames[0], "bench", 1, None, True)
    cam_l = camera.scale(scales_q[lvl])
    p3d, fref, valid = reloc.bank
    M = reloc.n_static
    out = torch.empty(M, 4, device=dev)
    args_k = (maps_q[lvl], int(OUTPUT_DIMS[lvl]), [float(x) for x in cam_l.as10().tolist()], int(cam_l._data.shape[-1] - 6),
              p3d, fref, valid, reloc._poses_dev[:M], reloc._ranges_dev[:M], int(reloc.conf.pad), int(reloc.conf.loss),
              float(reloc.conf.loss_alpha), float(reloc.conf.loss_scale), out)
    for _ in range(5):
        ops.score_pose_hypotheses(*args_k)
    ks = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.score_pose_hypotheses(*args_k)
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1))
    score_ms = float(np.median(ks))
    n_scored = int(reloc._counts_dev[:M].sum().item())
    cs = int(fref.shape[1])
    gather_bytes = n_scored * 4 * cs * 4
    fmap = maps_q[lvl]

    # ---- recovery rate of localize
    ok = [close(reloc.localize(fr, camera).pose or Pose(torch.zeros(12)), R, t)[0] for fr, (R, t) in zip(frames, gts)]

    # ---- the LM's basin against the in-plane error: refine from the ground truth rolled by e, correct view's features
    refiner = tr.localizer.refiner
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=dev)
    bws = torch.empty(int(_lib.lib().pxt_lm_batch_workspace_bytes(1)), dtype=torch.uint8, device=dev)
    # two feature sources: the bank entry nearest to the ground truth (what localize refines with) and, for comparison,
    # the same view's UPRIGHT entry (roll 0: what a bank of one entry per view would hold)
    basin = {"nearest_entry": {}, "upright_view": {}}
    errs = (0.0, 5.0, 10.0, 15.0, 20.0, 30.0)
    per = max(1, args.basin_trials)
    for e in errs:
        hits = {"nearest_entry": 0, "upright_view": 0}
        for j in range(per):
            k = (j * 7 + int(e)) % len(gts)
            R, t = gts[k]
            near = reloc.nearest_view(R)
            Ri, ti = rolled(R, t, e if j % 2 == 0 else -e)
            maps, scs = refiner.dense_feature_extraction(frames[k], "basin", 1, None, True)
            for name, entry in (("nearest_entry", near), ("upright_view", near // reloc.rolls * reloc.rolls)):
                prob = refiner.lm_problem(maps, scs, camera, Pose.from_Rt(Ri, ti), reloc.views[entry].ref)
                prob["workspace"], prob["camera"] = ws, None
                res = PixTrackOptimizer.refine_levels_batch([prob], prob["conf"], bws, pool_key="basin")[0].result()
                hits[name] += (not res.failed) and close(res.T, R, t)[0]
        for name in hits:
            basin[name][f"{e:g}"] = round(hits[name] / per, 3)

    print(json.dumps({
        "workload": "relocalize", "width": args.width, "height": args.height, "views": reloc.n_views, "bank_entries": len(reloc.views),
        "rolls": reloc.rolls, "top_k": reloc.top_k, "bank_build_s": round(bank_s, 3), "bank_bytes": bank_bytes,
        "relocalize_ms_median": {k: round(v, 4) for k, v in med.items()},
        "score_kernel_ms_median": round(score_ms, 4), "hypotheses": M, "points_scored": n_scored,
        "points_per_hypothesis_mean": round(n_scored / M, 1), "query_map": list(fmap.shape),
        "gather_bytes": gather_bytes, "gather_TBps": round(gather_bytes / (score_ms * 1e-3) / 1e12, 3),
        "gather_share_of_l2": round(gather_bytes / (score_ms * 1e-3) / 1e12 / L2_AGGREGATE_TBPS, 4),
        "recovery_rate": round(sum(ok) / len(ok), 3), "trials": len(ok),
        "lm_recovery_by_initial_roll_error_deg": basin, "basin_trials_per_error": per,
        "targets": {"score_kernel_ms": 0.1, "relocalize_ms": 3.0},
    }))


if __name__ == "__main__":
    main()
