"""Measurements of the opt-in pose information -> profiles/r08_pose_uncertainty.json.

  (a) launch time of pxt_lm_information: HIP events around batches of launches, host parked ahead of the stream;
      N = 2048 / 10000, C = 32 / 128, 1 / 24 problems per launch; achieved TB/s of the bytes a launch must move
      (SURVEY 8d accounting: per valid point 12 footprint texels + 1 reference record of cstride floats, 3 floats p3d).
  (b) tracked frames/s with the option off and on, same process, same scene, alternating three times:
      the r9 tracker (640x480, 200 frames) and the eight-object lock-step tracker.
  (c) calibration: seeded Gaussian noise on the query maps of a make_lm_scene scene, 64 refinements from the ground
      truth; per eigen-direction of the predicted covariance the ratio empirical / predicted variance.
  (d) the two documented tracks (bottle, roncelli_blankk of objects8, 65 frames): condition, weakest direction and
      rotation error per frame.

    python scripts/bench_pose_uncertainty.py [--parts abcd] [--frames 200]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import _lib, parallel  # noqa: E402
from pixtrack_amd.geometry import Pose  # noqa: E402
from pixtrack_amd.ops import ops  # noqa: E402
from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for  # noqa: E402
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker  # noqa: E402
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9  # noqa: E402
from pixtrack_amd.synthetic import make_lm_scene, make_tracking_assets, render_query_frames  # noqa: E402
from pixtrack_amd.uncertainty import covariance_from_record, information_from_record  # noqa: E402


def pack_level(scene, level, dev, noise=None):
    fq = scene.feats_query[level].clone()
    Cc = fq.shape[0] - 1
    if noise is not None:
        fq[:-1] += noise
    cs = cstride_for(Cc)
    h, w = fq.shape[1:]
    fmap = torch.zeros(h, w, cs)
    d = fq[:-1]
    fmap[..., :Cc] = (d / d.norm(dim=0, keepdim=True).clamp_min(1e-12)).permute(1, 2, 0)
    fmap[..., Cc] = fq[-1]
    fr = scene.feats_ref[level]
    fref = torch.zeros(fr.shape[0], cs)
    fref[:, :Cc] = fr[:, :-1] / fr[:, :-1].norm(dim=1, keepdim=True).clamp_min(1e-12)
    fref[:, Cc] = fr[:, -1]
    return fmap.to(dev).contiguous(), fref.to(dev).contiguous(), Cc, scene.camera.scale(scene.scales[level])


# ------------------------------------------------------------------------------------------------ (a)
def part_a(dev):
    rows = []
    for N in (2048, 10000):
        sc = make_lm_scene(seed=1401, width=640, height=480, n_points=N)
        p3d = torch.from_numpy(sc.p3d).float().to(dev).contiguous()
        pose = torch.from_numpy(np.concatenate([sc.R_init.reshape(-1), sc.t_init]).astype(np.float32)).to(dev)
        for level, Cc in ((0, 32), (1, 128)):
            fmap, fref, C_, cam = pack_level(sc, level, dev)
            assert C_ == Cc
            for K in (1, 24):
                ws = torch.zeros(int(_lib.lib().pxt_lm_information_workspace_bytes(K)), dtype=torch.uint8, device=dev)
                recs = [torch.zeros(48, device=dev) for _ in range(K)]
                cams = [float(x) for x in cam.as10().tolist()] * K
                nd = [int(cam._data.shape[-1] - 6)] * K

                # the native entry called directly on a problem array built ONCE: a timed call costs the host a few
                # microseconds (reported as host_us_per_call; the entry waits on its staging ring of four for more than
                # two problems, which only keeps the host at most four calls ahead), so the events time the device
                L = _lib.lib()
                probs = (_lib.LmInfoProblem * K)()
                for k in range(K):
                    q = probs[k]
                    q.p3d, q.point_mask, q.n_points = p3d.data_ptr(), None, N
                    h, w, cs_ = (int(x) for x in fmap.shape)
                    q.level.fmap, q.level.fref = fmap.data_ptr(), fref.data_ptr()
                    q.level.h, q.level.w, q.level.C, q.level.cstride = h, w, Cc, cs_
                    q.level.cam[:] = cams[:10]
                    q.level.ndist = nd[0]
                    q.pose, q.pose_is_lm_record, q.out = pose.data_ptr(), 0, recs[k].data_ptr()
                conf = _lib.LmConf()
                conf.pad, conf.loss, conf.loss_alpha, conf.loss_scale, conf.min_valid = 1, 2, 0.0, 0.1, 10
                stream = _lib.stream_ptr(dev)
                conf_ref, ws_ptr = C.byref(conf), ws.data_ptr()

                def launch():
                    rc = L.pxt_lm_information(probs, K, conf_ref, ws_ptr, stream)
                    assert rc == 0, rc

                for _ in range(20):
                    launch()
                torch.cuda.synchronize(dev)
                reps, host, per = [], [], 50
                for _ in range(7):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    # park the host ahead: the launches queue up behind a sleep, so the events time the device alone
                    torch.cuda._sleep(2_000_000)
                    e0.record()
                    t0 = time.perf_counter()
                    for _ in range(per):
                        launch()
                    host.append((time.perf_counter() - t0) * 1e6 / per)
                    e1.record()
                    e1.synchronize()
                    reps.append(e0.elapsed_time(e1) * 1e3 / per)
                n_valid = float(recs[0][1])
                cs = cstride_for(Cc)
                bytes_moved = K * n_valid * (13 * cs * 4 + 12)
                us = float(np.median(reps))
                rows.append({"N": N, "C": Cc, "problems": K, "us_per_launch_median": us, "us_min": float(min(reps)),
                             "us_max": float(max(reps)), "host_us_per_call": float(np.median(host)), "n_valid": n_valid, "bytes": bytes_moved,
                             "TB_per_s": bytes_moved / (us * 1e-6) / 1e12})
                print(rows[-1], flush=True)
    return rows


# ------------------------------------------------------------------------------------------------ (b)
def _run_r9(dev, assets, frames, names, on):
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, uncertainty=on)
    warm = 10
    for i in range(warm):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(warm, len(names)):
        tr.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    tracked = sum(bool(tr.pose_history[n]["tracked"]) for n in names[warm:])
    return tracked / dt, tracked


def part_b(dev, n_frames):
    out = {}
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n_frames + 10)
    probe = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, probe.testbed)
    names = [f"{i:06d}.png" for i in range(n_frames + 10)]
    del probe
    r9 = {"off": [], "on": []}
    for _ in range(3):
        for key, on in (("off", False), ("on", True)):
            fps, tracked = _run_r9(dev, assets, frames, names, on)
            r9[key].append(fps)
            print("r9", key, fps, tracked, flush=True)
    out["r9_640x480"] = {k: {"fps": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))} for k, v in r9.items()}
    objs = parallel.load_object_configs()
    n = 70
    names = [f"{i:06d}.png" for i in range(n)]
    assets8 = [make_tracking_assets(seed=1002 + u, width=640, height=480, n_frames=n, aabb=objs[u]["aabb"]) for u in range(8)]
    frames8 = None
    l8 = {"off": [], "on": []}
    for _ in range(3):
        for key, on in (("off", False), ("on", True)):
            trs = [PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=a) for a in assets8]
            if frames8 is None:
                frames8 = [render_query_frames(a, t.testbed) for a, t in zip(assets8, trs)]
            multi = MultiObjectTracker(trs, n_groups=2, uncertainty=on)
            warm = 10
            for i in range(warm):
                multi.run_single_frames([(names[i], frames8[j][i]) for j in range(8)])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(warm, n):
                multi.run_single_frames([(names[i], frames8[j][i]) for j in range(8)])
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            tracked = sum(bool(t.pose_history[nm]["tracked"]) for t in trs for nm in names[warm:])
            l8[key].append(tracked / dt)
            print("objects8", key, tracked / dt, tracked, flush=True)
    out["objects8_lockstep"] = {k: {"fps": v, "median": float(np.median(v)), "spread": float(max(v) - min(v))}
                                for k, v in l8.items()}
    return out


# ------------------------------------------------------------------------------------------------ (c)
def part_c(dev, runs=64, sigma=0.02):
    from pixtrack_amd.geometry import se3_exp

    sc = make_lm_scene(seed=1402, width=320, height=240, n_points=2048)
    opt = PixTrackOptimizer(dict(num_iters=100, pad=1))
    conf = opt.native_conf()
    lm_ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=dev)
    info_ws = torch.zeros(int(_lib.lib().pxt_lm_information_workspace_bytes(1)), dtype=torch.uint8, device=dev)
    p3d = torch.from_numpy(sc.p3d).float().to(dev).contiguous()
    T_gt = Pose.from_Rt(torch.from_numpy(sc.R_gt), torch.from_numpy(sc.t_gt)).float()
    lam = torch.full((6,), 1e-2)
    g = torch.Generator().manual_seed(77)
    xis, covs = [], []
    for r in range(runs):
        packs = []
        for level in (2, 1, 0):
            shape = sc.feats_query[level][:-1].shape
            fmap, fref, Cc, cam = pack_level(sc, level, dev, noise=torch.randn(shape, generator=g) * sigma * float(sc.feats_query[level][:-1].std()))
            packs.append(LevelPack(fmap, fref, Cc, cam, lam))
        res = PixTrackOptimizer.refine_levels(p3d, packs, T_gt, conf, lm_ws).result()
        rec = PixTrackOptimizer.information_levels([{"p3d": p3d, "mask": None, "pack": packs[-1], "pose": res.T}], conf, info_ws,
                                                   pool_key="calib").result()[0]
        cov, flag = covariance_from_record(rec, packs[-1].C)
        assert flag == "ok" and not res.failed
        # the left perturbation that takes the ground truth to the estimate (first order)
        D = Pose(res.T.as12().double()) @ Pose(T_gt.as12().double()).inv()
        Rd = D.R.numpy()
        w = np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2
        xis.append(np.concatenate([D.t.numpy(), w]))
        covs.append(cov)
    xis = np.stack(xis)
    cov_pred = np.mean(covs, 0)
    lamp, vec = np.linalg.eigh(cov_pred)
    proj = (xis - xis.mean(0)) @ vec
    emp = proj.var(0, ddof=1)
    return {"runs": runs, "noise_sigma_relative": sigma, "predicted_variance": lamp.tolist(), "empirical_variance": emp.tolist(),
            "ratio_empirical_over_predicted": (emp / lamp).tolist(), "bias_norm": float(np.linalg.norm(xis.mean(0)))}


# ------------------------------------------------------------------------------------------------ (d)
def part_d(dev, n=65):
    objs = parallel.load_object_configs()
    out = {}
    for u in (0, 6):
        assets = make_tracking_assets(seed=1002 + u, width=640, height=480, n_frames=n, aabb=objs[u]["aabb"])
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets, uncertainty=True)
        frames = render_query_frames(assets, tr.testbed)
        rows = []
        for i in range(n):
            name = f"{i:06d}.png"
            tr.run_single_frame((name, frames[i]))
            ret = tr.pose_history[name]
            R_gt = np.asarray(assets["gt_poses"][i][0], np.float64)
            R = tr.pose.R.double().numpy()
            err = float(np.arccos(np.clip((np.trace(R @ R_gt.T) - 1) / 2, -1, 1)))
            obs = ret.get("observability")
            rows.append({"frame": i, "tracked": bool(ret["tracked"]), "rot_err_rad": err, "reference_id": int(tr.reference_ids[0]),
                         "condition": None if obs is None else float(obs["condition"]),
                         "weakest_sigma": None if obs is None else float(obs["weakest_sigma"]),
                         "weakest_direction": None if obs is None else [float(x) for x in obs["weakest_direction"]]})
        out[objs[u]["name"]] = rows
        cond = np.array([r["condition"] if r["condition"] is not None else np.nan for r in rows])
        lo, hi = (10, 20) if u == 0 else (35, 46)
        inside, outside = cond[lo:hi + 1], np.concatenate([cond[1:lo], cond[hi + 1:]])
        out[objs[u]["name"] + "_summary"] = {"window": [lo, hi], "median_condition_inside": float(np.nanmedian(inside)),
                                             "median_condition_outside": float(np.nanmedian(outside)),
                                             "max_condition_outside": float(np.nanmax(outside)),
                                             "max_rot_err_inside": float(max(r["rot_err_rad"] for r in rows[lo:hi + 1]))}
        print(objs[u]["name"], out[objs[u]["name"] + "_summary"], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08_pose_uncertainty.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    for part, fn in (("a", lambda: part_a(dev)), ("b", lambda: part_b(dev, args.frames)), ("c", lambda: part_c(dev)),
                     ("d", lambda: part_d(dev))):
        if part in args.parts:
            result[part] = fn()
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
