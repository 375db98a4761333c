#!/usr/bin/env python
"""Headline benchmark: tracked frames/s at 640x480, full per-frame hot path
(NeRF template render + depth mask -> UNet pyramids (reference + query) -> sparse sampling ->
fused LM refinement) on the synthetic premier_protein-style object of BASELINE.json configs[1].

    python bench.py --gpus N --steps K --warmup W

N = 1 : one sequence on cuda:0.  N > 1 (launched by torch.distributed.run, one rank per GPU):
every rank tracks its OWN independently seeded sequence (frames of one video are sequentially
dependent), no communication in the loop, one RCCL all_gather of the pose
records at the end -> "weak" scaling.  A step = one tracked frame; query frames are resident
in HBM before the timed region.  Rank 0 prints ONE JSON line.

Workloads (--config): `frames640` (default; BASELINE configs[1], the metric's configuration),
`objects8` (configs[3]: rank r tracks the object whose render box is the r-th OBJ_AABB of the
reference's config/*.sh), `hd` (configs[4]: 1920x1080 queries, 10 000 points, the 4-level stress
pyramid, ONE video cut into per-rank frame segments that cold-start, stitched by the final gather).

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints its line, which
carries the live roofline of the dominant kernel from the timed steps.  `--full` adds what takes
runs of its own: the untimed per-stage and roofline passes (`stage_ms_per_frame`,
`roofline_stages`), the extra passes (`extras`, N = 1), the CPU baseline (N = 1) and, for
objects8, the phase times and the one-object comparison passes.

The timed loop carries only the roofline's instrumentation (HIP events around the dominant
kernel's launches of every 4th render, one sample-count atomic per workgroup); with --full,
per-stage times come from a separate untimed pass over the next 20 frames.  Garbage is collected
and frozen BEFORE the warm-up frames (collected between them and the timed region it left the
GPU idle and the first timed frame 0.75 ms slow).  The per-frame cost
varies along the synthetic orbit (longer rays as the object turns: render 0.66 ms on the first
frames, 0.70-0.79 later), so `value` depends a little on K: 680-692 frames/s at the driver's K = 20
and at K = 60, 652-665 over 200 frames (`extras.value_k200`); `extras.value_two_renders` (549-552) is
the real-asset case in which the mask and the reference image need two renders, and
`extras.value_ycb_refshape` / `value_r9_phone` / `value_r9_12mp` (410 / 407 / 248) run the reference's
own reference-image shapes (921x921, 960x720, 2016x1512 -> 1024x768).  The pool's boxes differ by ~5 %.

N > 1 without a launcher (`python bench.py --gpus 8`) spawns its own N ranks under
torch.distributed.run; a world size that differs from --gpus, or fewer GPUs than ranks with the
RCCL backend, is an error.  The line carries what the collective layer saw: `ranks_seen`, per-rank
device / PCI bus / NUMA node / own frames/s, `rccl_version`.

`--dump-outputs DIR` writes what the timed path handed its caller in its last step (rank 0: the frame's pose record, one
row per tracker) as float64 DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

# commits at which the committed rocprofv3 PMC summaries were collected (files without a `_meta` record)
PROFILE_COMMITS = {"r06": "a77c9a2", "r05": "0f536bf", "r04": "57b838f", "r03": "a686fc1", "r02": "2a1bccf"}
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
NERF_BYTES_PER_SAMPLE = 512.0  # 16 levels x 8 corners x 2 features x 2 B
# the dominant kernel: gathers + both MLPs of a round's samples (Shade + Depth of the same rays: MODE 2)
GATHER_KERNEL = "ngp_render_kernel<2> (a whole render: persistent waves marching their rays, hash-grid gathers + both MLPs + compositing)"
GATHER_KERNEL_PMC = "pxt::ngp_render_kernel_v<2>"


MFMA_PEAK_TFLOPS = 2500.0  # dense fp16 MFMA peak (/opt/skills/guides/MI355X_MICROARCH.md)


def unet_gflop(H, W):
    """2 * 9 * Cin * Cout * h * w over the 17 3x3 convolutions of one image (241.4 at 640x480; the 1x1 heads
    add 0.5 % and are not counted)."""
    from pixtrack_amd.unet import conv_layer_dims

    hs = [(H >> i, W >> i) for i in range(5)]
    dec = [(hs[4][0] * 2 ** (d + 1), hs[4][1] * 2 ** (d + 1)) for d in range(4)]
    res = [hs[0]] * 2 + [hs[1]] * 2 + [hs[2]] * 3 + [hs[3]] * 3 + [hs[4]] * 3 + dec
    return sum(2 * 9 * cin * cout * h * w for (cin, cout), (h, w) in zip(conv_layer_dims(), res)) / 1e9


def lm_algorithmic_mb(n_points, iters, channels):
    """SURVEY 8d per iteration and level: N * (12 * C' * 4 + 12 + C' * 4) bytes, C' = C + 1, summed over the iterations
    each level ran."""
    return sum(it * n_points * (12 * (c + 1) * 4 + 12 + (c + 1) * 4) for it, c in zip(iters, channels)) / 1e6


def stage_rooflines(tracker, frames, names, lo, hi, dev, run_frame=None):
    """Live per-stage rooflines of the UNet and the LM from an untimed pass over frames[lo:hi]:
    HIP events around the frame's two-image UNet call with the join INSIDE the call, and around the LM launch; render-ahead
    off so that nothing rides behind the LM kernel.  UNet: GFLOP of the sizes actually run / ms against the dense fp16 MFMA
    peak; LM: algorithmic bytes of the iterations the kernel log reports / kernel time against the HBM peak."""
    from pixtrack_amd.optimizer import PixTrackOptimizer

    ex = tracker.localizer.extractor
    model = ex.model
    ev_unet, ev_lm, sizes, lm_meta = [], [], [], []
    orig_fwd, orig_lm = model.forward_packed_batch, PixTrackOptimizer.refine_levels
    defer0, ahead0 = ex.defer_join, tracker.render_ahead

    def fwd(items):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_fwd(items)
        e1.record()
        ev_unet.append((e0, e1))
        sizes.append([(int(it[0].shape[0]), int(it[0].shape[1])) for it in items])
        return out

    def lm(p3d, levels, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pend = orig_lm(p3d, levels, *a, **k)
        e1.record()
        ev_lm.append((e0, e1))
        lm_meta.append((int(p3d.shape[0]), [int(lp.C) for lp in levels]))
        return pend

    model.forward_packed_batch = fwd
    PixTrackOptimizer.refine_levels = staticmethod(lm)
    ex.defer_join = False
    tracker.render_ahead = False
    tracker._ahead_ok = None
    iters = []
    try:
        torch.cuda.synchronize()
        for i in range(lo, hi):
            if run_frame is not None:
                run_frame(i)
            else:
                tracker.run_single_frame((names[i], frames[i]))
            iters.append([list(r.iters) for r in tracker.localizer.refiner.last_lm])
        torch.cuda.synchronize()
    finally:
        model.forward_packed_batch = orig_fwd
        PixTrackOptimizer.refine_levels = staticmethod(orig_lm)
        ex.defer_join, tracker.render_ahead = defer0, ahead0
    out = {}
    if ev_unet:
        ms = float(np.mean([a.elapsed_time(b) for a, b in ev_unet]))
        gf = float(np.mean([sum(unet_gflop(h, w) for h, w in sz) for sz in sizes]))
        out["unet"] = {"bound": "mfma", "gflop_per_call": round(gf, 1), "image_sizes_hw": sizes[-1], "ms": round(ms, 4),
                       "achieved": round(gf / ms, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                       "frac": round(gf / ms / MFMA_PEAK_TFLOPS, 4), "calls": len(ev_unet),
                       "what": "the frame's UNet call (both images, join inside), HIP events, untimed pass"}
    if ev_lm:
        us = [a.elapsed_time(b) * 1e3 for a, b in ev_lm]
        flat = [it for per in iters for it in per]
        mb = [lm_algorithmic_mb(n, it, ch) for (n, ch), it in zip(lm_meta, flat)]
        n_it = [sum(it) for it in flat]
        tbs = float(np.sum(mb)) / float(np.sum(us))  # MB / us = TB/s
        out["lm"] = {"bound": "hbm", "iterations_per_level_mean": [round(float(x), 2) for x in np.mean(np.array(flat, float), 0)],
                     "level_channels": lm_meta[-1][1], "n_points": lm_meta[-1][0],
                     "algorithmic_mb": round(float(np.mean(mb)), 2), "kernel_us": round(float(np.mean(us)), 2),
                     "us_per_iteration": round(float(np.sum(us)) / max(int(np.sum(n_it)), 1), 2),
                     "achieved": round(tbs * 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(tbs * 1e3 / HBM_PEAK_GBS, 4), "launches": len(ev_lm),
                     "what": "lm_refine_kernel, HIP events around the launch, iterations from the kernel's own log"}
    return out


def _tracked(ret) -> bool:
    """A frame counts as tracked when the TRACKER accepted it (refiner success and the cost gate), parallel.frame_tracked."""
    from pixtrack_amd.parallel import frame_tracked

    return frame_tracked(ret)


def dump_outputs(out_dir, trackers, name):
    """--dump-outputs DIR: what the timed path handed its caller in its last step (frame `name`), one row per tracker, as
    float64 .npy files: the frame's pose_history entry - `T_refined`, `T_init` as R (9, row-major) | t (3), `cost`,
    `success` and `tracked` (0 / 1) - and `pose`, the pose the tracker carries into the next frame.  Called right after
    the timed loop, before the untimed passes run more frames through the same trackers."""
    def as12(T):
        return T.as12().detach().cpu().double().numpy().reshape(12)

    cols = {"T_refined": [], "T_init": [], "pose": [], "cost": [], "success": [], "tracked": []}
    for tr in trackers:
        ret = tr.pose_history[name]
        cols["T_refined"].append(as12(ret.get("T_refined", ret["T_init"])))
        cols["T_init"].append(as12(ret["T_init"]))
        cols["pose"].append(as12(tr.pose))
        cols["cost"].append(float(ret.get("cost", float("nan"))))
        cols["success"].append(1.0 if ret["success"] else 0.0)
        cols["tracked"].append(1.0 if _tracked(ret) else 0.0)
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for k, v in cols.items():
        np.save(out / f"{k}.npy", np.asarray(v, dtype=np.float64))


class StageTimer:
    """HIP-event timing of a wrapped callable on torch's current stream (the stream every
    pxt_* launch of this process uses)."""

    def __init__(self):
        self.events = {}
        self.enabled = False

    def wrap(self, obj, attr, name):
        fn = getattr(obj, attr)

        def timed(*a, **k):
            if not self.enabled:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.events.setdefault(name, []).append((e0, e1))
            return out

        setattr(obj, attr, timed)

    def totals_ms(self):
        return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in self.events.items()}


def cpu_baseline(assets, frames, first, ref_id, budget_s=70.0, max_frames=20, min_frames=5, warmup_frames=1):
    """The CPU oracle ("port" of the reference PyTorch-CPU path) on a bounded sample of the same
    workload, on the GPU box's host cores: whole frames of `oracle.frame_oracle.track_frame` at FULL size - depth
    render (mask) + RGB render (reference) + UNet x2 + sparse sampling + LM - frame `first + k` tracked from the
    ground-truth pose of frame `first + k - 1`, 1 warm-up frame, then up to `max_frames` frames or `budget_s` seconds
    (at least `min_frames`).  Every stage runs on `cores` host cores: the NeRF renders are dealt row-wise to that many
    worker processes (oracle.ngp_oracle.render_parallel: rays are independent; the image is asserted bit-identical to
    the serial oracle's on a band of rows), the UNet / LM legs use that many torch threads."""
    from oracle import frame_oracle as FO
    from oracle import ngp_oracle as NO

    # 16-32 threads are the sweet spot of torch-CPU convs on the 2 x 64-core host (256 threads: 35x slower)
    n_threads = min(32, os.cpu_count() or 1)
    torch.set_num_threads(n_threads)
    procs_before = NO.DEFAULT_PROCS
    NO.DEFAULT_PROCS = n_threads
    try:
        gt = assets["gt_poses"]
        # the tiled render IS the serial render: a band of rows, serially, against the same rows of the tiled image
        ngp = FO.ngp_model(assets["snapshot"])
        qcam = FO.colmap_camera_to_pix(dict(assets["query_camera"]))
        view = FO.nerf_view(assets["snapshot"], assets["nerf2sfm"], assets["aabb"], gt[first][0], gt[first][1], qcam, 0)
        t0 = time.perf_counter()
        tiled, st = NO.render(ngp, view, return_stats=True)
        t_one_render = time.perf_counter() - t0
        r0 = view.height // 2 - 8
        band, _ = NO.render(ngp, view, return_stats=True, rows=(r0, r0 + 16))
        tiled_identical = bool(np.array_equal(band, tiled[r0:r0 + 16]))
        assert tiled_identical, "tiled oracle render differs from the serial oracle"
        per_frame, stage_s, ok = [], {}, 0
        t_start = time.perf_counter()
        for k in range(max_frames + warmup_frames):  # k < warmup_frames: warm-up (thread pools, allocator, worker start-up)
            i = first + 1 + k
            if i >= len(frames) or i >= len(gt):
                break
            tm = {}
            img = frames[i].cpu().numpy()
            t0 = time.perf_counter()
            ret = FO.track_frame(assets, gt[i - 1][0], gt[i - 1][1], img, ref_id, multiscale=(1,), use_mask=True, timings=tm)
            dt = time.perf_counter() - t0
            if k < warmup_frames:
                continue
            per_frame.append(dt)
            ok += int(bool(ret["success"]))
            for name, v in tm.items():
                stage_s[name] = stage_s.get(name, 0.0) + v
            if len(per_frame) >= min_frames and time.perf_counter() - t_start > budget_s:
                break
    finally:
        NO.DEFAULT_PROCS = procs_before
        NO.close_pool()
    n = len(per_frame)
    t_frame = float(np.mean(per_frame))
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "")
    except OSError:
        pass
    return {
        "value": round(1.0 / t_frame, 5), "unit": "frames/s", "cores": n_threads, "kind": "port",
        "host_cpu_count": os.cpu_count(), "torch_threads": torch.get_num_threads(), "render_processes": n_threads,
        "host_cpu": model, "frames": n, "tracked_ok": ok, "seconds_per_frame": round(t_frame, 3),
        "stage_seconds_per_frame": {k: round(v / n, 3) for k, v in stage_s.items()},
        "tiled_render_bit_identical_to_serial": tiled_identical,
        "one_render_seconds": round(t_one_render, 2), "samples_per_render": int(st["samples"]),
        "warmup_frames": warmup_frames, "render_pool_degraded_to_serial": bool(NO._POOL.get("degraded")),
        "baseline_md_section_3": ("to the letter (3 warm-up + >= 20 frames)" if warmup_frames >= 3 and n >= 20 else
                                  f"bounded sample ({warmup_frames} warm-up + {n} frames: the default run keeps the whole bench "
                                  "within a few minutes; `--cpu-baseline-frames 20` runs 3 + 20)"),
        "sample": (f"{n} whole 640x480 frames after {warmup_frames} warm-up frame(s) (oracle.frame_oracle.track_frame: depth + RGB NeRF renders at "
                   f"full size, spp 8, UNet x2, sparse sampling, LM), mean {t_frame:.2f} s/frame; every stage on {n_threads} of the "
                   f"{os.cpu_count()} host CPUs (NeRF rows dealt to {n_threads} processes - bit-identical to the serial oracle, "
                   f"asserted; UNet / LM on {n_threads} torch threads)"),
    }


def _timed_frames(tracker, frames, names, lo, hi):
    """frames/s of run_single_frame over frames[lo:hi] (synchronised on both sides)."""
    import gc

    # (as the headline loop: no generation-2 collection - a 10 ms stall of the host in a process that by now holds several
    # trackers' assets - in the middle of a timed pass; round 5: value_r9_phone 464 inside the full run, 551 on its own)
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(lo, hi):
            tracker.run_single_frame((names[i], frames[i]))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        if was:
            gc.enable()
    ok = sum(1 for i in range(lo, hi) if _tracked(tracker.pose_history[names[i]]))
    return (hi - lo) / dt, ok


def run_extras(tracker, assets, frames, names, warmup, n_timed_end, first_free, dev):
    """Extra passes that say what the headline leaves out (N = 1 only; outside the contract's timed region):
    (a) `value_two_renders`: the mask and the reference image need TWO renders - the real-asset case, where
        SfM camera 1 x reference_scale differs from the query camera (pixloc_tracker_r9.py:145-152);
    (b) `value_host_frames_debug1`: frames arrive from pinned HOST memory (H2D copy inside the loop, as the
        reference's ImageIterator hands frames over) and --debug 1 (the shipped run_inference.sh setting);
    both REPLAY the frames of the timed region (same warm-up frames, same timed frames) on a fresh tracker,
    so they compare with `value` frame for frame;
    (c) `value_k200`: the headline configuration over the 200 frames that follow (the per-frame cost drifts
        along the synthetic orbit as the object turns its broad side to the camera);
    (d) `value_ycb_policy`: the YCB tracker's policy on its own synthetic object (ycb_policy_extra);
    (e) `value_objects8_one_gpu` (configs[3] at N = 1: all eight config/*.sh objects in lock-step, with the comparison
        against eight one-object runs), `value_hd`: the other two workloads at N = 1, each its own run of this file."""
    import gc

    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    out = {}

    def replay(setup, make_frame):
        tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
        setup(tr)
        fr = [make_frame(frames[i]) for i in range(n_timed_end)]
        gc.collect()  # (before the warm-up frames: no idle GPU between them and the timed ones)
        gc.disable()
        for i in range(warmup):
            tr.run_single_frame((names[i], fr[i]))
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(warmup, n_timed_end):
                tr.run_single_frame((names[i], fr[i]))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            gc.enable()
        n = n_timed_end - warmup
        ok = sum(1 for i in range(warmup, n_timed_end) if _tracked(tr.pose_history[names[i]]))
        return round(n / dt, 2), n, ok

    def two_renders(tr):
        tr.fuse_identical_views = False

    fps, n, ok = replay(two_renders, lambda f: f)
    out["value_two_renders"] = {"frames_per_s": fps, "frames": n, "tracked_ok": ok,
                                "what": "same frames as `value`; mask (Depth) and reference (Shade) rendered separately"}

    def debug1(tr):
        tr.debug = 1

    fps, n, ok = replay(debug1, lambda f: f.cpu().pin_memory())
    out["value_host_frames_debug1"] = {"frames_per_s": fps, "frames": n, "tracked_ok": ok,
                                       "what": "same frames as `value`, float32 in pinned host memory (3.7 MB H2D per "
                                               "frame inside the loop), DebugTracker at --debug 1"}
    gc.collect()
    gc.disable()
    try:
        fps, ok = _timed_frames(tracker, frames, names, first_free, first_free + 200)
    finally:
        gc.enable()
    out["value_k200"] = {"frames_per_s": round(fps, 2), "frames": 200, "tracked_ok": ok,
                         "what": "headline configuration, the 200 frames after the timed and diagnostic ones"}
    out["value_ycb_policy"] = ycb_policy_extra(dev)
    # the reference's OWN reference-image shapes (VERDICT r3 missing #1)
    from pixtrack_amd.synthetic import REF_CAMERA_12MP, REF_CAMERA_PHONE

    for key, fn in (("value_ycb_refshape", lambda: ycb_policy_extra(dev, refshape=True)),
                    ("value_r9_phone", lambda: r9_refshape_extra(dev, REF_CAMERA_PHONE, "1920x1440 (4:3 phone frames)")),
                    ("value_r9_12mp", lambda: r9_refshape_extra(dev, REF_CAMERA_12MP, "4032x3024 (12-MP stills)", n=34))):
        try:
            out[key] = fn()
        except Exception as e:  # (reported, never fatal: the headline line must come out)
            out[key] = {"frames_per_s": None, "error": repr(e)[:300]}
    # BASELINE configs[3] / [4] at N = 1, each as its own `--config` run of this file: one driver record for all three workloads
    for key, argv in (("value_objects8_one_gpu", ["--config", "objects8", "--steps", "20", "--warmup", "5", "--full"]),
                      ("value_hd", ["--config", "hd", "--steps", "12", "--warmup", "3", "--full"])):
        out[key] = other_config_extra(argv)
    return out


def other_config_extra(argv, timeout_s=420):
    import subprocess

    try:
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], capture_output=True, text=True, timeout=timeout_s,
                           env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
        line = json.loads(r.stdout.strip().splitlines()[-1])
        rec = {"frames_per_s": line["value"], "frames": line.get("frames_total", line["steps"]), "tracked_ok": line.get("tracked_ok"),
               "ms_per_step": line["ms_per_step"], "what": "python bench.py " + " ".join(argv) + ": " + line["config"]["workload"][:200]}
        if line.get("solo_runs"):  # objects8 in lock-step: the comparison against one-object runs and the batched stages
            rec["solo_aggregate_frames_per_s"] = line["solo_runs"]["aggregate_frames_per_s"]
            rec["lockstep_speedup"] = line["solo_runs"]["lockstep_speedup"]
            rec["max_abs_pose_difference_vs_solo"] = max(line["solo_runs"]["max_abs_pose_difference_vs_lockstep"])
            vb = line.get("value_bit_identical") or {}
            rec["value_bit_identical"] = {k: vb.get(k) for k in ("frames_per_s", "bit_identical_to_solo_runs", "tracked_ok")}
            rec["max_rot_err_vs_gt_rad"] = line.get("max_rot_err_vs_gt_rad")
            st = line.get("roofline_stages") or {}
            rec["unet_batched"] = {k: st["unet"][k] for k in ("images_per_call", "ms_per_image_pair", "achieved", "frac")} if "unet" in st else None
            rec["lm_batched"] = {k: st["lm"][k] for k in ("problems_per_launch", "kernel_us", "us_per_problem")} if "lm" in st else None
        return rec
    except Exception as e:  # (reported, never fatal: the headline line must come out)
        return {"frames_per_s": None, "what": "python bench.py " + " ".join(argv), "error": repr(e)[:200]}


def refshape_stage_block(tr, run_frame, lo, hi, dev):
    """`roofline_refshape` of an extra pass: per-stage HIP-event ms over frames [lo, mid) with the
    render-ahead off, then the live UNet / LM rooflines over [mid, hi) - where a real-asset frame's time goes."""
    mid = (lo + hi) // 2
    timer = StageTimer()
    for attr in ("render_device", "render_both_device", "render_frame_device", "render_frame_pair_device"):
        timer.wrap(tr.testbed, attr, "nerf_render")
    timer.wrap(tr.localizer.extractor.model, "forward_packed_batch", "unet")
    timer.wrap(tr.localizer.refiner, "refine_pose_using_features", "lm")
    timer.wrap(tr.localizer.refiner, "interp_sparse_observations", "sample")
    ahead = tr.render_ahead
    tr.render_ahead = False
    tr._ahead_ok = None
    torch.cuda.synchronize()
    timer.enabled = True
    for i in range(lo, mid):
        run_frame(i)
    torch.cuda.synchronize()
    timer.enabled = False
    tr.render_ahead = ahead
    stage = {k: round(v[0] / max(mid - lo, 1), 4) for k, v in timer.totals_ms().items()}
    roof = stage_rooflines(tr, None, None, mid, hi, dev, run_frame=run_frame)
    dom = max(stage, key=stage.get) if stage else None
    return {"stage_ms_per_frame": stage, "dominant_stage": dom, **roof,
            "what": f"untimed: HIP-event stage times over {mid - lo} frames (render-ahead off; `nerf_render` = the frame's two renders as "
                    "one chain of three launches), then the UNet call / LM launch with events"}


def ycb_policy_extra(dev, n=70, lead=10, refshape=False):
    """BASELINE configs[2]'s policy (pixloc_tracker_ycb.py:241-295: mask every frame, GT-gated pose update, reference
    camera x 0.3, render box from the SfM points) on the synthetic unit-cube object at 640x480: per frame two renders of
    DIFFERENT cameras and two UNet passes of different sizes.  A different object and policy than `value` - reported
    beside it, never as it.  ``refshape``: with the reference's OWN camera shapes instead of the "query size / 0.3"
    stand-in - SfM camera 1 = 3072 x 3072, f 2700 (scripts/create_sfm_from_obj.py:154-159) x 0.3 -> a 921 x 921
    reference render and UNet pass per frame (2.76 x the pixels of 640 x 480), the query camera with the YCB-Video
    intrinsics fx 1066.778 / fy 1067.487 and the principal point forced to (319.5, 239.5) (pixtrack/utils/io.py:46-50)."""
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.pose_trackers import pixloc_tracker_ycb as ycb
    from pixtrack_amd.synthetic import (CRACKER_BOX_AABB, REF_CAMERA_YCB, YCB_QUERY_FXY, make_tracking_assets,
                                        render_query_frames)

    kw = dict(ref_camera=REF_CAMERA_YCB, query_f=YCB_QUERY_FXY[0]) if refshape else {}
    n_diag = 12 if refshape else 0
    assets = make_tracking_assets(seed=1005, width=640, height=480, n_frames=n + n_diag, aabb=CRACKER_BOX_AABB,
                                  reference_scale=0.3, n_points=5600, **kw)
    tr = ycb.PixLocPoseTrackerYCB("", "", "/tmp", "003_cracker_box", device=dev, assets=assets)
    f = float(assets["query_camera"]["params"][0])
    fxy = YCB_QUERY_FXY if refshape else (f, f)
    cam = Camera.from_colmap(dict(model="OPENCV", width=640, height=480, params=np.array([fxy[0], fxy[1], 319.5, 239.5])))
    frames = render_query_frames(assets, tr.testbed)
    gts = [Pose.from_Rt(*p) for p in assets["gt_poses"]]
    import gc

    ok, t0 = 0, 0.0
    gc_was = gc.isenabled()
    try:
        for i in range(n):
            if i == lead:
                gc.collect()  # (no collection inside the timed frames: see _timed_frames)
                gc.disable()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            good = bool(tr.refine((f"{i + 1:06d}-color.png", frames[i], gts[i], cam)))
            ok += int(good and i >= lead)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        if gc_was:
            gc.enable()
    block = None
    if refshape:
        block = refshape_stage_block(tr, lambda i: tr.refine((f"{i + 1:06d}-color.png", frames[i], gts[i], cam)), n, n + n_diag, dev)
    what = ("the YCB policy (configs[2]) on the synthetic unit-cube object, 640x480, 5600 points, reference at 0.3 x: "
            "two renders of different cameras (ONE chain of launches) + two UNet passes of different sizes per frame")
    if refshape:
        what = ("the YCB policy with the reference's own camera shapes: SfM camera 3072x3072 f 2700 x 0.3 -> 921x921 "
                "reference render + UNet pass, query 640x480 with fx 1066.778 / fy 1067.487, c (319.5, 239.5)")
    return {"frames_per_s": round((n - lead) / dt, 2), "frames": n - lead, "tracked_ok": ok,
            "renders_ahead_used": int(tr.renders_ahead_used),
            "reference_render_wh": [int(x) for x in tr._reference_camera().size],
            "reference_unet_input_wh": [int(x) for x in (getattr(tr.localizer.refiner, "last_reference_wh", None) or (0, 0))],
            **({"roofline_refshape": block} if block else {}), "what": what}


def r9_refshape_extra(dev, ref_camera, label, n=44, lead=10):
    """The r9 policy (configs[1]) with SfM camera 1 shaped as the reference's own assets have it instead of the
    "2 x query" stand-in: the reference render is `cameras[1] x 0.5` (pixloc_tracker_r9.py:145-152), a different
    camera than the 640x480 query, so a frame needs two renders of different views and two UNet passes of
    different sizes; above 1024 px the extractor's resize path runs (feature_extractor.py:41-45)."""
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    n_diag = 12
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n + n_diag, ref_camera=ref_camera)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, tr.testbed)
    names = [f"{i:06d}.png" for i in range(n + n_diag)]
    for i in range(lead):
        tr.run_single_frame((names[i], frames[i]))
    fps, ok = _timed_frames(tr, frames, names, lead, n)
    rw, rh = (int(x) for x in tr._reference_camera().size)
    block = refshape_stage_block(tr, lambda i: tr.run_single_frame((names[i], frames[i])), n, n + n_diag, dev)
    return {"frames_per_s": round(fps, 2), "frames": n - lead, "tracked_ok": ok, "reference_render_wh": [rw, rh],
            "reference_unet_input_wh": [int(x) for x in (getattr(tr.localizer.refiner, "last_reference_wh", None) or (rw, rh))],
            "roofline_refshape": block,
            "renders_ahead_used": int(tr.renders_ahead_used),
            "what": f"r9 policy, query 640x480, SfM camera 1 = {label} x 0.5 -> {rw}x{rh} reference render"}


def run_hd(args, rank, ws, dev, coll_dev, numa_node):
    """BASELINE configs[4]: 1920x1080 queries (the extractor resizes them to 1024x576), ~10 000 3-D
    points per reference image, the 4-level STRESS pyramid {image scale 4: level 2; scale 1: levels
    2, 1, 0} (the reference has 3 levels per image scale; this plan is the builder's definition, not
    a parity configuration), ONE video of --steps frames cut into contiguous per-rank segments.  Every
    segment head is a cold start from an externally supplied pose (here: ground truth moved by
    3 deg / 2 cm), so results at segment heads differ from a sequential run.  value =
    frames of the whole video / slowest rank's time ("strong" scaling)."""
    from pixtrack_amd import parallel
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, perturb_pose, render_query_frames

    W, H = 1920, 1080
    n_total = args.steps
    segs_all = [parallel.shard_segments(n_total, ws, r) for r in range(ws)]
    segs = segs_all[rank]
    assets = make_tracking_assets(seed=1005, width=W, height=H, n_frames=n_total, n_points=24500)
    tracker = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    tracker.steady_multiscale = [4, 1]
    tracker.localizer.refiner.conf.level_plan = {4: [2], 1: [2, 1, 0]}
    # only this rank's frames are rendered (query frames are inputs: set-up, not timed)
    mine = [i for (a, b) in segs for i in range(a, b)]
    sub = dict(assets)
    sub["gt_poses"] = [assets["gt_poses"][i] for i in mine]
    heads = {mine.index(a) for (a, b) in segs}  # segment heads are cold starts: worse observations (see synthetic.py)
    frames = dict(zip(mine, render_query_frames(sub, tracker.testbed, cold_start_indices=heads)))
    names = {i: f"{i:06d}.png" for i in mine}
    rng = np.random.default_rng(77 + rank)
    # warm-up: the first frames of the first segment, then the tracker is reset for the timed pass
    import gc

    gc.collect()  # (before the warm-up frames: no idle GPU between them and the timed ones)
    gc.freeze()
    gc.disable()
    if mine:
        for i in mine[: max(1, min(args.warmup, len(mine)))]:
            tracker.run_single_frame((names[i], frames[i]))
    if ws > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for (a, b) in segs:
        Rg, tg = assets["gt_poses"][a]
        Ri, ti = perturb_pose(Rg, tg, rng, 3.0, 0.02, assets["center"])
        tracker.start_segment(Pose.from_Rt(Ri, ti))
        for i in range(a, b):
            tracker.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize()
    if ws > 1:
        torch.distributed.barrier()
    own = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [tracker], names[mine[-1]])
    elapsed = parallel.max_over_ranks(own, coll_dev)
    gc.enable()
    report = rank_report(rank, dev.index, dev, numa_node, len(mine), own, coll_dev)
    records = parallel.pack_pose_records(tracker.pose_history, [names[i] for i in mine])
    gathered = parallel.gather_pose_records(records.to(coll_dev), coll_dev)
    video = parallel.stitch_segments(gathered, segs_all, n_total)
    if rank != 0:
        return
    rot, tra = [], []
    for i in range(n_total):
        if video[i, 12] > 0:
            Rr, tt = video[i, :9].reshape(3, 3).numpy(), video[i, 9:12].numpy()
            Rg, tg = assets["gt_poses"][i]
            rot.append(float(np.arccos(np.clip((np.trace(Rr @ Rg.T) - 1) / 2, -1, 1))))
            tra.append(float(np.linalg.norm(tt - tg)))
    lm = tracker.localizer.refiner.last_lm
    # untimed (--full): where a frame of this workload goes (HIP events per stage, the last frames of this rank's last segment
    # again)
    stage_hd = None
    if mine and args.full:
        timer = StageTimer()
        for attr in ("render_device", "render_both_device", "render_frame_device", "render_frame_pair_device"):
            timer.wrap(tracker.testbed, attr, "nerf_render")
        timer.wrap(tracker.localizer.extractor.model, "forward_packed_batch", "unet")
        timer.wrap(tracker.localizer.extractor.model, "forward_packed", "unet")
        timer.wrap(tracker.localizer.refiner, "refine_pose_using_features", "lm")
        timer.wrap(tracker.localizer.refiner, "interp_sparse_observations", "sample")
        tail = mine[-min(4, len(mine)):]
        torch.cuda.synchronize()
        timer.enabled = True
        t1 = time.perf_counter()
        for i in tail:
            tracker.run_single_frame((names[i], frames[i]))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t1) / len(tail) * 1e3
        timer.enabled = False
        stage_hd = {k: round(v[0] / len(tail), 4) for k, v in timer.totals_ms().items()}
        stage_hd["wall_ms_per_frame"] = round(wall, 4)
    out = {
        "metric": "tracked frames/sec at 1920x1080 (configs[4] stress workload)", "value": round(n_total / elapsed, 3),
        "unit": "frames/s", "n_gpus": ws, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / max(n_total, 1) * 1e3, 4), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "fp16 storage / fp32 accumulate (UNet, NeRF MLPs); fp32 (LM)",
        "data": "synthetic (seeded hash-grid NeRF, He-init UNet, NeRF-rendered query frames + noise)",
        "config": {"workload": "configs[4]: 1920x1080 queries (-> 1024x576 in the extractor), 4-level stress pyramid "
                               "{scale 4: [2], scale 1: [2,1,0]} (builder-defined, NOT a parity configuration), one video "
                               "in per-rank segments; segment heads cold-start from GT + (3 deg, 2 cm)",
                   "width": W, "height": H, "spp": 8, "segments": segs_all,
                   "n_points_per_reference": int(tracker.localizer.refiner._points_of(tracker.reference_ids)[1].shape[0]),
                   "lm_levels_per_frame": sum(len(r.iters) for r in lm), "host_numa_node": numa_node},
        "tracked_ok": int(video[:, 12].sum()), "frames_total": n_total,
        "mean_rot_err_vs_gt_rad": round(float(np.mean(rot)), 6) if rot else None,
        "mean_trans_err_vs_gt": round(float(np.mean(tra)), 6) if tra else None,
        "stage_ms_per_frame": stage_hd,
        "roofline": None, "cpu_baseline": {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port",
                                           "sample": "reported with the frames640 workload only"},
        **report,
    }
    print(json.dumps(out), flush=True)


def objects8_phase_stages(args, multi, trackers, units, frames, names, n, n_diag):
    """Untimed (--full): per-phase HIP-event times of a lock-step step over frames [n, n + n_diag) (render-ahead off:
    nothing rides behind the LM launch) and the live rooflines of the batched UNet pass and the batched LM launch."""
    ahead = [tr.render_ahead for tr in trackers]
    for tr in trackers:
        tr.render_ahead = False
        tr._ahead_ok = None
    phases, lm_iters = [], []
    multi.set_groups(1)  # (one group: the phases of a step follow each other on one stream)
    for i in range(n, n + n_diag):
        multi.timing = {}
        multi.run_single_frames([(names[i], frames[u][i]) for u in units])
        torch.cuda.synchronize()
        t = multi.timing
        order = ["step_begin", "renders_enqueued", "unet_enqueued", "sampling_enqueued", "lm_enqueued", "step_end"]
        phases.append([t[a][0].elapsed_time(t[b][0]) for a, b in zip(order[:-1], order[1:])])
        lm_iters.append([[list(r.iters) for r in tr.localizer.refiner.last_lm][0] for tr in trackers])
    multi.timing = None
    for tr, a in zip(trackers, ahead):
        tr.render_ahead = a
    ph = np.mean(np.array(phases[1:]), 0)  # (the first diagnostic step still consumed queued renders)
    K = len(units)
    gf = 2 * K * unet_gflop(args.height, args.width)
    n_pts = [int(tr.localizer.refiner._points_of(tr.reference_ids)[1].shape[0]) for tr in trackers]
    lm_mb = float(np.mean([sum(lm_algorithmic_mb(npt, it, [128, 128, 32]) for npt, it in zip(n_pts, per)) for per in lm_iters[1:]]))
    return {
        "phase_ms_per_step": {"renders": round(float(ph[0]), 4), "unet": round(float(ph[1]), 4), "sampling": round(float(ph[2]), 4),
                              "lm": round(float(ph[3]), 4), "host_policy": round(float(ph[4]), 4)},
        "unet": {"bound": "mfma", "images_per_call": 2 * K, "gflop_per_call": round(gf, 1), "ms": round(float(ph[1]), 4),
                 "achieved": round(gf / float(ph[1]), 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                 "frac": round(gf / float(ph[1]) / MFMA_PEAK_TFLOPS, 4), "ms_per_image_pair": round(float(ph[1]) / K, 4)},
        "lm": {"bound": "hbm", "problems_per_launch": K, "algorithmic_mb": round(lm_mb, 1), "kernel_us": round(float(ph[3]) * 1e3, 1),
               "us_per_problem": round(float(ph[3]) * 1e3 / K, 1), "achieved": round(lm_mb / (float(ph[3]) * 1e3) * 1e3, 1),
               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(lm_mb / (float(ph[3]) * 1e3) * 1e3 / HBM_PEAK_GBS, 4),
               "iterations_per_level_mean": [round(float(x), 2) for x in np.mean(np.array(lm_iters[1:], float), (0, 1))]},
        "what": "HIP events between the phases of an untimed lock-step step (render-ahead off), mean of 3 steps",
    }


def run_objects8(args, rank, ws, dev, coll_dev, numa_node):
    """BASELINE configs[3]: the eight objects of the reference's config/*.sh tracked CONCURRENTLY on N GPUs - rank r carries
    objects r, r + N, ... (8 / N per rank), advanced in lock-step by a MultiObjectTracker: their 2 K images of a step in one
    batched UNet pass, their K refinements in one persistent launch (pxt_lm_refine_batch), one renderer context per object.
    A step = one frame of every object of the rank; value = frames of all 8 objects / slowest rank's time (the work is
    the same 8 objects whatever N: "strong" scaling).  With --full, untimed passes follow: per-phase HIP-event times of a
    lock-step step and, at N = 1, the same frames tracked by eight one-object trackers, one after the other, for the
    comparison the line carries (solo aggregate, pose differences)."""
    import gc

    from pixtrack_amd import parallel
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    objs = parallel.load_object_configs()
    units = parallel.shard_units(len(objs), rank, ws)
    n = args.warmup + args.steps
    n_diag = 4 if args.full else 0
    names = [f"{i:06d}.png" for i in range(n + n_diag)]
    assets = {u: make_tracking_assets(seed=1002 + u, width=args.width, height=args.height, n_frames=n + n_diag,
                                      aabb=objs[u]["aabb"]) for u in units}

    def fresh(u):
        return PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets[u])

    trackers = [fresh(u) for u in units]
    # (first_frame_sigma: the reference gates every frame on cost <= 1.1 x the FIRST frame's, synthetic.render_query_frames;
    # the headline object's margin - a cold-start frame with sigma 12 - is not enough for every config/*.sh box: with it
    # 11 of 160 frames were refused by the gate, bottle and the thin slab mostly; `--first-frame-sigma` keeps that run)
    frames = {u: render_query_frames(assets[u], tr.testbed, first_frame_sigma=args.first_frame_sigma)
              for u, tr in zip(units, trackers)}
    multi = MultiObjectTracker(trackers, lm_workgroups=args.lm_grid, per_image_plan=args.per_image_plan, n_groups=args.groups)
    gc.collect()
    gc.freeze()
    gc.disable()
    for i in range(args.warmup):
        multi.run_single_frames([(names[i], frames[u][i]) for u in units])
    if ws > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, n):
        multi.run_single_frames([(names[i], frames[u][i]) for u in units])
    torch.cuda.synchronize()
    if ws > 1:
        torch.distributed.barrier()
    own = time.perf_counter() - t0
    gc.enable()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, trackers, names[n - 1])
    elapsed = parallel.max_over_ranks(own, coll_dev)
    report = rank_report(rank, dev.index, dev, numa_node, args.steps * len(units), own, coll_dev)
    timed = names[args.warmup:n]
    recs = [parallel.pack_pose_records(tr.pose_history, timed) for tr in trackers]
    gathered = parallel.gather_pose_records(torch.cat(recs).to(coll_dev), coll_dev)  # the one collective (RCCL)
    units_all = parallel.gather_objects(units)
    n_ok = int(sum(float(g[:, 12].sum()) for g in gathered))
    total_frames = sum(g.shape[0] for g in gathered)
    stages, solo = None, None
    if args.full:
        stages = objects8_phase_stages(args, multi, trackers, units, frames, names, n, n_diag)
    if args.full and ws == 1 and not args.no_solo:
        # the same frames through eight ONE-object trackers, one after the other: what the lock-step run is compared with
        fps, diffs, solo_err, lock_err, solo_ok = [], [], [], [], 0
        for u, tr_multi in zip(units, trackers):
            tr = fresh(u)
            gc.collect()
            gc.disable()
            for i in range(args.warmup):
                tr.run_single_frame((names[i], frames[u][i]))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(args.warmup, n):
                tr.run_single_frame((names[i], frames[u][i]))
            torch.cuda.synchronize()
            fps.append(args.steps / (time.perf_counter() - t1))
            gc.enable()
            solo_ok += sum(1 for nm in timed if _tracked(tr.pose_history[nm]))
            a = parallel.pack_pose_records(tr.pose_history, timed)[:, :12]
            b = parallel.pack_pose_records(tr_multi.pose_history, timed)[:, :12]
            diffs.append(float((a - b).abs().max()))
            # (and each run against the synthetic ground truth: a difference between the two runs is read against these)
            for rec, store in ((a, solo_err), (b, lock_err)):
                e = []
                for k in range(len(timed)):
                    Rr, Rg = rec[k, :9].reshape(3, 3).numpy(), assets[u]["gt_poses"][args.warmup + k][0]
                    e.append(float(np.arccos(np.clip((np.trace(Rr @ Rg.T) - 1) / 2, -1, 1))))
                store.append(round(float(np.max(e)), 5))
            del tr
        agg = len(units) * args.steps / sum(args.steps / f for f in fps)
        solo = {"frames_per_s_per_object": [round(f, 1) for f in fps], "aggregate_frames_per_s": round(agg, 2),
                "lockstep_speedup": round(total_frames / elapsed / agg, 3), "tracked_ok": solo_ok,
                "max_abs_pose_difference_vs_lockstep": [float(f"{d:.3g}") for d in diffs],
                "max_rot_err_vs_gt_rad_solo": solo_err, "max_rot_err_vs_gt_rad_lockstep": lock_err,
                "what": "untimed second pass: the same frames tracked by one-object trackers one after the other (aggregate = "
                        "all frames / summed time); pose difference = largest |element| difference of the 12 pose floats"}
        # third pass: the lock-step configuration whose poses are BIT-identical to one-object runs (every image planned as a
        # batch of one; the LM grid of both sides 32 workgroups per problem - the solo default of 128 x 8 problems does not
        # fit the 256 resident workgroups of a persistent launch) - timed like `value`, then checked against eight solo runs
        grid_bit = 32

        def fresh_grid(u):
            tr = fresh(u)
            for opt in tr.localizer.optimizer:
                opt.conf.n_workgroups = grid_bit
            # (a one-object tracker encodes a WINDOW of its reference render where that saves >= 35 % of the pixels; in
            # lock-step a reference of the query's size stays whole so that it rides in the batch: another tile plan,
            # another fp32 summation order - both sides whole here)
            tr.localizer.refiner.conf.reference_window = False
            return tr

        tb = [fresh_grid(u) for u in units]
        multi_b = MultiObjectTracker(tb, lm_workgroups=grid_bit, per_image_plan=True, n_groups=args.groups)
        gc.collect()
        gc.disable()
        for i in range(args.warmup):
            multi_b.run_single_frames([(names[i], frames[u][i]) for u in units])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.warmup, n):
            multi_b.run_single_frames([(names[i], frames[u][i]) for u in units])
        torch.cuda.synchronize()
        el_b = time.perf_counter() - t1
        gc.enable()
        worst, ok_b = 0.0, 0
        for u, trb in zip(units, tb):
            tr = fresh_grid(u)
            for i in range(n):
                tr.run_single_frame((names[i], frames[u][i]))
            torch.cuda.synchronize()
            a = parallel.pack_pose_records(tr.pose_history, names[:n])
            b = parallel.pack_pose_records(trb.pose_history, names[:n])
            worst = max(worst, float((a - b).abs().max()))
            ok_b += sum(1 for nm in timed if _tracked(trb.pose_history[nm]))
            del tr
        solo["value_bit_identical"] = {
            "frames_per_s": round(len(units) * args.steps / el_b, 2), "tracked_ok": ok_b, "lm_workgroups_per_problem": grid_bit,
            "unet_per_image_plan": True, "bit_identical_to_solo_runs": worst == 0.0, "max_abs_pose_record_difference": worst,
            "what": "lock-step with every image planned as a batch of one, both sides' LM grid at 32 workgroups per problem and the "
                    "reference pass on the whole render on both sides: "
                    "poses, decisions and costs compared with eight one-object runs of the same frames, all frames (warm-up included)"}
    if rank != 0:
        return
    rot, tra, per_obj = [], [], {}
    for tr, u in zip(trackers, units):
        r_u, t_u = [], []
        for k, nm in enumerate(timed):
            ret = tr.pose_history[nm]
            if _tracked(ret):
                Rr, tt = ret["T_refined"].numpy()
                Rg, tg = assets[u]["gt_poses"][args.warmup + k]
                r_u.append(float(np.arccos(np.clip((np.trace(Rr @ Rg.T) - 1) / 2, -1, 1))))
                t_u.append(float(np.linalg.norm(tt - tg)))
        rot += r_u
        tra += t_u
        # (per object, against the SYNTHETIC ground truth - ADVICE r4: the record of what each object's track looks like)
        per_obj[objs[u]["name"]] = {"tracked": sum(1 for nm in timed if _tracked(tr.pose_history[nm])), "frames": len(timed),
                                    "first_frame_cost": round(float(tr.cost_threshold / 1.1), 6) if tr.cost_threshold else None,
                                    "max_cost": round(max(float(tr.pose_history[nm].get("cost", 0.0)) for nm in timed), 6),
                                    "mean_rot_err_rad": round(float(np.mean(r_u)), 6) if r_u else None,
                                    "max_rot_err_rad": round(float(np.max(r_u)), 6) if r_u else None,
                                    "mean_trans_err": round(float(np.mean(t_u)), 6) if t_u else None,
                                    "camera_distance": round(float(np.linalg.norm(assets[u]["gt_poses"][args.warmup][1])), 3)}
    out = {
        "metric": "tracked frames/sec at 640x480 (8 objects of config/*.sh tracked concurrently; full NeRF render + UNet + LM loop)",
        "value": round(total_frames / elapsed, 3), "unit": "frames/s", "n_gpus": ws, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "fp16 storage / fp32 accumulate (UNet, NeRF MLPs); fp32 (LM)",
        "data": "synthetic (seeded hash-grid NeRF, He-init UNet, NeRF-rendered query frames + noise)",
        "config": {"workload": (f"configs[3]: the 8 objects of config/*.sh tracked concurrently on {ws} GPU(s), {len(units)} per rank in "
                                "lock-step (batched UNet pass + one persistent LM launch per step), 640x480, full loop; a step = one "
                                "frame of every object"),
                   "objects_per_rank": [[objs[u]["name"] for u in us] for us in units_all], "width": args.width,
                   "height": args.height, "spp": 8, "lm_workgroups_per_problem": args.lm_grid, "groups": args.groups, "first_frame_sigma": args.first_frame_sigma, "unet_per_image_plan": bool(args.per_image_plan),
                   "host_numa_node": numa_node},
        "tracked_ok": n_ok, "frames_total": total_frames,
        "per_object_frames_per_s": round(args.steps / elapsed, 3),
        "lockstep_frames": int(multi.lockstep_frames), "solo_frames_inside_lockstep": int(multi.solo_frames),
        "renders_ahead_used": [int(tr.renders_ahead_used) for tr in trackers],
        "mean_rot_err_vs_gt_rad": round(float(np.mean(rot)), 6) if rot else None,
        "mean_trans_err_vs_gt": round(float(np.mean(tra)), 6) if tra else None,
        "per_object_error_vs_synthetic_gt": per_obj,
        "value_bit_identical": (solo or {}).pop("value_bit_identical", None),
        "max_rot_err_vs_gt_rad": {k: v["max_rot_err_rad"] for k, v in per_obj.items()},
        "roofline": None, "roofline_stages": stages, "solo_runs": solo,
        "cpu_baseline": {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port",
                         "sample": "reported with the frames640 workload only"},
        **report,
    }
    print(json.dumps(out), flush=True)


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-run this command under torch.distributed.run with
    N ranks on this node (one per GPU; rendezvous on 127.0.0.1, a free port) and return its exit code.
    With RCCL as the backend a node with fewer than N GPUs is refused HERE, before anything is spawned -
    a 1-GPU run must never come back labelled n_gpus = N."""
    import socket
    import subprocess

    backend = os.environ.get("PXT_DIST_BACKEND", "nccl")
    n_dev = torch.cuda.device_count()
    if backend == "nccl" and n_dev < n:
        print(f"bench.py --gpus {n}: only {n_dev} GPU(s) visible on this node; RCCL needs one GPU per rank "
              "(PXT_DIST_BACKEND=gloo rehearses the control flow with ranks sharing devices)", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               PXT_SELF_LAUNCHED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def rank_report(rank, local_rank, dev, numa_node, frames, seconds, coll_dev):
    """What the collective layer saw: every rank's id, device, PCI bus, NUMA node and own frames/s, all-gathered
    (RCCL for backend nccl).  `ranks_seen` in the JSON line is the sorted list of rank ids that answered."""
    from pixtrack_amd import parallel

    p = torch.cuda.get_device_properties(dev)
    mine = {"rank": rank, "local_rank": local_rank, "device": f"cuda:{dev.index}", "name": p.name,
            "pci_bus": f"{int(getattr(p, 'pci_domain_id', 0)):04x}:{int(p.pci_bus_id):02x}:{int(p.pci_device_id):02x}",
            "numa_node": numa_node, "frames": frames, "frames_per_s": round(frames / seconds, 3) if seconds > 0 else None,
            "pid": os.getpid()}
    reports = parallel.gather_objects(mine)
    backend = torch.distributed.get_backend() if torch.distributed.is_initialized() else None
    try:
        v = torch.cuda.nccl.version()
        rccl = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    except Exception:
        rccl = None
    return {"ranks_seen": sorted(r["rank"] for r in reports), "ranks": sorted(reports, key=lambda r: r["rank"]),
            "dist_backend": backend, "rccl_version": rccl, "self_launched": os.environ.get("PXT_SELF_LAUNCHED") == "1",
            "distinct_devices": len({r["pci_bus"] for r in reports})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra passes (two renders, host frames, K=200)")
    ap.add_argument("--config", choices=["frames640", "objects8", "hd"], default="frames640")
    ap.add_argument("--object-index", type=int, default=-1,
                    help="objects8: ONE object per rank, rank r tracking object (object-index + r) mod 8 of config/*.sh; default "
                         "(-1): all eight objects, dealt round-robin to the ranks and tracked in lock-step per rank")
    ap.add_argument("--extra", choices=["ycb_policy", "ycb_refshape", "r9_phone", "r9_12mp"], default=None,
                    help="run only this extra pass (the reference's own reference-image shapes) and print its record")
    ap.add_argument("--lm-grid", type=int, default=0, help="objects8 lock-step: LM workgroups per problem (0: 256 / K)")
    ap.add_argument("--per-image-plan", action="store_true",
                    help="objects8 lock-step: UNet layers planned per image (maps bit-identical to the one-object tracker)")
    ap.add_argument("--first-frame-sigma", type=float, default=None,
                    help="noise (8-bit levels) of the cold-start frame, which sets the cost gate's threshold (default: 12, "
                         "objects8: 24 - not every config/*.sh box keeps the headline object's margin)")
    ap.add_argument("--groups", type=int, default=2,
                    help="objects8 lock-step: groups of objects with their own stream and batched passes (UNet passes take turns)")
    ap.add_argument("--no-solo", action="store_true", help="objects8 lock-step at N = 1: skip the one-object comparison pass")
    ap.add_argument("--cpu-baseline-frames", type=int, default=0,
                    help="CPU baseline: track exactly this many frames after 3 warm-up frames (BASELINE.md 3 asks for >= 20); "
                         "0 = as many as fit the default ~70 s budget after 1 warm-up frame")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step (poses, cost, flags) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the untimed per-stage and roofline passes, the "
                         "extra passes, the CPU baseline and (objects8) the one-object comparison passes")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_baseline_frames and not args.full:
        ap.error("--cpu-baseline-frames needs --full (a plain run does not run the CPU baseline)")
    if args.dump_outputs and args.extra:
        ap.error("--dump-outputs needs the timed path; --extra runs an extra pass only")
    if args.first_frame_sigma is None:
        args.first_frame_sigma = 24.0 if args.config == "objects8" else 12.0
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))  # plain `python bench.py --gpus N`: spawn the N ranks ourselves

    from pixtrack_amd import parallel
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    # RCCL ("nccl") is the backend of a real multi-GPU run.  PXT_DIST_BACKEND=gloo exists to
    # rehearse the multi-rank control flow (barriers, max-over-ranks, pose gather) on a box with
    # fewer GPUs than ranks: the ranks then share devices and the collectives run on host tensors.
    backend = os.environ.get("PXT_DIST_BACKEND", "nccl")
    rank, ws, local_rank = parallel.init_from_env(backend)
    if ws != max(1, args.gpus):
        raise SystemExit(f"bench.py --gpus {args.gpus} is running with WORLD_SIZE={ws}: the number would be labelled with "
                         "the wrong GPU count (launch with torch.distributed.run --nproc-per-node N, or plain "
                         "`python bench.py --gpus N`, which spawns its own ranks)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm device (no CPU fallback for the product path)")
    n_dev = torch.cuda.device_count()
    if backend == "nccl" and ws > n_dev:
        raise SystemExit(f"{ws} ranks but {n_dev} visible GPUs: RCCL needs one GPU per rank")
    local_rank = local_rank % n_dev
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    coll_dev = dev if backend == "nccl" else torch.device("cpu")
    numa_node = parallel.bind_to_device_numa(local_rank)  # before any pinned allocation
    try:  # best effort: the host thread feeds the GPU launch by launch; a box shared with other jobs can de-schedule it for
        os.nice(-10)  # tens of ms (round 5: one 28-ms frame in a 60-frame window, 1.43 ms every other frame)
    except (OSError, PermissionError):
        pass

    if args.extra:  # one of the extra passes on its own (profiling: scripts/collect_profiles.sh's refshape leg)
        from pixtrack_amd.synthetic import REF_CAMERA_12MP, REF_CAMERA_PHONE

        fn = {"ycb_policy": lambda: ycb_policy_extra(dev), "ycb_refshape": lambda: ycb_policy_extra(dev, refshape=True),
              "r9_phone": lambda: r9_refshape_extra(dev, REF_CAMERA_PHONE, "1920x1440 (4:3 phone frames)"),
              "r9_12mp": lambda: r9_refshape_extra(dev, REF_CAMERA_12MP, "4032x3024 (12-MP stills)", n=34)}[args.extra]
        print(json.dumps({args.extra: fn()}), flush=True)
        return
    if args.config == "hd":
        return run_hd(args, rank, ws, dev, coll_dev, numa_node)
    if args.config == "objects8" and args.object_index < 0 and ws < 8:
        return run_objects8(args, rank, ws, dev, coll_dev, numa_node)
    args.object_index = max(args.object_index, 0)

    # (frames are generated in order from one seeded stream: frame i is the same whatever the number after it)
    n_diag = min(20, args.steps) if args.full else 0  # untimed diagnostic pass (per-stage HIP-event times)
    n_roof = 8 if args.full else 0                    # untimed pass of the per-stage rooflines (UNet TFLOP/s, LM TB/s)
    n_timed_end = args.warmup + args.steps
    extras_on = args.full and ws == 1 and not args.no_extras and args.config == "frames640"
    n_extra = 200 if extras_on else 0
    n_frames = n_timed_end + n_diag + n_roof + n_extra
    unit = parallel.shard_units(ws, rank, ws)[0]  # one sequence per rank, seeds 1002, 1003, ...
    obj = None
    if args.config == "objects8":  # BASELINE configs[3]: one object of the reference's config/*.sh per rank
        objs = parallel.load_object_configs()
        obj = objs[(args.object_index + unit) % len(objs)]
        assets = make_tracking_assets(seed=1002 + unit, width=args.width, height=args.height, n_frames=n_frames,
                                      aabb=obj["aabb"])
    else:
        assets = make_tracking_assets(seed=1002 + unit, width=args.width, height=args.height, n_frames=n_frames)
    tracker = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, tracker.testbed, first_frame_sigma=args.first_frame_sigma)
    names = [f"{i:06d}.png" for i in range(n_frames)]
    torch.cuda.synchronize()

    timer = StageTimer()
    timer.wrap(tracker.testbed, "render_device", "nerf_render")
    timer.wrap(tracker.testbed, "render_both_device", "nerf_render")
    timer.wrap(tracker.testbed, "render_frame_device", "nerf_render")
    timer.wrap(tracker.testbed, "render_frame_pair_device", "nerf_render")
    timer.wrap(tracker.localizer.extractor.model, "forward_packed_batch", "unet")
    timer.wrap(tracker.localizer.refiner, "refine_pose_using_features", "lm")
    timer.wrap(tracker.localizer.refiner, "interp_sparse_observations", "sample")
    tracker.testbed.stats_accum = torch.zeros(4, dtype=torch.int64, device=dev)

    # the frame loop allocates a few hundred small Python objects per frame; a generation-2 collection in the middle of
    # it is a 10 ms stall of the host that feeds the GPU.  Collected and frozen BEFORE the warm-up frames (round 4): done
    # between warm-up and the timed region it left the GPU idle for tens of ms right before the first timed frame, which
    # then ran 0.75 ms slower than every other one (`frame_ms.argmax` = 0 in rounds 1-3: 2.5 % of the driver's K = 20 window).
    import gc

    gc.collect()
    gc.freeze()
    gc.disable()
    for i in range(args.warmup):
        tracker.run_single_frame((names[i], frames[i]))
    torch.cuda.synchronize()
    ref_id_start = tracker.reference_ids[0]  # (the CPU baseline tracks the same first frames with the same reference)
    tracker.testbed.stats_accum.zero_()
    n_renders0 = tracker.testbed.n_renders
    # HIP events around the render-kernel launch (GATHER_KERNEL) of every 4th render: live over the timed
    # region, sampled so that the marker packets do not slow what they measure
    tracker.testbed.timing_enable(4)

    if ws > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frame_t = []
    for i in range(args.warmup, n_timed_end):
        tracker.run_single_frame((names[i], frames[i]))
        frame_t.append(time.perf_counter())  # host-side frame boundaries (each frame ends on its LM result)
    torch.cuda.synchronize()
    if ws > 1:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [tracker], names[n_timed_end - 1])
    frame_ms = np.diff(np.array([t0] + frame_t)) * 1e3
    tracker.testbed.timing_enable(0)
    enc_ms, enc_launches = tracker.testbed.timing_read()
    own_elapsed = elapsed
    elapsed = parallel.max_over_ranks(elapsed, coll_dev)
    report = rank_report(rank, local_rank, dev, numa_node, args.steps, own_elapsed, coll_dev)
    stats = tracker.testbed.stats_accum.cpu().tolist()
    n_renders = tracker.testbed.n_renders - n_renders0
    render_ahead = getattr(tracker, "render_ahead", False)
    roofline_stages = None
    if args.full:
        # Two untimed passes over the next frames of the same sequence.
        # (1) per-stage times: event pairs around every stage cost ~10 % of a frame, so they stay out
        #     of the timed region;
        #     with the tracker's render-ahead off: a render enqueued behind the LM launch would be booked to "lm"
        n_stage = n_diag // 2
        tracker.render_ahead = False
        tracker._ahead_ok = None  # (the render queued behind the last timed frame's LM launch is not used either)
        torch.cuda.synchronize()
        timer.enabled = True
        for i in range(n_timed_end, n_timed_end + n_stage):
            tracker.run_single_frame((names[i], frames[i]))
        torch.cuda.synchronize()
        timer.enabled = False
        for i in range(n_timed_end + n_stage, n_timed_end + n_diag):  # (frames kept in step with the earlier rounds' passes)
            tracker.run_single_frame((names[i], frames[i]))
        torch.cuda.synchronize()
        tracker.render_ahead = render_ahead
        # (3) live rooflines of the other two stages (the UNet is ~47 % of the frame, the LM ~6 %)
        roofline_stages = stage_rooflines(tracker, frames, names, n_timed_end + n_diag, n_timed_end + n_diag + n_roof, dev)

    extras = None
    if extras_on:
        extras = run_extras(tracker, assets, frames, names, args.warmup, n_timed_end, n_timed_end + n_diag + n_roof, dev)

    records = parallel.pack_pose_records(tracker.pose_history, names[args.warmup:n_timed_end])
    gathered = parallel.gather_pose_records(records.to(coll_dev), coll_dev)  # the one collective (RCCL)
    n_ok = int(sum(float(g[:, 12].sum()) for g in gathered))
    total_frames = sum(g.shape[0] for g in gathered)

    if rank != 0:
        return
    stage = timer.totals_ms()
    # dominant kernel: ngp_render_kernel<MODE> - ONE launch per render: persistent waves march their rays, gather the
    # hash-grid features of their samples, run both MLPs on them and composite (since round 6 nothing else runs beside it:
    # the launch's duration is the kernel's own).  ALGORITHMIC bytes per launch = composited samples per render x 512 B
    # (SURVEY 8d); samples a step evaluates past a ray's termination are waste and are not credited.
    enc_avg_ms = enc_ms / max(enc_launches, 1)          # over the timed (sampled) launches
    launches_total = n_renders
    samples_per_launch = stats[0] / max(launches_total, 1)
    achieved = samples_per_launch * NERF_BYTES_PER_SAMPLE / (enc_avg_ms * 1e-3) / 1e9 if enc_avg_ms > 0 else 0.0
    # accuracy vs the synthetic ground truth over the timed frames (reported, not the metric)
    rot_err, tr_err = [], []
    for i in range(args.warmup, n_timed_end):
        ret = tracker.pose_history[names[i]]
        if _tracked(ret):
            Rr, tt = ret["T_refined"].numpy()
            Rg, tg = assets["gt_poses"][i]
            c = np.clip((np.trace(Rr @ Rg.T) - 1) / 2, -1, 1)
            rot_err.append(float(np.arccos(c)))
            tr_err.append(float(np.linalg.norm(tt - tg)))
    # HBM-side traffic of the same kernel from the committed rocprofv3 PMC passes of this command
    # (FETCH_SIZE and WRITE_SIZE need separate runs, so they cannot be taken live here)
    traffic, traffic_src = None, None
    pmc = next((q for q in (ROOT / "profiles" / f"r0{r}_pmc_traffic.json" for r in (6, 5, 4, 3, 2)) if q.exists()), None)
    static_commit = None
    if pmc is not None:
        recs = json.loads(pmc.read_text())
        static_commit = (recs.get("_meta") or {}).get("collected_at_commit") or PROFILE_COMMITS.get(pmc.name[:3])
        rec = recs.get(GATHER_KERNEL_PMC) or recs.get("void " + GATHER_KERNEL_PMC)
        if rec:
            traffic = round((rec["fetch_bytes_per_launch"] + rec["write_bytes_per_launch"]) / 1e6, 2)
            traffic_src = f"profiles/{pmc.name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, raw, MB per launch)"
    # What actually binds the kernel (rocprofv3 TCP / TCC counter passes of this command, scripts/collect_profiles.sh):
    # not HBM bytes - the fabric side moves ~0.35 x the algorithmic bytes - but the L1's miss path: requests to the L2
    # x their latency.  `l2` prices the kernel against the L2's own peak as well.
    l2 = None
    l2f = next((q for q in (ROOT / "profiles" / f"r0{r}_pmc_l2.json" for r in (6, 5, 4, 3)) if q.exists()), None)
    if l2f is not None:
        recs = json.loads(l2f.read_text())
        rec = recs.get(GATHER_KERNEL_PMC) or recs.get("void " + GATHER_KERNEL_PMC)
        if rec and rec.get("TCP_TCC_READ_REQ_sum") and enc_avg_ms > 0:
            req = rec["TCP_TCC_READ_REQ_sum"]
            tbs = req * 64.0 / (enc_avg_ms * 1e-3) / 1e12
            l2 = {"what": "L1 -> L2 read requests of the same kernel (64 B each) per launch over the live launch time",
                  "requests_per_launch": round(req, 1), "achieved": round(tbs, 3), "peak": 34.5, "unit": "TB/s",
                  "frac": round(tbs / 34.5, 4),
                  "mean_request_latency_cycles": (round(rec["TCP_TCC_READ_REQ_LATENCY_sum"] / req, 1)
                                                  if rec.get("TCP_TCC_READ_REQ_LATENCY_sum") else None),
                  "l2_hit_rate": (round(rec["TCC_HIT_sum"] / max(rec["TCC_HIT_sum"] + rec.get("TCC_MISS_sum", 0.0), 1.0), 3)
                                  if rec.get("TCC_HIT_sum") else None),
                  "source": f"profiles/{l2f.name}", "static": True,
                  "static_note": "request counts read from the committed rocprofv3 pass, priced with this run's live launch time",
                  "collected_at_commit": (recs.get("_meta") or {}).get("collected_at_commit") or PROFILE_COMMITS.get(l2f.name[:3])}
    roofline = {"kernel": GATHER_KERNEL, "bound": "hbm", "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                "traffic_unit": "MB per launch", "traffic_source": traffic_src,
                "traffic_static": {"static": True, "collected_at_commit": static_commit,
                                   "note": "FETCH_SIZE / WRITE_SIZE need their own rocprofv3 passes: read from the committed "
                                           "profile, not measured by this run (achieved / frac / avg_launch_ms / samples ARE live)"},
                "algorithmic_mb_per_launch": round(samples_per_launch * NERF_BYTES_PER_SAMPLE / 1e6, 2),
                "avg_launch_ms": round(enc_avg_ms, 5), "launches_timed": enc_launches, "launches": launches_total,
                "samples_per_launch": round(samples_per_launch, 1), "bytes_per_sample": NERF_BYTES_PER_SAMPLE,
                "samples_per_render": round(stats[0] / max(n_renders, 1), 1),
                "rays_in_the_box_per_render": round(stats[1] / max(n_renders, 1), 1),
                "note": ("one launch = one render (a frame's mask + reference image in one march); timed with HIP events on "
                         "the render's own stream over every 4th render of the timed region; nothing runs beside it"),
                "binding_resource": ("VALU issue (~3100 VALU instructions per wave step of 64 sample slots, VALU busy 0.74-0.78 at 3.3 waves "
                                     "per SIMD; the gathers - 7.9 M vector-memory reads per render after the box fetch - come second), "
                                     "NOT HBM bytes: "
                                     "`bound` keeps the contract's hbm|mfma vocabulary and prices the ALGORITHMIC gather bytes "
                                     "against the HBM peak; `traffic` is the fabric side (tables cache-resident), `l2` prices the "
                                     "L2 requests against the L2's peak (DESIGN.md 3.3)"),
                "l2": l2}
    out = {
        "metric": "tracked frames/sec at 640x480 (full NeRF render + UNet + LM loop)",
        "value": round(total_frames / elapsed, 3),
        "unit": "frames/s",
        "n_gpus": ws,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp16 storage / fp32 accumulate (UNet, NeRF MLPs); fp32 (LM)",
        "data": "synthetic (seeded hash-grid NeRF, He-init UNet, NeRF-rendered query frames + noise)",
        "config": {"workload": ("configs[1]: premier_protein-style object, 640x480, full NeRF render + UNet + LM loop, "
                                "1 sequence per GPU" if obj is None else
                                f"configs[3]: one object of config/*.sh per GPU (rank {rank}: {obj['name']}, OBJ_AABB {obj['OBJ_AABB']}), "
                                "640x480, full loop"), "width": args.width, "height": args.height, "spp": 8,
                   "n_points_per_reference": int(tracker.localizer.refiner._points_of(tracker.reference_ids)[1].shape[0]),
                   "parallelism": f"{ws} independent sequence(s), 1 process/GPU, final RCCL all_gather of poses",
                   "mask_and_reference_render_fused": bool(tracker._views_coincide()),
                   "next_render_enqueued_behind_lm": bool(render_ahead),
                   "renders_ahead_used": int(getattr(tracker, "renders_ahead_used", 0)),
                   "host_numa_node": numa_node},
        "tracked_ok": n_ok,
        "frames_total": total_frames,
        "mean_rot_err_vs_gt_rad": round(float(np.mean(rot_err)), 6) if rot_err else None,
        "mean_trans_err_vs_gt": round(float(np.mean(tr_err)), 6) if tr_err else None,
        "frame_ms": {"p50": round(float(np.percentile(frame_ms, 50)), 4), "p90": round(float(np.percentile(frame_ms, 90)), 4),
                     "max": round(float(frame_ms.max()), 4), "argmax": int(frame_ms.argmax())},
        "roofline": roofline,
        "full": bool(args.full),
        **report,
    }
    if args.full:
        out["stage_ms_per_frame"] = {k: round(v[0] / max(n_diag // 2, 1), 4) for k, v in stage.items()}
        out["stage_ms_note"] = (f"HIP-event times of a separate untimed pass over the next {n_diag // 2} frames; `unet` ends when "
                                "the reference pass ends on the caller's stream - the query pass is joined behind the sparse "
                                "sampling (deferred join), so its last ~20-40 us are booked to `sample` / `lm`")
        out["roofline_stages"] = roofline_stages
    # other kernels' utilisation from the committed rocprofv3 SQ counter pass of this command
    # (profiles/r02_pmc_sq.json; scripts/pmc_sq_summary.py): matrix-pipe busy of the UNet convolutions,
    # VALU busy of the march (a serial DDA per ray: latency- and tail-bound, not VALU-bound)
    sq = next((q for q in (ROOT / "profiles" / f"r0{r}_pmc_sq.json" for r in (6, 5, 4, 3, 2)) if q.exists()), None)
    if sq is not None:
        rec = json.loads(sq.read_text())
        pick = {}
        for name, r in rec.items():
            if name == "_meta":
                continue
            if "conv3x3_v" in name or "ngp_r" in name or "lm_refine" in name:
                pick[name.replace("void pxt::", "").replace("pxt::", "")] = {
                    k: round(r[k], 4) for k in ("mfma_busy", "valu_busy", "mean_waves_per_simd") if k in r}
        out["kernel_utilisation"] = {"source": f"profiles/{sq.name} (rocprofv3 --pmc SQ_*, same command)", "static": True,
                                     "collected_at_commit": (rec.get("_meta") or {}).get("collected_at_commit")
                                     or PROFILE_COMMITS.get(sq.name[:3]), "kernels": pick}
    if extras is not None:
        out["extras"] = extras
    if args.full and not args.no_cpu_baseline and ws == 1:
        try:
            if args.cpu_baseline_frames > 0:  # BASELINE.md 3 to the letter: 3 warm-up frames, then exactly this many
                out["cpu_baseline"] = cpu_baseline(assets, frames, args.warmup, ref_id_start, budget_s=1e9,
                                                   max_frames=args.cpu_baseline_frames, min_frames=args.cpu_baseline_frames,
                                                   warmup_frames=3)
            else:
                out["cpu_baseline"] = cpu_baseline(assets, frames, args.warmup, ref_id_start)
        except Exception as e:  # the baseline is a report, never a reason to lose the GPU number
            out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port",
                                   "sample": f"failed: {e!r}"}
    else:
        out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port",
                               "sample": "timed on rank 0 at N=1 only" if args.full or ws > 1 else "not run: `--full` runs it"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
