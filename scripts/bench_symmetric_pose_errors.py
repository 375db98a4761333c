"""Measurements of the symmetry-aware pose errors -> profiles/r13_symmetric_pose_errors.json.

  (gpu)  time of one pxt_symmetric_pose_errors call (both launches) for (F, V, S) = (200, 2620, 1), (200, 65536, 1),
         (200, 65536, 630): HIP events around 20 calls with the host parked ahead of the stream, median of 7.  Per case:
         transform-project-compare triples per second (F * S * V per call) and the fraction of the fp32 VALU peak,
         counting 55.5 VALU instructions per triple (the inner loop's ISA) against MI355X's 157.3 TFLOPS vector fp32 peak
         taken as 78.65e12 VALU lane-operations per second (the TFLOPS figure counts a multiply-add as two).
  (host) wall time of evaluation.symmetric_pose_errors_host (float64 numpy) on a slice of each case's frames
         (--host_frames), scaled linearly to F.  Needs no GPU.

    python scripts/bench_symmetric_pose_errors.py [--parts gpu,host] [--host_frames 20,2,1] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pixtrack_amd import evaluation as E, symmetry as SY  # noqa: E402

CASES = ((200, 2620, 1), (200, 65536, 1), (200, 65536, 630))
VALU_OPS_PER_TRIPLE = 55.5
PEAK_VALU_OPS = 157.3e12 / 2  # lane-operations per second: the vector fp32 peak counts an FMA as 2 FLOP
KMAT = (600.0, 600.0, 319.5, 239.5)
OFFSET = np.array([0.3, -0.1, 0.5])


def make_case(F, V, S, seed=13):
    """A Gaussian cloud of diameter ~0.2 away from the origin, the set (identity, or an axis through the cloud times a
    flip) and F (estimate, ground truth) pose pairs a few degrees and millimetres apart, up to a member of the set."""
    rng = np.random.default_rng(seed + V)
    v = rng.normal(size=(V, 3)) * 0.03 + OFFSET
    if S == 1:
        sym = SY.symmetry_transforms()
    else:
        Rx = SY.rotation([1, 0, 0], np.pi)
        flip = np.eye(4)
        flip[:3, :3], flip[:3, 3] = Rx, OFFSET - Rx @ OFFSET
        sym = SY.symmetry_transforms([flip], [dict(axis=[0, 0, 1], offset=list(OFFSET))])
    assert len(sym) == S
    T_gt, T_est = np.tile(np.eye(4), (F, 1, 1)), np.tile(np.eye(4), (F, 1, 1))
    for k in range(F):
        T_gt[k, :3, :3] = SY.rotation(rng.normal(size=3), rng.uniform(0, np.pi))
        T_gt[k, :3, 3] = np.r_[rng.uniform(-0.3, 0.3, 2), rng.uniform(1.5, 3)]
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = SY.rotation(rng.normal(size=3), rng.uniform(0, 0.05)), rng.normal(size=3) * 0.005
        T_est[k] = T_gt[k] @ sym[(7 * k) % S] @ D
    return v, sym, T_est, T_gt


def part_gpu():
    import torch

    from pixtrack_amd import _lib

    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    rows = []
    for F, V, S in CASES:
        v, sym, T_est, T_gt = make_case(F, V, S)
        c = v.mean(axis=0)
        verts = torch.from_numpy((v - c).astype(np.float32)).to(dev)
        syms = torch.from_numpy(SY.centred_12(sym, c).astype(np.float32)).to(dev)
        frames = torch.from_numpy(E.symmetric_frames(T_est, T_gt, c, np.tile(KMAT, (F, 1)))).to(dev)
        rec = torch.zeros(F, 8, device=dev)
        need = int(L.pxt_symmetric_pose_errors_workspace_bytes(F, S, V))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def launch():
            rc = L.pxt_symmetric_pose_errors(verts.data_ptr(), V, syms.data_ptr(), S, frames.data_ptr(), F, rec.data_ptr(),
                                             ws.data_ptr(), stream)
            assert rc == 0, rc

        per, ms = 20, []
        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(2_000_000)  # park the host ahead: the launches queue up behind a sleep
            e0.record()
            for _ in range(per):
                launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        t = float(np.median(ms)) * 1e-3
        triples = F * S * V / t
        r = rec.cpu().numpy()
        rows.append({"F": F, "V": V, "S": S, "workspace_bytes": need, "ms_per_call_median": t * 1e3, "ms_min": float(min(ms)),
                     "ms_max": float(max(ms)), "triples_per_s": triples, "valu_ops_per_triple": VALU_OPS_PER_TRIPLE,
                     "peak_valu_ops_per_s": PEAK_VALU_OPS,
                     "fraction_of_fp32_valu_peak": triples * VALU_OPS_PER_TRIPLE / PEAK_VALU_OPS,
                     "mssd_mean": float(r[:, 0].mean()), "mspd_mean": float(r[:, 2].mean())})
        print(rows[-1], flush=True)
    return {"peak": "157.3 TFLOPS vector fp32 (MI355X_MICROARCH) = 78.65e12 VALU lane-operations/s", "cases": rows}


def part_host(host_frames):
    rows = []
    for (F, V, S), n in zip(CASES, host_frames):
        n = min(n, F)
        v, sym, T_est, T_gt = make_case(F, V, S)
        t0 = time.perf_counter()
        e3, e2 = E.symmetric_pose_errors_host(T_est[:n], T_gt[:n], v, KMAT, sym)
        dt = time.perf_counter() - t0
        rows.append({"F": F, "V": V, "S": S, "frames_run": n, "seconds_run": dt, "seconds_for_F_frames": dt * F / n,
                     "scaled_linearly": n != F, "mssd_of_frame_0": float(e3[0].min()), "mspd_of_frame_0": float(e2[0].min())})
        print(rows[-1], flush=True)
    return {"what": "evaluation.symmetric_pose_errors_host (numpy float64, one process)", "cpus": os.cpu_count(),
            "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="gpu,host")
    ap.add_argument("--host_frames", default="20,2,1")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_symmetric_pose_errors.json"))
    args = ap.parse_args()
    path = Path(args.out)
    result = json.loads(path.read_text()) if path.exists() else {}
    host_frames = [int(x) for x in args.host_frames.split(",")]
    for part, fn in (("gpu", part_gpu), ("host", lambda: part_host(host_frames))):
        if part in args.parts.split(","):
            result[part] = fn()
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1))
    print(json.dumps({k: "done" for k in result}))


if __name__ == "__main__":
    main()
