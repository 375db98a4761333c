"""The opt-in per-point residual report of the trackers (``point_report="summary" | "full"`` / ``--point_report``): with
the option off nothing changes and pxt_lm_point_report is never called; with it on every LM launch is followed by one
report problem, poses stay bit-identical, and a frame's history entry says how many points carried the pose
(the kernel itself is held to the oracle by tests/test_point_report_gpu.py)."""
import pickle

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd.point_report import POINT_KEYS, SUMMARY_KEYS
from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 6
NAMES = [f"{i:06d}.png" for i in range(N)]
_SHARED = {}


class CallCounter:
    """Wraps the binding's pxt_lm_point_report entry and counts the calls."""

    def __init__(self, monkeypatch):
        self.calls = 0
        L = _lib.lib()
        real = L.pxt_lm_point_report

        def counted(*a):
            self.calls += 1
            return real(*a)

        monkeypatch.setattr(L, "pxt_lm_point_report", counted, raising=False)


def _assets(seed=1002):
    key = ("assets", seed)
    if key not in _SHARED:
        _SHARED[key] = make_tracking_assets(seed=seed, width=W, height=H, n_frames=N)
    return _SHARED[key]


def _tracker(device, seed=1002, debug=0, lm_grid=0, **kw):
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=debug, device=device, assets=_assets(seed), **kw)
    if lm_grid:
        for opt in tr.localizer.optimizer:
            opt.conf.n_workgroups = lm_grid
    return tr


def _frames(tr, seed=1002):
    key = ("frames", seed)
    if key not in _SHARED:
        _SHARED[key] = render_query_frames(_assets(seed), tr.testbed)
    return _SHARED[key]


def _run(device, key, n=N, seed=1002, **kw):
    """(history, tracker) of a run over the first ``n`` frames, computed once per key."""
    if key not in _SHARED:
        tr = _tracker(device, seed=seed, **kw)
        frames = _frames(tr, seed)
        for i in range(n):
            tr.run_single_frame((NAMES[i], frames[i]))
        torch.cuda.synchronize()
        _SHARED[key] = (tr.pose_history, tr)
    return _SHARED[key]


def _row(ret):
    T = ret["T_refined"] if ret.get("success") else ret["T_init"]
    return np.concatenate([T.as12().double().numpy().reshape(-1), [float(bool(ret.get("success"))), float(ret["tracked"]),
                                                                   float(ret["cost"])]])


def _check_entry(ret, full, n_points=None):
    assert set(SUMMARY_KEYS) <= set(ret)
    assert ("point_report" in ret) == full
    if not ret["success"]:
        assert all(ret[k] is None for k in SUMMARY_KEYS)
        return
    assert 0 < ret["n_inliers"] <= ret["n_valid_points"]
    assert ret["inlier_ratio"] == ret["n_inliers"] / ret["n_valid_points"]
    assert 0.0 < ret["mean_robust_weight"] <= 1.0
    assert set(ret["rejected_points"]) == {"masked", "projection", "border"}
    if full:
        rep = ret["point_report"]
        assert set(rep) == set(POINT_KEYS)
        n = len(rep["valid"])
        assert n_points is None or n == n_points
        assert all(len(rep[k]) == n for k in POINT_KEYS) and rep["p2d"].shape == (n, 2)
        assert int(rep["valid"].sum()) == ret["n_valid_points"]
        assert n == ret["n_valid_points"] + sum(ret["rejected_points"].values())
        assert int((rep["robust_weight"][rep["valid"]] >= 0.5).sum()) == ret["n_inliers"]
        for code, name in enumerate(("masked", "projection", "border"), 1):
            assert int((rep["reject"] == code).sum()) == ret["rejected_points"][name]


def test_off_summary_and_full(device, monkeypatch):
    counter = CallCounter(monkeypatch)
    off, tr_off = _run(device, "off")
    assert counter.calls == 0 and tr_off.localizer.refiner._report_ws is None
    rows = {"off": np.stack([_row(off[nm]) for nm in NAMES])}
    for nm in NAMES:
        assert not ((set(SUMMARY_KEYS) | {"point_report"}) & set(off[nm]))
    for mode in ("summary", "full"):
        before, fresh = counter.calls, mode not in _SHARED
        hist, tr = _run(device, mode, point_report=mode)
        if fresh:
            assert counter.calls - before == N + 1  # one call per LM launch: the cold start makes two
        rows[mode] = np.stack([_row(hist[nm]) for nm in NAMES])
        refiner = tr.localizer.refiner
        for nm in NAMES:
            _check_entry(hist[nm], mode == "full")
        assert (refiner.last_point_report["points"] is not None) == (mode == "full")
        assert refiner.last_point_report["level"] == 0  # image scale 1, finest level
        if mode == "full":
            rep = hist[NAMES[-1]]["point_report"]
            assert len(rep["valid"]) == int(refiner.last_point_report["points"].shape[0])
    assert np.array_equal(rows["off"].view(np.uint64), rows["summary"].view(np.uint64))
    assert np.array_equal(rows["off"].view(np.uint64), rows["full"].view(np.uint64))
    # summary and full agree on the summary keys
    s, f = _SHARED["summary"][0], _SHARED["full"][0]
    for nm in NAMES:
        assert all(s[nm][k] == f[nm][k] for k in SUMMARY_KEYS), nm
    assert any(off[nm]["tracked"] for nm in NAMES[1:])


def test_both_reference_point_settings_and_the_debug_tracker(device):
    # "sfm": the arrays cover the SfM points of the reference image the frame was refined on
    hist, tr = _run(device, "full", point_report="full")
    refiner = tr.localizer.refiner
    for nm in NAMES:
        ret = hist[nm]
        if ret["success"]:
            n_ref = len(refiner._points_of(ret["dbids"])[0])
            assert len(ret["point_report"]["valid"]) == n_ref
    # "render": the lattice slots of the frame's own depth render; ids are slot indices; debug >= 2 keeps the point set
    hist, tr = _run(device, "render-full", point_report="full", reference_points="render", debug=2)
    slots = int(tr.localizer.refiner.conf.reference_points_max)
    ok = 0
    for nm in NAMES:
        ret = hist[nm]
        _check_entry(ret, True, slots)
        if not ret["success"]:
            continue
        ok += 1
        # unused slots are masked out by the refinement's own slot mask
        assert ret["rejected_points"]["masked"] >= slots - ret["n_reference_points"]
        dbg = tr.pose_tracker_history[nm]
        assert dbg.p3d_ids == list(range(slots)) and dbg.p3d.shape == (slots, 3)
        assert dbg.point_report is ret["point_report"]
    assert ok >= N - 1
    back = pickle.loads(pickle.dumps(tr.pose_tracker_history[NAMES[-1]]))
    assert set(back.point_report) == set(POINT_KEYS) and back.p3d.shape == (slots, 3)
    # debug < 2: the DebugTracker keeps nothing
    _h, tr0 = _run(device, "full", point_report="full")
    assert tr0.pose_tracker_history[NAMES[-1]].point_report is None and tr0.pose_tracker_history[NAMES[-1]].p3d is None


def test_lockstep_summaries_equal_solo_runs(device, monkeypatch):
    """The bit-identical configuration of tests/test_multi_object_gpu.py (per-image UNet plan, solo LM grid of 32): each
    object's summary equals its one-object run's; a lock-step step makes ONE pxt_lm_point_report call."""
    counter = CallCounter(monkeypatch)
    seeds = [1002, 1003]
    solo = [_run(device, ("solo", s), seed=s, lm_grid=32, point_report="summary")[0] for s in seeds]
    trackers = [_tracker(device, seed=s, lm_grid=32) for s in seeds]
    multi = MultiObjectTracker(trackers, lm_workgroups=32, per_image_plan=True, n_groups=1, point_report="summary")
    assert all(tr.localizer.refiner.point_report == "summary" for tr in trackers)
    frames = [_frames(trackers[j], s) for j, s in enumerate(seeds)]
    lockstep_steps = 0
    for i in range(N):
        before, steps = counter.calls, multi.lockstep_frames
        multi.run_single_frames([(NAMES[i], frames[j][i]) for j in range(len(seeds))])
        if multi.lockstep_frames - steps == len(seeds):  # both objects went through the batched step
            assert counter.calls - before == 1
            lockstep_steps += 1
    torch.cuda.synchronize()
    assert lockstep_steps >= 1
    for j, tr in enumerate(trackers):
        for nm in NAMES:
            got, want = tr.pose_history[nm], solo[j][nm]
            assert np.array_equal(_row(got).view(np.uint64), _row(want).view(np.uint64)), (j, nm)
            for k in SUMMARY_KEYS:
                assert got[k] == want[k], (j, nm, k, got[k], want[k])


def test_an_occluded_block_lowers_the_weights_of_the_points_under_it(device):
    """Seeded uniform noise over a quarter of the bounding box of the object's points in one steady frame: the points
    under the block keep less robust weight than the others, and the frame's inlier ratio drops."""
    k = 3
    clean, _tr = _run(device, "full", point_report="full")
    ref = clean[NAMES[k]]
    assert ref["tracked"] and clean[NAMES[k - 1]]["tracked"]
    rep = ref["point_report"]
    p = rep["p2d"][rep["valid"]]
    x0, y0, x1, y1 = p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()
    bx1, by1 = int(round(x0 + 0.5 * (x1 - x0))), int(round(y0 + 0.5 * (y1 - y0)))  # the top-left quarter of the box
    bx0, by0 = int(np.floor(x0)), int(np.floor(y0))
    tr = _tracker(device, point_report="full")
    frames = _frames(tr)
    for i in range(k):
        tr.run_single_frame((NAMES[i], frames[i]))
    img = frames[k].clone()
    g = torch.Generator().manual_seed(5)
    noise = torch.randint(0, 256, (by1 - by0, bx1 - bx0, img.shape[2]), generator=g)
    img[by0:by1, bx0:bx1] = noise.to(img.device, img.dtype)
    tr.run_single_frame((NAMES[k], img))
    torch.cuda.synchronize()
    got = tr.pose_history[NAMES[k]]
    assert got["success"]
    r = got["point_report"]
    v, q = r["valid"], r["p2d"]
    inside = v & (q[:, 0] >= bx0) & (q[:, 0] < bx1) & (q[:, 1] >= by0) & (q[:, 1] < by1)
    outside = v & ~inside
    assert inside.sum() >= 10 and outside.sum() >= 10
    w_in, w_out = float(r["robust_weight"][inside].mean()), float(r["robust_weight"][outside].mean())
    print("occlusion: mean robust weight inside", w_in, "outside", w_out, "inlier ratio painted", got["inlier_ratio"],
          "clean", ref["inlier_ratio"])
    assert w_in < w_out
    assert got["inlier_ratio"] < ref["inlier_ratio"]
