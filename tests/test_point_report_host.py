"""Host-side checks of the opt-in per-point residual report (no GPU): the C ABI, the binding, the op, the command lines,
the option's validation and the decoders of pixtrack_amd/point_report.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import _build, _lib, ops, point_report

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("pxt_lm_point_report", "pxt_lm_point_report_workspace_bytes")


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pixtrack_hip.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.PROTOTYPES
    for macro, value in (("PXT_LM_POINT_RECORD", 8), ("PXT_LM_REPORT_SUMMARY", 16), ("PXT_LM_REPORT_MAX_PROBLEMS", 64)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
        assert getattr(_lib, macro) == value
    assert "pxt_lm_report_problem" in text
    _build.build(verbose=False)
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
    assert (_build.CSRC / "pxt_lm_report.hip").exists()


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 13
    assert _lib.lib().pxt_version() == 13


def test_op_is_registered():
    import torch

    assert "lm_point_report" in ops.op_names()
    s = str(torch.ops.pixtrack.lm_point_report.default._schema)
    assert "points" in s and "Tensor(b!)[] summaries" in s and "float[] inlier_weights" in s


def test_workspace_bytes_refuses_problem_counts_out_of_range():
    L = _lib.lib()
    assert int(L.pxt_lm_point_report_workspace_bytes(0)) < 0
    assert int(L.pxt_lm_point_report_workspace_bytes(65)) < 0
    assert int(L.pxt_lm_point_report_workspace_bytes(1)) > 0
    assert int(L.pxt_lm_point_report_workspace_bytes(64)) > int(L.pxt_lm_point_report_workspace_bytes(1))


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess

    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pixtrack_hip.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pxt_lm_report_problem), '
                                  'offsetof(pxt_lm_report_problem, inlier_weight), offsetof(pxt_lm_report_problem, points), '
                                  'offsetof(pxt_lm_report_problem, summary)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    P = _lib.LmReportProblem
    assert got == [ctypes.sizeof(P), P.inlier_weight.offset, P.points.offset, P.summary.offset]


def test_both_command_lines_parse_the_flag():
    from pixtrack_amd.pose_trackers import multi_object_tracker as multi_cli
    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as r9_cli

    base = ["--object_path", "o", "--query", "q", "--out_dir", "d"]
    for cli in (r9_cli, multi_cli):
        p = cli.build_parser()
        assert p.parse_args(base).point_report == "off"
        for mode in ("off", "summary", "full"):
            assert p.parse_args(base + ["--point_report", mode]).point_report == mode
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--point_report", "everything"])


def test_a_bad_value_raises_before_anything_is_built():
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB

    # (no assets, no paths, no device: anything that got as far as building would fail differently)
    with pytest.raises(ValueError, match="point_report"):
        PixLocPoseTrackerR9("", "", "", "/tmp", point_report="everything")
    with pytest.raises(ValueError, match="point_report"):
        PixLocPoseTrackerR9("", "", "", "/tmp", point_report=True)
    with pytest.raises(ValueError, match="point_report"):
        PixLocPoseTrackerYCB("", "", "/tmp", "obj", point_report="points")
    with pytest.raises(ValueError, match="point_report"):
        MultiObjectTracker([object()], point_report="everything")
    assert point_report.parse_mode(None) is False and point_report.parse_mode("off") is False
    assert point_report.parse_mode(False) is False
    assert point_report.parse_mode("summary") == "summary" and point_report.parse_mode("full") == "full"


def test_summary_decoder():
    s = np.zeros(16, np.float32)
    s[:8] = [12.5, 40, 30, 6.0, 8.0, 3, 2, 5]
    s[15] = 1.0
    d = point_report.decode_summary(s)
    assert d["n_valid_points"] == 40 and d["n_inliers"] == 30
    assert d["inlier_ratio"] == 0.75 and d["mean_robust_weight"] == 0.75
    assert d["rejected"] == {"masked": 3, "projection": 2, "border": 5}
    assert d["cost_sum"] == 12.5 and d["status"] == 1.0
    e = point_report.frame_entries(s)
    assert set(e) == set(point_report.SUMMARY_KEYS)
    assert e["rejected_points"] == d["rejected"] and e["inlier_ratio"] == 0.75
    # no valid point: the ratios are None, the counts stay numbers
    z = np.zeros(16, np.float32)
    z[5], z[15] = 7, -2.0
    d = point_report.decode_summary(z)
    assert d["n_valid_points"] == 0 and d["n_inliers"] == 0
    assert d["inlier_ratio"] is None and d["mean_robust_weight"] is None
    assert d["rejected"]["masked"] == 7 and d["status"] == -2.0
    # no refinement at all
    e = point_report.frame_entries(None, None, full=True)
    assert set(e) == set(point_report.SUMMARY_KEYS) | {"point_report"} and all(v is None for v in e.values())
    with pytest.raises(ValueError):
        point_report.decode_summary(np.zeros(48))


def test_points_decoder():
    nan = np.nan
    pts = np.array([[1, 10.5, 20.25, 0.02, 0.011, 0.5, 0.3, 0],
                    [0, 11.0, 21.0, 0, 0, 0, 0, 1],
                    [0, nan, nan, 0, 0, 0, 0, 2],
                    [0, -4.0, 300.0, 0, 0, 0, 0, 3]], np.float32)
    d = point_report.decode_points(pts)
    assert set(d) == set(point_report.POINT_KEYS)
    assert d["valid"].tolist() == [True, False, False, False] and d["valid"].dtype == bool
    assert d["reject"].tolist() == [0, 1, 2, 3] and d["reject"].dtype == np.uint8
    assert d["p2d"].shape == (4, 2) and d["p2d"][0].tolist() == [10.5, 20.25] and np.isnan(d["p2d"][2]).all()
    assert d["cost"][0] == np.float32(0.02) and d["rho"][0] == np.float32(0.011)
    assert d["robust_weight"][0] == 0.5 and d["confidence"][0] == np.float32(0.3)
    e = point_report.frame_entries(np.r_[np.zeros(15), 1.0], d, full=True)
    assert e["point_report"] is d
    import torch

    assert np.array_equal(point_report.decode_points(torch.from_numpy(pts))["reject"], d["reject"])
    with pytest.raises(ValueError):
        point_report.decode_points(np.zeros((3, 7)))


def test_the_inlier_weight_is_a_documented_convention():
    from pixtrack_amd.refiner import PoseTrackerRefiner

    assert PoseTrackerRefiner.default_config["point_report_inlier_weight"] == point_report.DEFAULT_INLIER_WEIGHT == 0.5
    # barron, alpha 0: rho'(y) = 2 / (y + 2) is 0.5 at y = |r|^2 / scale^2 = 2
    assert 2.0 / (2.0 + 2.0) == 0.5
