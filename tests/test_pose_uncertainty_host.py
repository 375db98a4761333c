"""Host side of the pose-uncertainty option (no GPU): the adjoint, the record algebra of pixtrack_amd/uncertainty.py, the
struct mirror of pxt_lm_info_problem and the registration of torch.ops.pixtrack.lm_information."""
import ctypes
import subprocess
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd.geometry import Pose, se3_exp, so3exp_map, to_object_frame
from pixtrack_amd.uncertainty import (covariance_from_record, frame_entries, information_from_record, observability)

ROOT = Path(__file__).resolve().parent.parent
IU = np.triu_indices(6)


def _random_pose(g):
    return Pose.from_Rt(so3exp_map(torch.randn(3, dtype=torch.float64, generator=g)),
                        torch.randn(3, dtype=torch.float64, generator=g))


def _record(H, g=None, n_valid=500.0, wr2=3.0, flag=1.0):
    rec = np.zeros(48)
    rec[0], rec[1], rec[2], rec[3] = 1.0, n_valid, wr2, 10.0
    rec[4:10] = np.zeros(6) if g is None else g
    rec[10:31] = np.asarray(H)[IU]
    rec[47] = flag
    return rec


def test_adjoint_moves_a_left_perturbation_to_the_right():
    g = torch.Generator().manual_seed(5)
    for _ in range(50):
        T = _random_pose(g)
        xi = torch.randn(6, dtype=torch.float64, generator=g) * 0.7
        left = se3_exp(xi) @ T
        right = T @ se3_exp(T.inv().adjoint() @ xi)
        assert float((left.as12() - right.as12()).abs().max()) < 1e-12
    # ... and for a tiny rotation (the series branch of the exponential)
    T = _random_pose(g)
    xi = torch.tensor([0.3, -0.2, 0.1, 1e-9, -2e-9, 1e-9], dtype=torch.float64)
    assert float(((se3_exp(xi) @ T).as12() - (T @ se3_exp(T.inv().adjoint() @ xi)).as12()).abs().max()) < 1e-12


def test_object_frame_information_and_covariance_are_consistent():
    g = torch.Generator().manual_seed(9)
    T = _random_pose(g)
    A = np.random.default_rng(2).normal(size=(6, 6))
    H = A @ A.T + 6 * np.eye(6)
    Ho = to_object_frame(H, T)
    So = to_object_frame(np.linalg.inv(H), T, covariance=True)
    np.testing.assert_allclose(Ho @ So, np.eye(6), atol=1e-9)
    xo = np.random.default_rng(3).normal(size=6)
    xc = T.adjoint().numpy() @ xo  # the same perturbation, camera frame
    assert xo @ Ho @ xo == pytest.approx(xc @ H @ xc, rel=1e-12)


def test_covariance_inverts_a_known_spd_matrix():
    A = np.random.default_rng(0).normal(size=(6, 6))
    H = A @ A.T + np.diag([1, 2, 3, 4, 5, 6.0])
    g = np.arange(6.0)
    rec = _record(H, g, n_valid=400.0, wr2=7.5)
    g2, H2 = information_from_record(rec)
    np.testing.assert_array_equal(g2, g)
    np.testing.assert_allclose(H2, H, rtol=0, atol=0)
    cov, flag = covariance_from_record(rec, 32)
    sigma0_2 = 7.5 / (32 * 400.0 - 6)
    assert flag == "ok"
    np.testing.assert_allclose(cov @ H, sigma0_2 * np.eye(6), atol=1e-12 * sigma0_2 * 1e3)
    np.testing.assert_allclose(cov, sigma0_2 * np.linalg.inv(H), rtol=1e-10)
    np.testing.assert_allclose(cov, cov.T, rtol=0, atol=1e-18)


def test_singular_indefinite_and_skipped_records_give_none_and_a_flag():
    B = np.random.default_rng(1).normal(size=(6, 5))
    H5 = B @ B.T  # rank 5
    cov, flag = covariance_from_record(_record(H5), 128)
    assert cov is None and flag == "singular"
    Hneg = np.diag([1.0, 1, 1, 1, 1, -1e-3])
    cov, flag = covariance_from_record(_record(Hneg), 128)
    assert cov is None and flag == "singular"
    cov, flag = covariance_from_record(_record(np.eye(6), flag=-1.0), 128)
    assert cov is None and flag == "skipped"
    cov, flag = covariance_from_record(_record(np.eye(6), flag=-2.0), 128)
    assert cov is None and flag == "too_few_points"
    cov, flag = covariance_from_record(_record(np.eye(6), n_valid=0.0), 32)
    assert cov is None and flag == "dof"
    ent = frame_entries(_record(np.eye(6), flag=-1.0), 32, 0, Pose(torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).double()),
                        np.zeros((4, 3)))
    assert set(ent) == {"pose_info", "pose_cov", "observability", "info_level", "info_n_valid"}
    assert all(v is None for v in ent.values())


def test_observability_names_the_planted_weak_direction():
    g = torch.Generator().manual_seed(11)
    T = _random_pose(g)
    rng = np.random.default_rng(4)
    p3d = rng.normal(size=(500, 3)) * 0.05 + np.array([0.3, -0.1, 0.2])
    l = float(np.median(np.linalg.norm(p3d - p3d.mean(0), axis=1)))
    S = np.diag([l, l, l, 1, 1, 1.0])
    # object-frame scaled information with one weak direction d (unit, scaled coordinates)
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    lam = np.array([1e-4, 1.0, 2.0, 3.0, 4.0, 5.0])
    Hs = Q @ np.diag(lam) @ Q.T
    Ho = np.linalg.inv(S) @ Hs @ np.linalg.inv(S)
    Ainv = T.inv().adjoint().numpy()
    H = Ainv.T @ Ho @ Ainv  # back to the camera frame: to_object_frame(H, T) == Ho
    np.testing.assert_allclose(to_object_frame(H, T), Ho, rtol=1e-9, atol=1e-12)
    obs = observability(H, T, p3d, sigma0=2.0)
    want = S @ Q[:, 0]
    want /= np.linalg.norm(want)
    assert abs(float(obs["weakest_direction"] @ want)) > 1 - 1e-9
    assert np.linalg.norm(obs["weakest_direction"]) == pytest.approx(1.0)
    assert obs["condition"] == pytest.approx(5.0 / 1e-4, rel=1e-6)
    assert obs["weakest_sigma"] == pytest.approx(2.0 / np.sqrt(1e-4), rel=1e-6)
    assert obs["scale"] == pytest.approx(l)


def test_info_problem_struct_matches_the_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "pixtrack_hip.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(pxt_lm_info_problem), offsetof(pxt_lm_info_problem, level),
                 offsetof(pxt_lm_info_problem, pose), offsetof(pxt_lm_info_problem, out), sizeof(pxt_lm_level),
                 PXT_LM_INFO_RECORD, PXT_LM_INFO_MAX_PROBLEMS);
          return 0;
        }
        """
    )
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = [int(x) for x in subprocess.check_output([str(Path(d) / "s")]).decode().split()]
    P = _lib.LmInfoProblem
    assert got == [ctypes.sizeof(P), P.level.offset, P.pose.offset, P.out.offset, ctypes.sizeof(_lib.LmLevel),
                   _lib.PXT_LM_INFO_RECORD, _lib.PXT_LM_INFO_MAX_PROBLEMS]
    assert "pxt_lm_information" in _lib.PROTOTYPES and "pxt_lm_information_workspace_bytes" in _lib.PROTOTYPES


def test_op_is_registered_and_refuses_cpu_tensors():
    from pixtrack_amd import ops

    assert "lm_information" in ops.op_names()
    schema = str(torch.ops.pixtrack.lm_information.default._schema)
    assert "pose_is_lm_record" in schema and "records" in schema
    with pytest.raises((RuntimeError, NotImplementedError, _lib.PxtError)):
        torch.ops.pixtrack.lm_information([torch.zeros(20, 3)], [None], [torch.zeros(8, 8, 36)], [torch.zeros(20, 36)], [32],
                                          [8.0, 8, 10, 10, 4, 4, 0, 0, 0, 0], [0], [torch.zeros(12)], False, 1, 2, 0.0, 0.1,
                                          10, [torch.zeros(48)], torch.zeros(1 << 16, dtype=torch.uint8))


def test_trackers_take_the_option():
    import inspect

    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB

    for cls in (PixLocPoseTrackerR9, PixLocPoseTrackerYCB):
        assert inspect.signature(cls.__init__).parameters["uncertainty"].default is False
    assert inspect.signature(MultiObjectTracker.__init__).parameters["uncertainty"].default is None
