"""Host side of the pose-error evaluation (pixtrack_amd/evaluation.py: relative_poses, auc, accuracy_under, the vertex
readers, the command line) - everything that needs no GPU.  The kernel is tests/test_pose_errors_gpu.py's."""
import numpy as np
import pytest

from pixtrack_amd import evaluation as E


def _random_poses(rng, n):
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[k, :3, :3] = q * np.sign(np.linalg.det(q))
        out[k, :3, 3] = rng.normal(size=3) * 2.0
    return out


def _apply(rel12, u):
    R, t = rel12[:9].reshape(3, 3), rel12[9:]
    return u @ R.T + t


def test_relative_poses_keep_every_vertex_distance():
    """|T_rel' u - u| over centred u equals |T_est v - T_gt v| over v to 1e-12 (on the float64 values; float32 is one
    rounding of them)."""
    rng = np.random.default_rng(0)
    T_est, T_gt = _random_poses(rng, 9), _random_poses(rng, 9)
    v = rng.normal(size=(40, 3)) * 0.1 + np.array([0.4, -1.2, 2.5])
    c = v.mean(axis=0)
    rel64 = E.relative_poses(T_est, T_gt, c, dtype=np.float64)
    rel = E.relative_poses(list(T_est), list(T_gt), c)
    assert rel.dtype == np.float32 and rel.shape == (9, 12) and rel64.dtype == np.float64
    np.testing.assert_array_equal(rel, rel64.astype(np.float32))
    u = v - c
    for k in range(9):
        want = np.linalg.norm((v @ T_est[k, :3, :3].T + T_est[k, :3, 3]) - (v @ T_gt[k, :3, :3].T + T_gt[k, :3, 3]), axis=1)
        got = np.linalg.norm(_apply(rel64[k], u) - u, axis=1)
        assert np.abs(got - want).max() < 1e-12


def test_relative_poses_identity_is_exact():
    eye = np.tile(np.eye(4), (3, 1, 1))
    rel = E.relative_poses(eye, eye, [0.3, -2.0, 7.0])
    np.testing.assert_array_equal(rel, np.tile(np.r_[np.eye(3).reshape(-1), np.zeros(3)].astype(np.float32), (3, 1)))
    # the same (non-identity) matrices on both sides: exact too
    T = _random_poses(np.random.default_rng(2), 4)
    np.testing.assert_array_equal(E.relative_poses(T, T.copy(), [1.0, 2.0, 3.0]), rel[:1].repeat(4, axis=0))
    with pytest.raises(ValueError):
        E.relative_poses(T, T[:2], [0, 0, 0])


def test_auc_closed_cases():
    assert E.auc(np.zeros(7), 0.1) == 1.0
    assert E.auc([0.1, 0.2, 5.0], 0.1) == 0.0
    m = 0.1
    assert E.auc([0.0, m / 2, np.inf, np.nan], m) == pytest.approx(0.375, abs=1e-15)
    assert E.auc([0.0, None], m) == 0.5
    assert np.isnan(E.auc([], m))


def test_auc_is_the_area_under_the_accuracy_curve():
    rng = np.random.default_rng(3)
    d = np.abs(rng.normal(size=500)) * 0.06
    d[::17] = np.inf
    m = 0.1
    xs = (np.arange(10000) + 0.5) * (m / 10000)  # midpoint rule, 10 000 steps
    acc = (d[None, :] <= xs[:, None]).mean(axis=1)
    assert abs(E.auc(d, m) - acc.mean()) < 1e-3
    assert E.accuracy_under(d, 0.05) == pytest.approx((d < 0.05).mean())
    assert E.accuracy_under([0.01, np.nan, None, 0.2], 0.05) == 0.25


def test_evaluate_poses_refuses_a_cpu_device():
    from pixtrack_amd import _lib

    v = np.random.default_rng(4).normal(size=(10, 3))
    with pytest.raises(_lib.PxtError):
        E.evaluate_poses({}, v, "cpu")
    with pytest.raises(_lib.PxtError):
        E.pose_errors(np.eye(4)[None], np.eye(4)[None], v, "cpu")


def test_pose_errors_op_is_registered_for_the_device_only():
    import torch

    from pixtrack_amd import _lib, ops

    assert "pose_errors" in ops.op_names() and "pxt_pose_errors" in _lib.PROTOTYPES
    assert _lib.PXT_POSE_ERR_RECORD == 8
    s = str(torch.ops.pixtrack.pose_errors.default._schema)
    assert "Tensor(a!) records" in s and "Tensor(b!) workspace" in s
    with pytest.raises(NotImplementedError):  # no CPU kernel: the dispatcher refuses host tensors
        torch.ops.pixtrack.pose_errors(torch.zeros(4, 3), torch.zeros(1, 12), True, torch.zeros(1, 8),
                                       torch.zeros(64, dtype=torch.uint8))
    L = _lib.lib()
    assert int(L.pxt_pose_errors_workspace_bytes(3, 1500)) == 3 * 2 * 16
    for F, V in ((0, 10), (65536, 10), (1, 0), (1, (1 << 20) + 1)):
        assert int(L.pxt_pose_errors_workspace_bytes(F, V)) < 0


def test_vertex_readers(tmp_path):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(11, 3))
    np.save(tmp_path / "v3.npy", v)
    np.save(tmp_path / "v4.npy", np.c_[v, np.ones(11)].astype(np.float32))
    np.savetxt(tmp_path / "points.xyz", v)
    np.savetxt(tmp_path / "one.xyz", v[:1])
    np.testing.assert_array_equal(E.read_vertices(tmp_path / "v3.npy"), v)
    np.testing.assert_allclose(E.read_vertices(tmp_path / "v4.npy"), v, rtol=1e-6)
    assert E.read_vertices(tmp_path / "v4.npy").shape == (11, 3)
    np.testing.assert_allclose(E.read_vertices(tmp_path / "points.xyz"), v, rtol=1e-15)
    assert E.read_vertices(tmp_path / "one.xyz").shape == (1, 3)
    np.save(tmp_path / "bad.npy", np.zeros((4, 2)))
    with pytest.raises(ValueError):
        E.read_vertices(tmp_path / "bad.npy")


def test_cli_arguments():
    a = E.build_parser().parse_args(["--poses", "p.pkl", "--vertices", "v.npy"])
    assert (a.poses, a.vertices, a.symmetric, a.max_distance, a.threshold, a.offset, a.json) == \
        ("p.pkl", "v.npy", False, 0.1, None, False, None)
    a = E.build_parser().parse_args(["--poses", "p.pkl", "--vertices", "points.xyz", "--symmetric", "--max_distance", "0.2",
                                     "--threshold", "0.02", "--offset", "--json", "out.json"])
    assert (a.symmetric, a.max_distance, a.threshold, a.offset, a.json) == (True, 0.2, 0.02, True, "out.json")
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--poses", "p.pkl"])
