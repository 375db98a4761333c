"""Host side of the BOP errors (pixtrack_amd/evaluation.py: the kernel's per-frame input, the recall helpers, the
bindings' constants and bounds, the op's registration, the command lines) - everything that needs no GPU.  The kernel is
tests/test_bop_errors_gpu.py's."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, evaluation as E, ops, render_evaluation as RE


def _random_poses(rng, n):
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[k, :3, :3] = q * np.sign(np.linalg.det(q))
        out[k, :3, 3] = rng.normal(size=3) * 2.0
    return out


def test_symmetric_frames_hold_the_three_poses_for_centred_vertices():
    rng = np.random.default_rng(0)
    T_est, T_gt = _random_poses(rng, 5), _random_poses(rng, 5)
    c = np.array([0.4, -1.2, 2.5])
    K = rng.uniform(300, 700, size=(5, 4))
    fr = E.symmetric_frames(T_est, T_gt, c, K)
    assert fr.shape == (5, 40) and fr.dtype == np.float32 and _lib.PXT_SYM_ERR_FRAME == 40
    fr64 = E.symmetric_frames(list(T_est), list(T_gt), c, K, dtype=np.float64)
    np.testing.assert_array_equal(fr, fr64.astype(np.float32))  # float64, rounded once
    np.testing.assert_array_equal(fr64[:, :12], E.relative_poses(T_est, T_gt, c, dtype=np.float64))
    np.testing.assert_array_equal(fr64[:, 36:], K)
    v = rng.normal(size=(30, 3)) * 0.1 + c
    for k in range(5):
        for block, T in ((fr64[k, 12:24], T_est[k]), (fr64[k, 24:36], T_gt[k])):
            got = (v - c) @ block[:9].reshape(3, 3).T + block[9:]
            assert np.abs(got - (v @ T[:3, :3].T + T[:3, 3])).max() < 1e-14
    with pytest.raises(ValueError):
        E.symmetric_frames(T_est, T_gt, c, K[:4])


def test_cameras_give_intrinsics_and_widths():
    from pixtrack_amd.geometry import Camera

    cam = Camera(torch.tensor([640.0, 480.0, 600.0, 610.0, 319.5, 239.5]))
    wide = Camera(torch.tensor([1280.0, 960.0, 1200.0, 1220.0, 639.5, 479.5, 0.1, 0.0]))
    K, w = E._intrinsics(cam, 3)
    np.testing.assert_array_equal(K, np.tile([600.0, 610.0, 319.5, 239.5], (3, 1)))
    np.testing.assert_array_equal(w, [640.0] * 3)
    K, w = E._intrinsics([cam, wide], 2)
    np.testing.assert_array_equal(K[1], [1200.0, 1220.0, 639.5, 479.5])  # lens terms are dropped: a pinhole, as in BOP
    np.testing.assert_array_equal(w, [640.0, 1280.0])
    assert E._intrinsics([1.0, 2.0, 3.0, 4.0], 2)[0].shape == (2, 4) and E._intrinsics(np.ones((2, 4)), 2)[1] is None
    for bad, F in (([cam], 2), (np.ones((3, 4)), 2), (np.ones(5), 1)):
        with pytest.raises(ValueError):
            E._intrinsics(bad, F)


def test_recalls_are_strict_and_count_a_miss():
    d = 0.2
    assert E.BOP_THETAS[0] == 0.05 and E.BOP_THETAS[-1] == 0.5 and len(E.BOP_THETAS) == 10
    assert E.BOP_THETAS_PX[0] == 5.0 and E.BOP_THETAS_PX[-1] == 50.0 and len(E.BOP_THETAS_PX) == 10
    assert E.recall_mssd([0.0], d) == 1.0 and E.recall_mssd([0.5 * d], d) == 0.0  # at the last threshold: not below it
    assert E.recall_mssd([np.nextafter(0.5 * d, 0)], d) == pytest.approx(0.1)
    assert E.recall_mssd([0.0, np.inf, np.nan, None], d) == 0.25  # non-finite or missing: below no threshold
    assert E.recall_mssd([0.25 * d], d, thetas=(0.25, 0.5)) == 0.5  # strict at a threshold of the list
    assert np.isnan(E.recall_mssd([], d)) and np.isnan(E.recall_mspd([], 640))
    # r = width / 640: the same pixel distance is judged against thresholds twice as wide in an image twice as wide
    assert E.recall_mspd([5.0], 640) == pytest.approx(0.9) and E.recall_mspd([5.0], 1280) == 1.0
    assert E.recall_mspd([10.0], 1280) == pytest.approx(0.9) and E.recall_mspd([50.0], 640) == 0.0
    assert E.recall_mspd([49.0, 49.0], [640, 320]) == pytest.approx(0.05)  # per frame: 1 of 10 and 0 of 10
    assert E.recall_mspd([0.0, np.inf], 640) == 0.5
    rng = np.random.default_rng(1)
    x = np.abs(rng.normal(size=200)) * 0.08
    assert E.recall_mssd(x, d) == pytest.approx(np.mean([[v < t * d for t in E.BOP_THETAS] for v in x]))


def test_the_bindings_know_the_entry_point_and_its_bounds():
    assert {"pxt_symmetric_pose_errors", "pxt_symmetric_pose_errors_workspace_bytes"} <= set(_lib.PROTOTYPES)
    assert (_lib.PXT_SYM_ERR_RECORD, _lib.PXT_SYM_ERR_FRAME, _lib.PXT_SYM_ERR_MAX_SYMS) == (8, 40, 1024)
    header = (_lib._HERE.parent / "include" / "pixtrack_hip.h").read_text()
    for name in ("PXT_SYM_ERR_RECORD", "PXT_SYM_ERR_FRAME", "PXT_SYM_ERR_MAX_SYMS"):
        assert f"#define {name} {getattr(_lib, name)}\n" in header
    L = _lib.lib()
    assert L.pxt_version() == 13
    wb = L.pxt_symmetric_pose_errors_workspace_bytes
    assert int(wb(1, 1, 1)) > 0 and int(wb(65535, 1024, 1 << 20)) > 0
    assert int(wb(24, 315, 1025)) == 24 * int(wb(1, 315, 1025))  # per frame
    assert int(wb(1, 630, 300)) >= 630 * 2 * 4 and int(wb(1, 1024, 1 << 20)) <= 2 << 20
    for F, S, V in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1025, 1), (1, 1, 0), (1, 1, (1 << 20) + 1), (-1, 1, 1)):
        assert int(wb(F, S, V)) < 0, (F, S, V)


def test_the_op_is_registered_for_the_device_only():
    assert "symmetric_pose_errors" in ops.op_names()
    s = str(torch.ops.pixtrack.symmetric_pose_errors.default._schema)
    assert "Tensor(a!) records" in s and "Tensor(b!) workspace" in s and "Tensor syms" in s
    cpu = (torch.zeros(4, 3), torch.zeros(1, 12), torch.zeros(1, 40), torch.zeros(1, 8), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):  # no CPU kernel: the dispatcher refuses host tensors
        torch.ops.pixtrack.symmetric_pose_errors(*cpu)
    with pytest.raises(_lib.PxtError):  # the op body itself, called directly: host memory is refused before the native call
        ops._symmetric_pose_errors(*cpu)
    v = np.random.default_rng(4).normal(size=(10, 3))
    with pytest.raises(_lib.PxtError):
        E.symmetric_pose_errors(np.eye(4)[None], np.eye(4)[None], v, [600, 600, 320, 240], None, "cpu")
    with pytest.raises(_lib.PxtError):
        E.evaluate_poses_bop({}, v, "cpu", 0.2)


def test_merge_keeps_what_is_there():
    res = {"n_frames": 2, "add_mean": 0.1, "frames": {"a": {"add": 0.1, "ok": True}, "b": {"add": 0.2, "ok": True}}}
    bop = {"n_frames": 2, "ar_mssd": 0.5, "frames": {"a": {"mssd": 0.3, "ok": False}, "b": {"mssd": 0.4, "ok": True}}}
    out = E.merge_bop(res, bop)
    assert out["add_mean"] == 0.1 and out["ar_mssd"] == 0.5
    assert out["frames"]["a"] == {"add": 0.1, "ok": True, "mssd": 0.3}


def test_cli_flags_exist_and_the_defaults_change_nothing(tmp_path, monkeypatch, capsys):
    a = E.build_parser().parse_args(["--poses", "p.pkl", "--vertices", "v.npy"])
    assert (a.bop, a.diameter, a.models_info, a.obj_id, a.models_info_scale) == (False, None, None, None, 1.0)
    a = E.build_parser().parse_args(["--poses", "p.pkl", "--vertices", "v.npy", "--bop", "--diameter", "0.2",
                                     "--models_info", "m.json", "--obj_id", "5", "--models_info_scale", "0.001"])
    assert (a.bop, a.diameter, a.models_info, a.obj_id, a.models_info_scale) == (True, 0.2, "m.json", 5, 0.001)
    r = RE.build_parser().parse_args(["--poses", "p.pkl", "--object_path", "obj"])
    assert (r.bop, r.vertices, r.models_info, r.obj_id, r.diameter) == (False, None, None, None, None)
    r = RE.build_parser().parse_args(["--poses", "p.pkl", "--object_path", "obj", "--bop", "--vertices", "v.npy",
                                      "--models_info", "m.json", "--obj_id", "2"])
    assert (r.bop, r.vertices, r.models_info, r.obj_id) == (True, "v.npy", "m.json", 2)
    # the symmetry set the flags name, in the units of the vertices
    from pathlib import Path

    golden = Path(__file__).resolve().parent / "golden" / "bop_models_info.json"
    a = E.build_parser().parse_args(["--poses", "p", "--vertices", "v", "--bop", "--diameter", "0.2", "--models_info",
                                     str(golden), "--obj_id", "12", "--models_info_scale", "0.001"])
    sym = E.bop_symmetries(a)
    assert sym.shape == (2, 4, 4) and np.allclose(sym[1, :3, 3], [0.004, -0.002, 0.0], atol=1e-18)
    assert E.bop_symmetries(E.build_parser().parse_args(["--poses", "p", "--vertices", "v"])) is None

    # main(): without --bop only evaluate_poses runs and its keys are printed as they are; with it the BOP keys are added
    calls = []
    monkeypatch.setattr("pixtrack_amd.utils.io.load_reference_pickle", lambda path: {"f0": {}})
    monkeypatch.setattr(E, "read_vertices", lambda path: np.zeros((3, 3)))
    monkeypatch.setattr(E, "evaluate_poses", lambda *a, **k: {"frames": {"f0": {"add": 1.0, "ok": True}}, "n_frames": 1,
                                                              "add_mean": 1.0})

    def fake_bop(poses, vertices, device, diameter, symmetries=None, offset=False, ar_vsd=None):
        calls.append((diameter, symmetries, offset))
        return {"frames": {"f0": {"mssd": 2.0, "mspd": 3.0, "ok": True}}, "n_frames": 1, "ar_mssd": 0.5, "ar_mspd": 0.25}

    monkeypatch.setattr(E, "evaluate_poses_bop", fake_bop)
    res = E.main(["--poses", "p.pkl", "--vertices", "v.npy"])
    assert not calls and res == {"frames": {"f0": {"add": 1.0, "ok": True}}, "n_frames": 1, "add_mean": 1.0}
    assert capsys.readouterr().out.strip() == '{"n_frames": 1, "add_mean": 1.0}'
    out = tmp_path / "o.json"
    res = E.main(["--poses", "p.pkl", "--vertices", "v.npy", "--bop", "--diameter", "0.2", "--offset", "--json", str(out)])
    assert calls == [(0.2, None, True)] and res["ar_mssd"] == 0.5 and res["add_mean"] == 1.0
    assert res["frames"]["f0"] == {"add": 1.0, "ok": True, "mssd": 2.0, "mspd": 3.0}
    import json

    assert json.loads(out.read_text()) == res and '"ar_mspd": 0.25' in capsys.readouterr().out
    with pytest.raises(SystemExit):  # --bop needs the diameter
        E.main(["--poses", "p.pkl", "--vertices", "v.npy", "--bop"])
