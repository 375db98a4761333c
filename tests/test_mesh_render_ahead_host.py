"""Render-ahead for mesh templates, the parts that need no GPU: mesh_render.posed_view_reference against the host's own
view record, the declarations, the defaults and the command-line flag."""
import re
from pathlib import Path

import numpy as np
import torch

from pixtrack_amd import _lib, ops
from pixtrack_amd import mesh_render as R
from pixtrack_amd.geometry import Camera, Pose
from pixtrack_amd.mesh_template import MeshTemplate

ROOT = Path(__file__).resolve().parent.parent


class HostTemplate(MeshTemplate):
    """A MeshTemplate without a renderer: depth_q and requests_ahead read ``near``, ``radius`` and ``supersample`` alone."""

    def __init__(self, radius, supersample=2, near=1e-6):
        self.renderer, self.radius, self.supersample, self.near, self.render_ahead = None, float(radius), supersample, near, False


def camera(w=128, h=96, f=153.6, cx=63.5, cy=47.5):
    return Camera(torch.tensor([w, h, f, f * 0.99, cx, cy], dtype=torch.float64))


def rotations(n, rng):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return (q * np.sign(np.linalg.det(q))[:, None, None]).astype(np.float32)


def test_the_reference_equals_the_hosts_view_record_on_10000_poses():
    rng = np.random.default_rng(2024)
    n = 10000
    Rs = rotations(n, rng)
    ts = rng.normal((0.0, 0.0, 3.0), (0.5, 0.5, 1.0), size=(n, 3)).astype(np.float32)
    radii = rng.uniform(0.05, 2.0, size=n)
    cam = camera()
    host = R.view_record(cam, np.eye(4), 1e-6, 0.0)
    host[:12] = 0.0
    different = 0
    for Rm, t, radius in zip(Rs, ts, radii):
        rec = np.zeros(16, np.float32)
        rec[:9], rec[9:12] = Rm.reshape(9), t
        pose = Pose(torch.from_numpy(rec[:12].copy()))
        template = HostTemplate(radius)
        want = R.view_record(cam, pose, template.near, template.depth_q(pose))
        got, flag = R.posed_view_reference(rec, host, radius)
        different += not np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert flag == 1.0 and got.dtype == np.float32 and got.shape == (20,)
    assert different == 0


def test_requests_ahead_are_the_requests_without_a_pose():
    pose = Pose.from_Rt(np.eye(3), np.array([0.01, -0.02, 0.6]))
    for S, ref, depth in ((2, camera(), False), (1, camera(), True), (1, camera(96, 72, 115.2, 47.5, 35.5), True)):
        template = HostTemplate(0.1, S)
        full = template.requests(pose, camera(), ref, want_depth=depth)
        ahead = template.requests_ahead(camera(), ref, want_depth=depth)
        assert len(full) == len(ahead) == (1 if (S == 1 and ref.size[0] == 128) else 2)
        for (v, *rest), (va, *rest_a) in zip(full, ahead):
            assert rest == rest_a
            assert np.array_equal(v[12:17].view(np.uint32), va[12:17].view(np.uint32)) and (va[:12] == 0).all()
            assert va[17] == 0 and (va[18:] == 0).all() and va.dtype == np.float32
            # the device fills in what is missing: the reference on the pose's record gives the full record
            rec = np.zeros(16, np.float32)
            rec[:12] = v[:12]
            assert np.array_equal(R.posed_view_reference(rec, va, template.radius)[0].view(np.uint32), v.view(np.uint32))


def test_the_completion_word_follows_failed_and_status():
    host = np.arange(20, dtype=np.float32)
    for failed, status, want in ((0.0, 0.0, 1.0), (1.0, 0.0, -1.0), (0.0, -4.0, -1.0), (1.0, -6.0, -1.0), (0.0, 3.0, -1.0)):
        rec = np.zeros(20, np.float32)
        rec[9:12], rec[12], rec[13] = (0.1, 0.2, 2.0), failed, status
        got, flag = R.posed_view_reference(torch.from_numpy(rec), host, 0.25)
        assert flag == want
        assert np.array_equal(got[12:17], host[12:17]) and np.array_equal(got[18:], host[18:]) and np.array_equal(got[:12], rec[:12])
        assert got[17] == np.float32(1.0 / (np.sqrt(np.float64(np.float32(0.1)) ** 2 + np.float64(np.float32(0.2)) ** 2 + 4.0) + 0.25))


def test_non_finite_translations_pass_through():
    host = np.zeros(20, np.float32)
    for bad, q in ((np.nan, np.nan), (np.inf, 0.0), (-np.inf, 0.0)):
        rec = np.zeros(16, np.float32)
        rec[9:12] = (0.1, bad, 2.0)
        got, flag = R.posed_view_reference(rec, host, 0.5)
        assert flag == 1.0 and np.array_equal(got[10], np.float32(bad), equal_nan=True)
        assert np.array_equal(got[17], np.float32(q), equal_nan=True)
    rec = np.zeros(16, np.float32)  # t = 0 on a mesh of radius 0: 1 / 0, not an exception
    assert R.posed_view_reference(rec, host, 0.0)[0][17] == np.inf


def test_the_declarations():
    header = (ROOT / "include" / "pixtrack_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+pxt_mesh_render_frame_batch_posed\s*\(", code)
    assert re.search(r"#define\s+PXT_MESH_VIEW_OUT\s+24\b", code) and _lib.PXT_MESH_VIEW_OUT == 24 == R.VIEW_OUT
    assert re.search(r"}\s*pxt_mesh_view_pose\s*;", code)
    L = _lib.lib()
    assert L.pxt_version() == 13 == _lib.ABI_VERSION
    assert "pxt_mesh_render_frame_batch_posed" not in L._pxt_missing
    # the prototype: the batch call's arguments without its stream, then view_pose, views_out, stream
    res, args = _lib.PROTOTYPES["pxt_mesh_render_frame_batch_posed"]
    plain_res, plain_args = _lib.PROTOTYPES["pxt_mesh_render_frame_batch"]
    assert res is plain_res and args[:len(plain_args) - 1] == plain_args[:-1]
    assert args[len(plain_args) - 1:] == [_lib.C.POINTER(_lib.MeshViewPose), _lib.C.c_void_p, _lib.C.c_void_p]
    declared = re.search(r"pxt_mesh_render_frame_batch_posed\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(declared.split(",")) == len(args)
    assert _lib.C.sizeof(_lib.MeshViewPose) == 16 and _lib.MeshViewPose.radius.offset == 8
    assert "mesh_render_frame_batch_posed" in ops.op_names()


def test_the_option_is_off_by_default_and_reaches_the_command_lines():
    import inspect

    from pixtrack_amd.pose_trackers import multi_object_tracker, pixloc_tracker_r9

    assert inspect.signature(MeshTemplate.__init__).parameters["render_ahead"].default is False
    assert inspect.signature(MeshTemplate.from_files).parameters["render_ahead"].default is False
    parser = pixloc_tracker_r9.build_parser()
    assert parser.parse_args([]).mesh_render_ahead is False
    assert parser.parse_args(["--template", "mesh", "--mesh_render_ahead"]).mesh_render_ahead is True
    required = ["--object_path", "a", "--query", "b", "--out_dir", "c"]
    multi = multi_object_tracker.build_parser()
    assert multi.parse_args(required).mesh_render_ahead is False
    assert multi.parse_args(required + ["--mesh_render_ahead"]).mesh_render_ahead is True


def test_a_tracker_with_a_default_mesh_template_does_not_render_ahead(monkeypatch):
    """PixLocPoseTrackerR9's rule for its ``render_ahead`` (the constructor itself needs a GPU; the GPU tests build
    trackers): the NeRF template as ever, a mesh template by its own option, PXT_RENDER_AHEAD=0 switches both off."""
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    rule = PixLocPoseTrackerR9._render_ahead_default
    monkeypatch.delenv("PXT_RENDER_AHEAD", raising=False)
    on = HostTemplate(0.1)
    on.render_ahead = True
    assert rule(HostTemplate(0.1)) is False and rule(on) is True and rule(None) is True
    monkeypatch.setenv("PXT_RENDER_AHEAD", "0")
    assert rule(HostTemplate(0.1)) is False and rule(on) is False and rule(None) is False
