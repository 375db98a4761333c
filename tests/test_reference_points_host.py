"""Host-side checks of the opt-in ``reference_points`` (no GPU): the CLI switch, the boundary, the construction-time
refusals and the ngp -> SfM map the back-projection is chained with."""
import numpy as np
import pytest

from pixtrack_amd import _lib, ops
from pixtrack_amd.ngp import ngp_to_sfm_affine, nerf_matrix_to_ngp
from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as r9_cli
from pixtrack_amd.utils.ingp_utils import sfm_to_nerf_pose


def test_cli_accepts_reference_points():
    base = ["--object_path", "o", "--query", "q", "--out_dir", "out"]
    assert r9_cli.build_parser().parse_args(base).reference_points == "sfm"
    assert r9_cli.build_parser().parse_args(base + ["--reference_points", "render"]).reference_points == "render"
    with pytest.raises(SystemExit):
        r9_cli.build_parser().parse_args(base + ["--reference_points", "colmap"])


def test_boundary_has_the_entry_points():
    assert "points_from_depth" in ops.op_names()
    assert {"pxt_points_from_depth", "pxt_points_from_depth_workspace_bytes"} <= set(_lib.PROTOTYPES)
    L = _lib.lib()
    # header of 64 bytes, two int32 counts per 1024-pixel segment (rounded to 64 bytes), one bit per pixel of the segments
    assert int(L.pxt_points_from_depth_workspace_bytes(640, 480)) == 64 + 2432 + 300 * 128
    assert int(L.pxt_points_from_depth_workspace_bytes(0, 480)) < 0
    assert _lib.ABI_VERSION == 13


def test_unknown_and_refused_values_raise_before_anything_is_built():
    for kw in (dict(reference_points="colmap"), dict(reference_points="render", uncertainty=True),
               dict(reference_points="render", relocalizer="views")):
        with pytest.raises(ValueError):
            r9_cli.PixLocPoseTrackerR9("", "", "", "/tmp", **kw)


def test_ngp_to_sfm_affine_inverts_the_pose_chain():
    """A camera centre taken SfM -> NeRF -> ngp by the renderer's own chain comes back through the affine map."""
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Rn = np.eye(4)
    Rn[:3, :3] = q * np.sign(np.linalg.det(q))
    nerf2sfm = {"centroid": rng.normal(size=3), "avglen": 2.3, "totp": rng.normal(size=3), "R": Rn}
    scale, offset = 0.33, 0.5
    A = ngp_to_sfm_affine(nerf2sfm, scale, offset)
    for _ in range(4):
        c2w = np.eye(4)
        c2w[:3, 3] = rng.normal(size=3)
        cam_ngp = nerf_matrix_to_ngp(sfm_to_nerf_pose(nerf2sfm, c2w)[:3, :], scale, offset)
        np.testing.assert_allclose(A[:, :3] @ cam_ngp[:, 3] + A[:, 3], c2w[:3, 3], rtol=0, atol=1e-12)
        # a point one unit down the camera's viewing axis (ngp column 2 is the forward axis of the render's rays)
        z = 0.7
        p_ngp = cam_ngp[:, 3] + z * cam_ngp[:, 2]
        fwd_sfm = c2w[:3, 2]  # identity rotation: the SfM camera looks down +z
        want = c2w[:3, 3] + (z / (scale * 3.0 / nerf2sfm["avglen"])) * fwd_sfm
        np.testing.assert_allclose(A[:, :3] @ p_ngp + A[:, 3], want, rtol=0, atol=1e-12)
