"""reference_points="template" without a GPU: mesh_render.points_reference (the numpy restatement of
pxt_points_from_depth_views) on handmade planes and on a plane the CPU rasteriser drew, every PXT_E_ARG bound of the C
entry, the declarations, the constructor rules and the command lines."""
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import mesh_render as R

ROOT = Path(__file__).resolve().parent.parent
IDENTITY_VIEW = R.pack_view(np.eye(3), [0.0, 0.0, 0.0], 10.0, 10.0, 3.5, 3.5, 1e-6, 1.0)


def plane(H, W, covered):
    """A depth plane as the rasteriser writes it: ``covered`` bool [H, W] -> depth 0.5 and alpha 1 there, zeros elsewhere."""
    d = np.zeros((H, W, 4), np.float32)
    d[covered] = (0.5, 0.5, 0.5, 1.0)
    return d


def first_pixels(H, W, n):
    covered = np.zeros(H * W, bool)
    covered[:n] = True
    return covered.reshape(H, W)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement on handmade planes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,s", [(35, 1), (36, 1), (37, 2), (143, 2), (144, 2), (145, 3)])
def test_stride_rule(A, s):
    """n_max = 36: the smallest s with s * s * 36 >= A, just below, at and above 36 and 144."""
    p3d, valid, rec = R.points_reference(plane(16, 16, first_pixels(16, 16, A)), IDENTITY_VIEW, 0.5, 0, 36)
    ys, xs = np.divmod(np.arange(A), 16)
    n_cand = int(((xs % s == s // 2) & (ys % s == s // 2)).sum())
    assert rec.tolist() == [A, s, min(n_cand, 36), n_cand] and int(valid.sum()) == min(n_cand, 36)


def cut_tail_plane():
    covered = np.zeros((8, 8), bool)
    covered[1:6:2, 1:6:2] = True  # (1, 1), (3, 1), (5, 1), (1, 3), ..., (5, 5)
    return plane(8, 8, covered)


def test_cut_tail():
    p3d, valid, rec = R.points_reference(cut_tail_plane(), IDENTITY_VIEW, 0.5, 0, 4)
    assert rec.tolist() == [9, 2, 4, 9] and valid.tolist() == [1, 1, 1, 1]
    # the first four candidates in row-major order: (1, 1), (3, 1), (5, 1), (1, 3); z = 0.5, fx = fy = 10, c = 3.5
    want = np.array([[0.5 * (x - 3.5) / 10, 0.5 * (y - 3.5) / 10, 0.5] for x, y in ((1, 1), (3, 1), (5, 1), (1, 3))])
    assert np.abs(p3d - want).max() < 1e-7


def test_empty_plane_holds_the_camera_centre():
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    t = np.array([0.3, -0.2, 2.5])
    view = R.pack_view(q, t, 50.0, 48.0, 3.0, 4.0, 1e-6, 0.25)
    p3d, valid, rec = R.points_reference(np.zeros((8, 8, 4), np.float32), view, 0.5, 1, 5)
    assert rec.tolist() == [0, 1, 0, 0] and not valid.any()
    centre = -q.T @ t  # R^T (-t)
    assert np.array_equal(p3d, np.repeat(p3d[:1], 5, 0)) and np.abs(p3d[0] - centre).max() < 1e-6


def test_erosion_at_the_border():
    full = plane(5, 5, np.ones((5, 5), bool))
    assert R.points_reference(full, IDENTITY_VIEW, 0.5, 0, 64)[2].tolist() == [25, 1, 25, 25]
    p3d, valid, rec = R.points_reference(full, IDENTITY_VIEW, 0.5, 1, 64)
    assert rec.tolist() == [9, 1, 9, 9]  # the inner 3 x 3
    assert np.abs(p3d[0] - [0.5 * (1 - 3.5) / 10, 0.5 * (1 - 3.5) / 10, 0.5]).max() < 1e-7
    p3d, valid, rec = R.points_reference(full, IDENTITY_VIEW, 0.5, 2, 64)
    assert rec.tolist() == [1, 1, 1, 1]  # the one centre pixel
    assert np.abs(p3d[0] - [0.5 * (2 - 3.5) / 10, 0.5 * (2 - 3.5) / 10, 0.5]).max() < 1e-7
    assert R.points_reference(plane(4, 4, np.ones((4, 4), bool)), IDENTITY_VIEW, 0.5, 2, 64)[2].tolist() == [0, 1, 0, 0]


def test_alpha_gate():
    d = plane(4, 4, np.ones((4, 4), bool))
    d[1, 2, 3] = 0.49
    d[2, 1, 0] = 0.0   # the depth half of the base test
    assert R.points_reference(d, IDENTITY_VIEW, 0.5, 0, 64)[2].tolist() == [14, 1, 14, 14]
    d[1, 2, 3] = 0.5   # alpha == min_alpha passes
    assert R.points_reference(d, IDENTITY_VIEW, 0.5, 0, 64)[2][0] == 15


# ----------------------------------------------------------------------------------------------------------------------
# round trip on a plane the CPU rasteriser drew
# ----------------------------------------------------------------------------------------------------------------------
def lattice_pixels(depth, min_alpha, erode, n_max):
    """The rule's pixels through scipy's erosion (independent of points_reference's own slicing)."""
    from scipy.ndimage import binary_erosion

    base = (depth[..., 3] >= min_alpha) & (depth[..., 0] > 0)
    size = 2 * erode + 1
    accepted = binary_erosion(base, structure=np.ones((size, size), bool), border_value=0) if erode else base
    s = 1
    while s * s * n_max < int(accepted.sum()):
        s += 1
    return [(int(x), int(y)) for y, x in np.argwhere(accepted) if x % s == s // 2 and y % s == s // 2][:n_max], s


def test_round_trip_on_a_drawn_plane():
    V, F = R.icosphere(1)
    V = V * np.array([1.0, 0.8, 0.6])
    radius = float(np.linalg.norm(V, axis=1).max())
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    t = np.array([0.15, -0.1, 3.0])
    # fx != fy, the principal point off the centre (599.5, 599.5).  The rasteriser snaps a vertex to 1 / 256 px: the plane
    # it interpolates lies up to z / (512 f) = 3.9e-6 units from the triangle's, so the 1e-5 bar needs this many pixels
    W, H, fx, fy, cx, cy = 1200, 1200, 1500.0, 1400.0, 580.25, 630.5
    view = R.pack_view(q, t, fx, fy, cx, cy, 1e-6, 1.0 / (np.linalg.norm(t) + radius))
    depth, ids, _ = R.rasterize_reference(V, F, view[None], W, H)
    p3d, valid, rec = R.points_reference(depth[0], view, 0.5, 1, 64)
    pixels, s = lattice_pixels(depth[0], 0.5, 1, 64)
    n = int(rec[2])
    assert n == len(pixels) and 20 < n <= 64 and rec[1] == s and s >= 2 and valid[:n].all() and not valid[n:].any()
    R64, t64 = view[:9].astype(np.float64).reshape(3, 3), view[9:12].astype(np.float64)
    f64 = view[12:16].astype(np.float64)
    cam = p3d[:n].astype(np.float64) @ R64.T + t64
    u, v = f64[0] * cam[:, 0] / cam[:, 2] + f64[2], f64[1] * cam[:, 1] / cam[:, 2] + f64[3]
    err = np.hypot(u - [x for x, _ in pixels], v - [y for _, y in pixels]).max()
    print(f"round trip: {n} points, stride {s}, max reprojection error {err:.3g} px")
    assert err < 1e-2
    # every point lies in the plane of the triangle that won its pixel
    V64, worst = np.asarray(V, np.float32).astype(np.float64), 0.0
    for (x, y), p in zip(pixels, p3d[:n].astype(np.float64)):
        a, b, c = V64[np.asarray(F)[ids[0, y, x]]]
        normal = np.cross(b - a, c - a)
        worst = max(worst, abs(np.dot(p - a, normal / np.linalg.norm(normal))))
    print(f"largest distance to the winning triangle's plane {worst:.3g} (mesh radius {radius:.3g})")
    assert worst < 1e-5 * radius


# ----------------------------------------------------------------------------------------------------------------------
# the C entry: declarations and bounds.  PXT_E_ARG comes from the host-side checks ahead of the first HIP call, so
# nothing is dereferenced and device pointers can be stood in for by aligned numbers
# ----------------------------------------------------------------------------------------------------------------------
BASE = 1 << 20


def test_the_entry_points_the_constant_and_the_op_are_declared():
    from pixtrack_amd import _lib, ops

    header = (ROOT / "include" / "pixtrack_hip.h").read_text()
    assert _lib.ABI_VERSION == 13 and re.search(r"int pxt_version\(void\);\s*/\* ABI version \(13\)", header)
    for name in ("pxt_points_from_depth_views", "pxt_points_from_depth_views_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    assert re.search(r"#define\s+PXT_POINTS_MAX_VIEWS\s+16\b", header) and _lib.PXT_POINTS_MAX_VIEWS == 16
    assert R.POINTS_MAX_VIEWS == 16 and "points_from_depth_views" in ops.op_names()
    L, C = _lib.lib(), _lib.C
    size = lambda sizes: int(L.pxt_points_from_depth_views_workspace_bytes(len(sizes) // 2, (C.c_int32 * len(sizes))(*sizes)))
    # 128 bytes of heads, two int32 counts per 1024-pixel segment (rounded to 64 bytes), one bit per pixel of the segments
    assert size([640, 480]) == 128 + 2432 + 300 * 128
    assert size([37, 29, 32, 32, 8, 8]) == 128 + 64 + 4 * 128 and size([37, 29, 32, 32, 8, 8]) % 16 == 0
    assert size([16384, 16384] * 16) > 0
    assert size([]) == -1 and size([8, 8] * 17) == -1 and size([0, 8]) == -1 and size([8, 16385]) == -1
    assert int(L.pxt_points_from_depth_views_workspace_bytes(1, None)) == -1


def views_call(n_views=2, sizes=(8, 8, 5, 7), views=None, planes=None, min_alpha=0.5, erode=1, n_max=16, p3d=BASE,
               slot_valid=BASE, records=BASE, workspace=BASE, null=()):
    from pixtrack_amd import _lib

    L, C = _lib.lib(), _lib.C
    K = len(sizes) // 2
    if views is None:
        views = np.stack([IDENTITY_VIEW] * max(K, 1))
    views = np.ascontiguousarray(views, np.float32)
    planes = [BASE + 4096 * k for k in range(K)] if planes is None else planes
    return L.pxt_points_from_depth_views(
        None if "depth" in null else (C.c_void_p * max(len(planes), 1))(*planes),
        None if "sizes" in null else (C.c_int32 * max(len(sizes), 1))(*sizes),
        None if "views" in null else views.ctypes.data_as(C.POINTER(C.c_float)), n_views, min_alpha, erode, n_max, p3d,
        slot_valid, records, workspace, None)


def bad_view(index, value):
    v = np.stack([IDENTITY_VIEW] * 2)
    v[1, index] = value
    return v


BAD_CALLS = {
    "no views": dict(n_views=0),
    "17 views": dict(n_views=17, sizes=(8, 8) * 17),
    "a width of 0": dict(sizes=(8, 8, 0, 7)),
    "a height of 16385": dict(sizes=(8, 8, 5, 16385)),
    "erode -1": dict(erode=-1),
    "erode 3": dict(erode=3),
    "n_max 0": dict(n_max=0),
    "n_max above 2^24": dict(n_max=(1 << 24) + 1),
    "no plane table": dict(null=("depth",)),
    "no sizes": dict(null=("sizes",)),
    "no view records": dict(null=("views",)),
    "a NULL plane": dict(planes=[BASE, 0]),
    "a plane that is not 16-byte aligned": dict(planes=[BASE, BASE + 8]),
    "no p3d": dict(p3d=None),
    "a p3d that is not 4-byte aligned": dict(p3d=BASE + 2),
    "no slot_valid": dict(slot_valid=None),
    "a slot_valid that is not 4-byte aligned": dict(slot_valid=BASE + 1),
    "no records": dict(records=None),
    "records that are not 4-byte aligned": dict(records=BASE + 2),
    "no workspace": dict(workspace=None),
    "a workspace that is not 16-byte aligned": dict(workspace=BASE + 8),
    "a NaN in R": dict(views=bad_view(4, np.nan)),
    "an infinite t": dict(views=bad_view(10, np.inf)),
    "a NaN in the padding": dict(views=bad_view(19, np.nan)),
    "fx = 0": dict(views=bad_view(12, 0.0)),
    "fy < 0": dict(views=bad_view(13, -10.0)),
    "depth_q = 0": dict(views=bad_view(17, 0.0)),
}


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_the_calls_bounds_are_argument_errors(case):
    assert views_call(**BAD_CALLS[case]) == -1  # PXT_E_ARG: nothing is launched or written


# ----------------------------------------------------------------------------------------------------------------------
# constructor rules and command lines
# ----------------------------------------------------------------------------------------------------------------------
def test_template_points_are_refused_by_name_where_they_cannot_run():
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB

    mesh = object.__new__(MeshTemplate)
    with pytest.raises(ValueError, match=r"reference_points='template'.*needs.*MeshTemplate.*'render'"):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="template")
    with pytest.raises(ValueError, match=r"reference_points='template'.*MeshTemplate"):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="template", template="nerf")
    with pytest.raises(ValueError, match=r"reference_points='template'.*uncertainty"):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="template", template=mesh, uncertainty=True)
    with pytest.raises(ValueError, match=r"relocalizer"):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="template", template=mesh, relocalizer="views")
    with pytest.raises(ValueError, match=r"reference_points='template' is not supported by PixLocPoseTrackerYCB"):
        PixLocPoseTrackerYCB("", "", "/tmp", "", reference_points="template")
    # "render" keeps its refusal with a mesh template
    with pytest.raises(ValueError, match=r"mesh template.*reference_points"):
        PixLocPoseTrackerR9("", "", "", "/tmp", reference_points="render", template=mesh)


def stand_in(template, reference_points):
    import torch

    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    tr = object.__new__(PixLocPoseTrackerR9)
    tr.device, tr.reference_points, tr.depth_refine, tr.occlusion, tr.template = torch.device("cpu"), reference_points, None, None, template
    return tr


def test_lock_step_tracking_takes_template_points_of_a_mesh_template():
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker, MutualOcclusion

    mesh = object.__new__(MeshTemplate)
    # accepted: the stand-in then fails on the first attribute it lacks, not on its points
    with pytest.raises(Exception) as e:
        MultiObjectTracker([stand_in(mesh, "template")])
    assert isinstance(e.value, AttributeError) and "reference_points" not in str(e.value), repr(e.value)
    with pytest.raises(ValueError, match=r"reference_points='template'.*mesh template"):
        MultiObjectTracker([stand_in(None, "template")])
    with pytest.raises(ValueError, match=r"mutual_occlusion.*reference_points='template'"):
        MultiObjectTracker([stand_in(mesh, "template"), stand_in(mesh, "sfm")], mutual_occlusion=MutualOcclusion(scenes=[None, None]))
    with pytest.raises(ValueError, match=r"reference_points='render'"):
        MultiObjectTracker([stand_in(mesh, "render")])


def test_the_refiner_takes_the_value():
    from pixtrack_amd.refiner import PoseTrackerRefiner

    assert PoseTrackerRefiner.default_config["reference_points"] == "sfm"  # (the default stays)
    probe = object.__new__(PoseTrackerRefiner)
    for value, render, template in (("sfm", False, False), ("render", True, False), ("template", True, True)):
        probe.conf = type("Conf", (), {"reference_points": value})()
        assert probe.render_points is render and probe.template_points is template


def test_the_parsers_accept_template_and_default_to_sfm():
    from pixtrack_amd.pose_trackers import multi_object_tracker as multi, pixloc_tracker_r9 as r9

    base = ["--object_path", "o", "--query", "q", "--out_dir", "out"]
    for module in (r9, multi):
        assert module.build_parser().parse_args(base).reference_points == "sfm"
        assert module.build_parser().parse_args(base + ["--reference_points", "template"]).reference_points == "template"
        with pytest.raises(SystemExit):
            module.build_parser().parse_args(base + ["--reference_points", "colmap"])
    assert r9.build_parser().parse_args(base + ["--reference_points", "render"]).reference_points == "render"
