"""The relocaliser's depth stage on the host: the placement grid, the numpy restatement of
pxt_score_pose_hypotheses_depth on a hand-made case, the ABI surface and the constructor rules of relocalizer="mesh" and
reloc_depth.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import _lib
from pixtrack_amd import relocalizer as RL

ROOT = Path(__file__).resolve().parent.parent


# ----------------------------------------------------------------------------------------------------- placements
def _views(rng, n):
    from pixtrack_amd.synthetic import look_at_pose

    centre = np.array([0.1, -0.2, 0.05])
    out = []
    for _ in range(n):
        eye = centre + 3.0 * (lambda d: d / np.linalg.norm(d))(rng.normal(size=3))
        R, t = look_at_pose(eye, centre + 0.1 * rng.normal(size=3))
        out.append((R, t, centre))
    return out


CAM10 = [640.0, 480.0, 700.0, 690.0, 322.5, 236.25, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("grid,distances", [((8, 6), (0.5, 0.71, 1.0, 1.41, 2.0)), ((3, 2), (1.0,)), ((1, 1), (0.8, 1.25))])
def test_placements_put_the_centre_on_the_cell_at_the_factor_of_the_entrys_depth(grid, distances):
    views, rolls = _views(np.random.default_rng(3), 4), 5
    poses, entry = RL.make_placements(views, rolls, CAM10, grid=grid, distances=distances)
    entries, owner = RL.make_hypotheses(views, rolls)
    gx, gy = grid
    per = 1 + len(distances) * gx * gy
    E = len(views) * rolls
    assert poses.dtype == np.float64 and poses.shape == (E * per, 12) and entry.shape == (E * per,)
    assert np.array_equal(entry, np.repeat(np.arange(E), per))
    # the first hypothesis of every entry is the entry's pose, bit for bit
    assert np.array_equal(poses[::per].view(np.uint64), entries.view(np.uint64))
    fx, fy, cx, cy = CAM10[2:6]
    cells = RL.cell_centres(CAM10, grid)
    assert cells[0] == (0.5 * 640 / gx - 0.5, 0.5 * 480 / gy - 0.5) and len(cells) == gx * gy
    if gx > 1:
        assert cells[1][0] > cells[0][0] and cells[1][1] == cells[0][1]  # row-major: x runs first
    for e in range(E):
        R, t = entries[e, :9].reshape(3, 3), entries[e, 9:]
        c = R @ views[int(owner[e])][2] + t
        k = e * per + 1
        for s in distances:  # entry-major, then distance, then the cells row-major
            for px, py in cells:
                P = poses[k]
                assert np.array_equal(P[:9], entries[e, :9])  # the rotation is the entry's
                cc = P[:9].reshape(3, 3) @ views[int(owner[e])][2] + P[9:]
                u, v = fx * cc[0] / cc[2] + cx, fy * cc[1] / cc[2] + cy
                assert abs(u - px) <= 1e-9 * max(1.0, abs(px)) and abs(v - py) <= 1e-9 * max(1.0, abs(py))
                assert abs(cc[2] - s * c[2]) <= 1e-9 * abs(s * c[2])
                k += 1
        assert k == (e + 1) * per


def test_placement_arguments():
    with pytest.raises(ValueError):
        RL.make_placements(_views(np.random.default_rng(1), 1), 2, CAM10, grid=(0, 3), distances=(1.0,))
    lookup = lambda name: None
    opt = RL.RelocDepth(lookup=lookup, sensor_depth_scale=1e-3)
    assert (opt.tolerance, opt.grid, opt.distances, opt.depth_points, opt.n_geometric, opt.min_in) == (
        0.05, (8, 6), (0.5, 0.71, 1.0, 1.41, 2.0), 256, 512, 0.5)
    for bad in (dict(sensor_depth_scale=0.0), dict(grid=(0, 1)), dict(distances=()), dict(distances=(1.0, -2.0)),
                dict(depth_points=0), dict(n_geometric=0), dict(min_in=1.5), dict(tolerance=float("nan"))):
        with pytest.raises(ValueError):
            RL.RelocDepth(**{**dict(lookup=lookup, sensor_depth_scale=1e-3), **bad})


# ----------------------------------------------------------------------------------------------------- restatement
# a 4 x 3 pinhole camera with f = 1, the principal point on pixel (1.5, 1): a point (x, y, z) lands on u = x / z + 1.5,
# v = y / z + 1.  Scale 0.5 and tolerance 0.5 are exact in float32.
HAND_CAM = ([4.0, 3.0, 1.0, 1.0, 1.5, 1.0, 0.0, 0.0, 0.0, 0.0], 0)
HAND_POINTS = np.array([
    [0.0, 0.0, 2.0],     # "agree": u = 1.5 -> pixel (2, 1), raw 5 -> d = 2.5, r = 0.5 == tolerance
    [-1.5, -1.0, 1.0],   # "behind": pixel (0, 0), raw 10 -> d = 5, r = 4 > tolerance
    [1.5, 1.0, 1.0],     # "unmeasured": pixel (3, 2), the image's last, raw 0
    [-2.0, 0.0, 1.0],    # "edge": u = -0.5, whose rounded pixel is 0 - but the projection's image test refuses u < 0
    [0.0, 0.0, -1.0],    # "behind the camera"
])
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def hand_sensor():
    s = np.full((3, 4), 40, np.uint16)  # far behind wherever no point is aimed
    s[1, 2], s[0, 0], s[2, 3] = 5, 10, 0
    return s


def test_the_restatement_on_the_hand_made_case():
    ref = RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], hand_sensor(), 0.5, 0.5, HAND_CAM)
    pts = ref["points"][0]
    assert pts["inside"].tolist() == [True, True, True, False, False]
    assert pts["measured"].tolist() == [True, True, False, False, False]
    assert pts["agree"].tolist() == [True, False, False, False, False]    # equality agrees
    assert pts["behind"].tolist() == [False, True, False, False, False]
    assert pts["r"].dtype == np.float32 and pts["r"][0] == np.float32(0.5) and pts["r"][1] == np.float32(4.0)
    assert pts["u"][3] == np.float32(-0.5) and not pts["projects"][3] and not pts["projects"][4]
    assert ref["out"].dtype == np.int32 and ref["out"].tolist() == [[3, 2, 1, 1]]
    # a surface in FRONT of the point (r < -tolerance): measured, neither agreeing nor behind
    s = hand_sensor()
    s[0, 0] = 1  # d = 0.5, r = -0.5: still agrees (|r| == tolerance) ...
    assert RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], s, 0.5, 0.5, HAND_CAM)["out"].tolist() == [[3, 2, 2, 0]]
    # ... and one step of the tolerance below it does not: measured, neither agreeing nor behind (while the "agree"
    # point's r = +0.5 is now past the tolerance: behind)
    tol = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], s, 0.5, tol, HAND_CAM)["out"].tolist() == [[3, 2, 0, 1]]


def test_the_restatement_masks_ranges_and_nan():
    s = hand_sensor()
    valid = np.array([1, 0, 1, 1, 1], np.uint8)  # the "behind" point leaves
    poses = np.stack([IDENTITY, IDENTITY, IDENTITY, IDENTITY])
    ranges = [[0, 5], [1, 2], [4, 2], [2, 0]]  # whole, a part, one past the bank, empty
    ref = RL.score_hypotheses_depth_reference(HAND_POINTS, valid, poses, ranges, s, 0.5, 0.5, HAND_CAM)
    assert ref["out"].tolist() == [[2, 1, 1, 0], [1, 0, 0, 0], [-1, -1, -1, -1], [0, 0, 0, 0]]
    assert ref["points"][2] is None
    # a NaN residual (a NaN tolerance here) counts in neither n_agree nor n_behind
    nan = RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], s, 0.5, float("nan"), HAND_CAM)
    assert nan["out"].tolist() == [[3, 2, 0, 0]]
    # float64 runs the same statements
    r64 = RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], s, 0.5, 0.5, HAND_CAM, dtype=np.float64)
    assert r64["points"][0]["r"].dtype == np.float64 and r64["out"].tolist() == [[3, 2, 1, 1]]
    with pytest.raises(ValueError):  # the camera is the sensor's
        RL.score_hypotheses_depth_reference(HAND_POINTS, None, IDENTITY[None], [[0, 5]], np.zeros((4, 4), np.uint16), 0.5, 0.5, HAND_CAM)


def test_the_depth_ranking_rule():
    import torch

    out = torch.tensor([[10, 10, 5, 0], [4, 4, 4, 0], [10, 9, 5, 1], [-1, -1, -1, -1], [0, 0, 0, 0], [5, 5, 5, 0]], dtype=torch.int32)
    counts = torch.tensor([10, 10, 10, 10, 0, 10], dtype=torch.int32)
    score = RL.rank_depth_scores(out, counts, 0.5)
    assert score.tolist() == [0.5, float("-inf"), 0.5, float("-inf"), float("-inf"), 0.5]  # 4 of 10 inside: below min_in
    assert RL.best_candidates(score, 4).tolist() == [0, 2, 5, 1]  # ties by index; the unranked ones last, by index too
    assert RL.best_candidates(score, 99).numel() == 6


# ----------------------------------------------------------------------------------------------------- ABI surface
def test_the_entry_point_is_declared_bound_and_keeps_the_abi_version():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pixtrack_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+pxt_score_pose_hypotheses_depth\s*\(", text)
    restype, argtypes = _lib.PROTOTYPES["pxt_score_pose_hypotheses_depth"]
    assert restype is _lib.C.c_int and len(argtypes) == 13
    assert argtypes[7] is _lib.C.c_float and argtypes[8] is _lib.C.c_float
    L = _lib.lib()
    assert L.pxt_version() == 13 == _lib.ABI_VERSION
    # the bounds that need no device memory: every one is PXT_E_ARG before anything is launched
    bank = _lib.RelocBank(64, None, None, 10)
    cam = (_lib.C.c_float * 10)(64, 48, 50, 50, 31.5, 23.5, 0, 0, 0, 0)
    ok = dict(bank=_lib.C.byref(bank), poses=1024, ranges=1024, M=4, sensor=1024, W=64, H=48, ndist=0, out=1024, cam=cam)

    def call(**kw):
        a = {**ok, **kw}
        return L.pxt_score_pose_hypotheses_depth(a["bank"], a["poses"], a["ranges"], a["M"], a["sensor"], a["W"], a["H"], 1e-3,
                                                 0.01, a["cam"], a["ndist"], a["out"], None)

    bad = [dict(bank=None), dict(poses=None), dict(ranges=None), dict(sensor=None), dict(out=None), dict(cam=None), dict(M=0),
           dict(M=-1), dict(M=(1 << 22) + 1), dict(W=0), dict(H=0), dict(W=1 << 15, H=(1 << 13) + 1), dict(ndist=1),
           dict(ndist=3), dict(ndist=5), dict(poses=1032), dict(out=1032), dict(ranges=1028), dict(sensor=1025),
           dict(W=63), dict(bank=_lib.C.byref(_lib.RelocBank(None, None, None, 10))),
           dict(bank=_lib.C.byref(_lib.RelocBank(64, None, None, 0)))]
    for kw in bad:
        assert call(**kw) == -1, kw


# ----------------------------------------------------------------------------------------------------- constructor rules
def test_the_constructor_rules_of_the_mesh_relocaliser():
    from pixtrack_amd.depth_refinement import DepthRefine
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.occlusion import OcclusionMask
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    mesh = object.__new__(MeshTemplate)
    lookup, other = (lambda name: None), (lambda name: None)
    new = lambda **kw: PixLocPoseTrackerR9("/nonexistent", "/nonexistent", "/nonexistent", "/nonexistent", **kw)
    # what was refused stays refused
    with pytest.raises(ValueError, match=r"mesh template.*relocalizer"):
        new(template=mesh, relocalizer="views")
    with pytest.raises(ValueError, match=r"relocalizer"):
        new(template=mesh, relocalizer="views", reference_points="template")
    with pytest.raises(ValueError, match=r"depth_refine.*relocalizer"):
        new(relocalizer="views", depth_refine=DepthRefine(lookup=lookup, sensor_depth_scale=1e-3))
    with pytest.raises(ValueError, match=r"occlusion.*relocalizer"):
        new(relocalizer="views", occlusion=OcclusionMask(lookup=lookup, sensor_depth_scale=1e-3))
    # "mesh" needs a mesh template, and the depth stage needs "mesh"
    for template in (None, "nerf"):
        with pytest.raises(ValueError, match=r"relocalizer='mesh'.*MeshTemplate"):
            new(relocalizer="mesh", template=template)
    with pytest.raises(ValueError, match=r"reference_points='render'"):
        new(relocalizer="mesh", template=mesh, reference_points="render")
    depth = RL.RelocDepth(lookup=lookup, sensor_depth_scale=1e-3)
    for kw in (dict(), dict(relocalizer="views"), dict(relocalizer="off", template=mesh)):
        with pytest.raises(ValueError, match=r"reloc_depth.*relocalizer='mesh'"):
            new(reloc_depth=depth, **kw)
    with pytest.raises(ValueError, match=r"reloc_depth: a relocalizer.RelocDepth"):
        new(relocalizer="mesh", template=mesh, reloc_depth=OcclusionMask(lookup=lookup, sensor_depth_scale=1e-3))
    # one sensor image per frame: the same lookup and scale as the other sensor options
    mk = dict(relocalizer="mesh", template=mesh, reference_points="template", reloc_depth=depth)
    with pytest.raises(ValueError, match=r"reloc_depth and depth_refine.*same\s+lookup"):
        new(depth_refine=DepthRefine(lookup=other, sensor_depth_scale=1e-3), **mk)
    with pytest.raises(ValueError, match=r"reloc_depth and depth_refine.*same\s+lookup"):
        new(depth_refine=DepthRefine(lookup=lookup, sensor_depth_scale=2e-3), **mk)
    with pytest.raises(ValueError, match=r"reloc_depth and occlusion.*same\s+lookup"):
        new(occlusion=OcclusionMask(lookup=other, sensor_depth_scale=1e-3), **mk)


def test_the_command_line_names_the_option():
    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as cli

    args = cli.build_parser().parse_args(["--object_path", "o", "--query", "q", "--out_dir", "d", "--relocalize", "mesh",
                                          "--relocalize_depth", "--sensor_depth_dir", "s", "--sensor_depth_scale", "0.001"])
    assert args.relocalize == "mesh" and args.relocalize_depth
    opt = cli.reloc_depth_option_from_args(args)
    assert isinstance(opt, RL.RelocDepth) and opt.sensor_depth_scale == 0.001
    args.depth_refine, args.depth_prior = True, None
    assert cli.depth_option_from_args(args).lookup is opt.lookup  # ONE lookup for every sensor option
    plain = cli.build_parser().parse_args(["--object_path", "o", "--query", "q", "--out_dir", "d"])
    assert plain.relocalize == "off" and cli.reloc_depth_option_from_args(plain) is None
    with pytest.raises(ValueError, match="--relocalize_depth needs --sensor_depth_dir"):
        cli.reloc_depth_option_from_args(cli.build_parser().parse_args(
            ["--object_path", "o", "--query", "q", "--out_dir", "d", "--relocalize", "mesh", "--relocalize_depth"]))
