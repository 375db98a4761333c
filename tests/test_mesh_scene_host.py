"""Mutual occlusion between the objects of one image: the properties of mesh_render.scene_reference and
occlusion.mask_exclude_reference, the declarations, and every PXT_E_ARG bound of pxt_mesh_render_scene_batch.  No GPU.

The fixture scene (70 x 37, fx 60, fy 58, cx 34.8, cy 17.6, R = I, depth_q = 1): A = icosphere(2) * 0.1 at
(0.01, -0.02, 0.45) covers 560 pixels; B = icosphere(1) * 0.12 at (0.07, 0.01, 0.60) covers 418, of which A hides 311;
C = A's mesh at (-0.20, 0, 0.45) covers 490, disjoint from both; A2 = A's mesh at A's view ties A on all 560 pixels."""
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import mesh_render as R

ROOT = Path(__file__).resolve().parent.parent
W, H = 70, 37
T_A, T_B, T_C = (0.01, -0.02, 0.45), (0.07, 0.01, 0.60), (-0.20, 0.0, 0.45)


def scene_view(t, near=1e-6, depth_q=1.0, fx=60.0, fy=58.0, cx=34.8, cy=17.6):
    return R.pack_view(np.eye(3), t, fx, fy, cx, cy, near, depth_q)


def grey(V, level=0.5):
    return {"colors": np.full((len(V), 3), level, np.float32)}


def fixture_items(want=("depth_nz",)):
    """{name: (V, F, shading, [the object's scene view])} for A, B, C, A2."""
    Va, Fa = R.icosphere(2)
    Vb, Fb = R.icosphere(1)
    Va, Vb = Va * 0.1, Vb * 0.12
    item = lambda V, F, t: (V, F, grey(V), [(scene_view(t), W, H, 1, tuple(want))])
    return {"A": item(Va, Fa, T_A), "B": item(Vb, Fb, T_B), "C": item(Va, Fa, T_C), "A2": item(Va, Fa, T_A)}


def mutual_pair(want=("depth_nz",), offset=0.1):
    """Two radius-0.1 spheres at equal z, `offset` apart in x: each hides part of the other."""
    V, F = R.icosphere(2)
    V = V * 0.1
    return [(V, F, grey(V), [(scene_view((-offset / 2, 0.0, 0.5)), W, H, 1, tuple(want))]),
            (V, F, grey(V), [(scene_view((offset / 2, 0.0, 0.5)), W, H, 1, tuple(want))])]


@pytest.fixture(scope="module")
def fixture():
    items = fixture_items()
    names = list(items)
    out = R.scene_reference([items[n] for n in names], [[0]] * 4, 0)
    return dict(items=items, names=names, out={n: o[0] for n, o in zip(names, out)})


def counts(res):
    r = res["records"]
    return int(r[R.W_COVERED]), int(r[R.W_HIDDEN]), int(r[R.W_OCCLUDER])


def test_the_fixture_scenes_counts(fixture):
    out = fixture["out"]
    assert counts(out["A"]) == (560, 0, 0)
    assert counts(out["B"]) == (418, 311, 311)  # 107 stay visible
    assert counts(out["C"]) == (490, 0, 0)
    assert counts(out["A2"]) == (560, 0, 0)  # equal bits do not hide: A and A2 tie on all 560 pixels
    for n, o in out.items():
        assert o["occluder"].dtype == np.uint8 and o["occluder"].shape == (H, W) and set(np.unique(o["occluder"])) <= {0, 1}
        assert int(o["occluder"].sum()) == counts(o)[2]
    # what hides B is A's silhouette: the hidden pixels are covered by both
    assert not (out["B"]["occluder"].astype(bool) & ~(out["A"]["depth_nz"].astype(bool) & out["B"]["depth_nz"].astype(bool))).any()
    assert not (out["C"]["depth_nz"].astype(bool) & (out["A"]["depth_nz"] | out["B"]["depth_nz"]).astype(bool)).any()


def test_the_plane_does_not_depend_on_the_members_order(fixture):
    items, names, want = fixture["items"], fixture["names"], fixture["out"]
    for order in ([2, 0, 3, 1], [3, 2, 1, 0]):
        got = R.scene_reference([items[names[k]] for k in order], [[5]] * 4, 0)  # ... nor on the scene's number
        for k, g in zip(order, got):
            assert np.array_equal(g[0]["occluder"], want[names[k]]["occluder"])
            assert np.array_equal(g[0]["records"], want[names[k]]["records"])


def test_a_scene_of_one_member_is_all_zeros_and_views_outside_a_scene_are_unchanged(fixture):
    items = fixture["items"]
    plain = R.frame_batch_reference([items["A"], items["B"]])
    got = R.scene_reference([items["A"], items["B"]], [[None], [3]], 2)
    assert "occluder" not in got[0][0] and np.array_equal(got[0][0]["records"], plain[0][0]["records"])
    assert not got[1][0]["occluder"].any() and counts(got[1][0]) == (418, 0, 0)
    # two scenes of one member each hide nothing of each other
    got = R.scene_reference([items["A"], items["B"]], [[0], [1]], 2)
    assert not got[0][0]["occluder"].any() and not got[1][0]["occluder"].any()
    # every plane but the occluder, and record words 0..9, are frame_batch_reference's
    got = R.scene_reference([items["A"], items["B"]], [[0], [0]], 3)
    for g, p in zip(got, plain):
        assert np.array_equal(g[0]["depth_nz"], p[0]["depth_nz"]) and np.array_equal(g[0]["records"][:10], p[0]["records"][:10])
        assert not p[0]["records"][10:].any() and not g[0]["records"][12:].any()


def test_growth_contains_the_hidden_pixels_stops_at_the_border_and_is_monotone(fixture):
    items = fixture["items"]
    # B moved so that what A hides of it touches the image's right border
    Vb, Fb, sb, _ = items["B"]
    Va, Fa, sa, _ = items["A"]
    a = (Va, Fa, sa, [(scene_view((0.21, -0.02, 0.45)), W, H, 1, ("depth_nz",))])
    b = (Vb, Fb, sb, [(scene_view((0.27, 0.01, 0.60)), W, H, 1, ("depth_nz",))])
    planes, n = {}, {}
    for r in (0, 1, 3):
        res = R.scene_reference([a, b], [[0], [0]], r)[1][0]
        planes[r], n[r] = res["occluder"].astype(bool), counts(res)
        assert n[r][1] == n[0][1] and n[r][2] == planes[r].sum()  # n_hidden does not grow
    assert planes[0][:, W - 1].any() and n[0][1] > 50
    assert not (planes[0] & ~planes[1]).any() and not (planes[1] & ~planes[3]).any()
    assert n[0][2] < n[1][2] < n[3][2]
    assert np.array_equal(planes[3], R.dilate_box(planes[0], 3)) and planes[3].shape == (H, W)
    # a full row of growth inside the image would add (2 r + 1) columns; at the border it adds fewer
    rows = planes[0].any(1)
    assert planes[3][rows].sum(1).max() <= planes[0][rows].sum(1).max() + 3


def test_each_of_the_mutual_pair_hides_part_of_the_other():
    got = R.scene_reference(mutual_pair(), [[0], [0]], 0)
    (ca, ha, _), (cb, hb, _) = counts(got[0][0]), counts(got[1][0])
    assert ha > 20 and hb > 20 and ha < ca and hb < cb
    assert not (got[0][0]["occluder"] & got[1][0]["occluder"]).any()  # a pixel shows one of the two


def test_near_and_depth_q_may_differ_but_the_camera_may_not(fixture):
    items = fixture["items"]
    Vb, Fb, sb, _ = items["B"]
    b = (Vb, Fb, sb, [(scene_view(T_B, near=1e-3, depth_q=0.25), W, H, 1, ("depth_nz", "depth"))])
    got = R.scene_reference([items["A"], b], [[0], [0]], 0)
    assert counts(got[1][0]) == (418, 311, 311)  # z is compared unscaled
    for bad in (dict(fx=60.5), dict(cy=17.5)):
        b = (Vb, Fb, sb, [(scene_view(T_B, **bad), W, H, 1, ("depth_nz",))])
        with pytest.raises(ValueError, match="camera"):
            R.scene_reference([items["A"], b], [[0], [0]], 0)
    b = (Vb, Fb, sb, [(scene_view(T_B), W, H - 1, 1, ("depth_nz",))])
    with pytest.raises(ValueError, match="camera"):
        R.scene_reference([items["A"], b], [[0], [0]], 0)
    b = (Vb, Fb, sb, [(scene_view(T_B), W, H, 2, ("rgb_u8",))])
    with pytest.raises(ValueError, match="supersample"):
        R.scene_reference([items["A"], b], [[0], [0]], 0)
    for r in (-1, 9):
        with pytest.raises(ValueError, match="r_grow"):
            R.scene_reference([items["A"]], [[0]], r)
    with pytest.raises(ValueError, match="scenes"):
        R.scene_reference([items["A"]], [[0], [0]], 0)


def test_mask_exclude_reference():
    from pixtrack_amd.occlusion import mask_exclude_reference

    rng = np.random.default_rng(3)
    m = (rng.integers(0, 3, (37, 70)) * 100).astype(np.uint8)  # 0, 100, 200: != 0 counts as 1
    g = rng.integers(0, 2, (37, 70)).astype(np.uint8)
    out = mask_exclude_reference(m, g)
    assert out["mask"].dtype == np.uint8 and set(np.unique(out["mask"])) == {0, 1}
    assert np.array_equal(out["mask"].astype(bool), (m != 0) & (g == 0))
    assert out["record"] == (int((m != 0).sum()), int(out["mask"].sum())) and out["record"][1] < out["record"][0]
    assert not (out["mask"] & g).any()
    assert np.array_equal(mask_exclude_reference(m, np.zeros_like(g))["mask"], (m != 0).astype(np.uint8))
    assert not mask_exclude_reference(m, g * 7)["mask"][g != 0].any()  # the occluder too: != 0 counts as set
    with pytest.raises(ValueError):
        mask_exclude_reference(m, g[:-1])


def test_the_entry_points_and_the_ops_are_declared():
    from pixtrack_amd import _lib, ops

    header = (ROOT / "include" / "pixtrack_hip.h").read_text()
    for name in ("pxt_mesh_render_scene_batch", "pxt_mesh_render_scene_batch_workspace_bytes", "pxt_mask_exclude"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    assert re.search(r"#define\s+PXT_MESH_SCENE_MAX_GROW\s+8\b", header) and _lib.PXT_MESH_SCENE_MAX_GROW == 8 == R.SCENE_MAX_GROW
    assert {"mesh_render_scene_batch", "mask_exclude"} <= set(ops.op_names())
    L, C = _lib.lib(), _lib.C
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)
    args = ([20, 80], [0, 1, 1], [8, 8, 1, 8, 8, 1, 5, 7, 2])
    size = lambda f: int(f(len(args[0]), i32(args[0]), len(args[1]), i32(args[1]), i32(args[2])))
    plain, scene = size(L.pxt_mesh_render_frame_batch_workspace_bytes), size(L.pxt_mesh_render_scene_batch_workspace_bytes)
    assert plain > 0 and scene > plain and (scene - plain) % 16 == 0  # the scene table rides behind the parameter record
    assert int(L.pxt_mesh_render_scene_batch_workspace_bytes(1, i32([20]), 1, i32([0]), i32([8, 8, 3]))) == -1


# ----------------------------------------------------------------------------------------------------------------------
# the bounds: PXT_E_ARG comes from the host-side checks ahead of the first HIP call, so nothing is dereferenced and
# device pointers can be stood in for by aligned numbers
# ----------------------------------------------------------------------------------------------------------------------
BASE = 1 << 20  # a 16-byte aligned stand-in for device memory


def scene_call(view_scene, r_grow=0, occluder_offsets=None, geometry=(8, 8, 1, 8, 8, 1), cameras=None, occluder=BASE,
               occluder_bytes=1 << 16, null=()):
    from pixtrack_amd import _lib

    L, C = _lib.lib(), _lib.C
    P = len(geometry) // 3
    desc = (_lib.MeshDesc * 1)()
    desc[0].vertices, desc[0].triangles, desc[0].colors, desc[0].n_vertices, desc[0].n_triangles = BASE, BASE, BASE, 12, 20
    views = np.zeros((P, 20), np.float32)
    for p in range(P):
        views[p] = scene_view((0.0, 0.0, 0.5), *(() if cameras is None else (1e-6, 1.0) + tuple(cameras[p])))
    offsets = []
    for p in range(P):
        S = geometry[3 * p + 2]
        offsets += [-1, 1024 * p, -1, -1] if S != 1 else [-1, -1, -1, 1024 * p]
    if occluder_offsets is None:
        occluder_offsets = [1024 * p if s >= 0 else -1 for p, s in enumerate(view_scene)]
    vs = None if "view_scene" in null else (C.c_int32 * len(view_scene))(*view_scene)
    oo = None if "occluder_offsets" in null else (C.c_int64 * len(occluder_offsets))(*occluder_offsets)
    return L.pxt_mesh_render_scene_batch(
        desc, 1, (C.c_int32 * P)(*([0] * P)), views.ctypes.data, P, (C.c_int32 * (3 * P))(*geometry),
        (C.c_int64 * (4 * P))(*offsets), None, BASE, None, BASE, (C.c_int64 * 4)(0, 1 << 16, 0, 1 << 16), vs, r_grow,
        occluder, occluder_bytes, oo, BASE, BASE, None)


BAD_SCENE_CALLS = {
    "a member with S = 2": dict(view_scene=[0, 0], geometry=(8, 8, 1, 8, 8, 2)),
    "a member with S = 4": dict(view_scene=[0, 0], geometry=(8, 8, 4, 8, 8, 1), occluder_offsets=[-1, 0]),
    "members that differ in width": dict(view_scene=[0, 0], geometry=(8, 8, 1, 12, 8, 1)),
    "members that differ in height": dict(view_scene=[1, 1], geometry=(8, 8, 1, 8, 9, 1)),
    "members that differ in fx": dict(view_scene=[0, 0], cameras=[(60, 58, 3.5, 3.5), (60.00001, 58, 3.5, 3.5)]),
    "members that differ in fy": dict(view_scene=[0, 0], cameras=[(60, 58, 3.5, 3.5), (60, 58.5, 3.5, 3.5)]),
    "members that differ in cx": dict(view_scene=[0, 0], cameras=[(60, 58, 3.5, 3.5), (60, 58, 3.25, 3.5)]),
    "members that differ in cy": dict(view_scene=[0, 0], cameras=[(60, 58, 3.5, 3.5), (60, 58, 3.5, -3.5)]),
    "a scene id of P": dict(view_scene=[2, -1]),
    "a scene id below -1": dict(view_scene=[-2, 0]),
    "an occluder offset on a view in no scene": dict(view_scene=[0, -1], occluder_offsets=[0, 1024]),
    "r_grow = -1": dict(view_scene=[0, 0], r_grow=-1),
    "r_grow = 9": dict(view_scene=[0, 0], r_grow=9),
    "a plane that is not 4-byte aligned": dict(view_scene=[0, 0], occluder_offsets=[0, 1022]),
    "a plane that does not fit the buffer": dict(view_scene=[0, 0], occluder_bytes=1024 + 63),
    "a plane without a buffer": dict(view_scene=[0, 0], occluder=None),
    "an occluder base that is not 4-byte aligned": dict(view_scene=[0, 0], occluder=BASE + 2),
    "no view_scene": dict(view_scene=[0, 0], null=("view_scene",)),
    "no occluder_offsets": dict(view_scene=[0, 0], null=("occluder_offsets",)),
}


@pytest.mark.parametrize("case", sorted(BAD_SCENE_CALLS))
def test_the_scene_calls_bounds_are_argument_errors(case):
    assert scene_call(**BAD_SCENE_CALLS[case]) == -1  # PXT_E_ARG: nothing is launched or written


def test_the_ops_tensor_free_scene_checks():
    from pixtrack_amd import _lib, ops

    geo = [8, 8, 1, 8, 8, 1, 5, 7, 2]
    assert ops.mesh_scene_planes([0, 0, -1], 2, [0, 64, -1], geo) == 128
    assert ops.mesh_scene_planes([2, -1, -1], 0, [64, -1, -1], geo) == 128  # a scene id is any number in [0, P)
    assert ops.mesh_scene_planes([-1, -1, -1], 8, [-1, -1, -1], geo) == 0
    assert ops.mesh_scene_planes([0, 0, -1], 0, [-1, -1, -1], geo) == 0     # members that want no plane
    bad = [([0, 0], 0, [0, 64], geo), ([0, 0, -1], 0, [0, 64], geo),          # one number per view
           ([0, 0, -1], -1, [0, 64, -1], geo), ([0, 0, -1], 9, [0, 64, -1], geo),
           ([3, 0, -1], 0, [0, 64, -1], geo), ([-2, 0, -1], 0, [-1, 64, -1], geo),
           ([0, -1, -1], 0, [0, 64, -1], geo),                                 # a plane on a view in no scene
           ([0, -1, 0], 0, [0, -1, 64], geo),                                  # S = 2 in a scene
           ([0, 0, -1], 0, [0, 64, -1], [8, 8, 1, 8, 12, 1, 5, 7, 2]),         # two sizes in one scene
           ([0, 0, -1], 0, [0, 62, -1], geo), ([0, 0, -1], 0, [0, 32, -1], geo)]  # alignment, overlap
    for view_scene, r_grow, offsets, geometry in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_scene_planes(view_scene, r_grow, offsets, geometry)


# ----------------------------------------------------------------------------------------------------------------------
# MultiObjectTracker(mutual_occlusion=...): what the constructor refuses, and the command line
# ----------------------------------------------------------------------------------------------------------------------
def stand_in(template, camera=None):
    import torch

    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    tr = object.__new__(PixLocPoseTrackerR9)
    tr.device, tr.reference_points, tr.depth_refine, tr.occlusion, tr.template = torch.device("cpu"), "sfm", None, None, template
    tr.camera = camera
    return tr


def pinhole(w=160, h=96, f=192.0, cx=80.0, cy=48.0, k=0.0):
    from pixtrack_amd.geometry import Camera

    return Camera.from_colmap(dict(model="SIMPLE_RADIAL", width=w, height=h, params=np.array([f, cx, cy, k])))


def test_the_lock_step_tracker_refuses_bad_scenes_before_it_touches_a_tracker():
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MUTUAL_HISTORY_KEYS, MultiObjectTracker, MutualOcclusion

    mesh = lambda cam=None: stand_in(object.__new__(MeshTemplate), cam)
    assert MutualOcclusion(scenes=[0, 0]).r_grow == 2 and len(MUTUAL_HISTORY_KEYS) == 5
    with pytest.raises(ValueError, match="no mesh template"):  # a NeRF-template tracker in a scene
        MultiObjectTracker([mesh(), stand_in(None)], mutual_occlusion=MutualOcclusion(scenes=["a", "a"]))
    with pytest.raises(ValueError, match="one scene .* per tracker"):
        MultiObjectTracker([mesh(), mesh()], mutual_occlusion=MutualOcclusion(scenes=[0]))
    for r in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="r_grow"):
            MultiObjectTracker([mesh(), mesh()], mutual_occlusion=MutualOcclusion(scenes=[0, 0], r_grow=r))
    for other in (pinhole(w=128), pinhole(f=190.0), pinhole(cy=47.5), pinhole(k=0.01)):
        with pytest.raises(ValueError, match="different query cameras"):
            MultiObjectTracker([mesh(pinhole()), mesh(other)], mutual_occlusion=MutualOcclusion(scenes=[0, 0]))
    with pytest.raises(ValueError, match="lens terms"):
        MultiObjectTracker([mesh(pinhole(k=0.01)), mesh()], mutual_occlusion=MutualOcclusion(scenes=[0, 0]))
    # a valid option passes the checks: the stand-ins then fail on the first attribute they lack, as without the option
    for option in (None, MutualOcclusion(scenes=[0, 0]), MutualOcclusion(scenes=[None, None]),
                   MutualOcclusion(scenes=[0, None])):
        with pytest.raises(AttributeError):
            MultiObjectTracker([mesh(pinhole()), mesh(pinhole())], mutual_occlusion=option)
    # a NeRF-template tracker outside every scene is fine
    with pytest.raises(AttributeError):
        MultiObjectTracker([mesh(), mesh(), stand_in(None)], mutual_occlusion=MutualOcclusion(scenes=[0, 0, None]))


def test_the_command_lines_mutual_occlusion_arguments():
    from pixtrack_amd.pose_trackers.multi_object_tracker import build_parser, mutual_occlusion_from_args

    base = ["--object_path", "a", "b", "c", "--out_dir", "da", "db", "dc"]
    args = build_parser().parse_args(base + ["--query", "q", "q", "r"])
    assert args.mutual_occlusion is False and args.mutual_occlusion_grow == 2 and mutual_occlusion_from_args(args) is None
    args = build_parser().parse_args(base + ["--query", "q", "q/", "r", "--template", "mesh", "--mutual_occlusion"])
    option = mutual_occlusion_from_args(args)
    assert option.r_grow == 2 and option.scenes[0] == option.scenes[1] is not None and option.scenes[2] is None
    args = build_parser().parse_args(base + ["--query", "q", "r", "s", "--template", "mesh", "--mutual_occlusion",
                                             "--mutual_occlusion_grow", "4"])
    option = mutual_occlusion_from_args(args)
    assert option.r_grow == 4 and option.scenes == [None, None, None]
    with pytest.raises(ValueError, match="--template mesh"):
        mutual_occlusion_from_args(build_parser().parse_args(base + ["--query", "q", "q", "r", "--mutual_occlusion"]))
