"""The numpy restatement of pxt_mesh_render_frame (mesh_render.supersampled_view, frame_reference), the declarations, the
tracker's refusals of what a mesh template is not combined with yet, and the parser's defaults.  No GPU."""
import numpy as np
import pytest

from pixtrack_amd import mesh_render as R
from test_mesh_raster_host import SPHERE_VIEW, rotation, view
from test_mesh_shade_host import colours
from test_mesh_texture_host import corner_uvs, random_texture


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_supersampled_view_gives_the_stated_floats():
    v = view(Rm=rotation(3), fx=77.3, fy=75.9, cx=31.37, cy=23.61, t=(0.013, -0.007, 0.6), near=0.01, depth_q=0.7)
    f32 = np.float32
    for S in (1, 2, 4):
        w = R.supersampled_view(v, S)
        assert w.dtype == np.float32 and w.shape == (20,)
        want = v.copy()
        want[12], want[13] = v[12] * f32(S), v[13] * f32(S)
        want[14] = f32(v[14] * f32(S)) + f32(0.5) * f32(S - 1)
        want[15] = f32(v[15] * f32(S)) + f32(0.5) * f32(S - 1)
        assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.supersampled_view(v, 1), v)
    # fine pixel (S i + a, S j + b) is the sample of pixel (i, j) at offset ((a + .5) / S - .5, (b + .5) / S - .5)
    w = R.supersampled_view(view(fx=50.0, fy=40.0, cx=10.0, cy=7.0), 4).astype(np.float64)
    i, j, a, b = 3, 5, 1, 2
    x, y = (4 * i + a - w[14]) / w[12], (4 * j + b - w[15]) / w[13]  # the ray of the fine pixel
    assert np.allclose([x * 50.0 + 10.0, y * 40.0 + 7.0], [i + (a + 0.5) / 4 - 0.5, j + (b + 0.5) / 4 - 0.5], atol=1e-12)
    with pytest.raises(ValueError):
        R.supersampled_view(v, 3)


def scene():
    V, F = R.icosphere(2)
    return V * 0.1, F, view(Rm=rotation(0), **SPHERE_VIEW), 33, 25


def shadings(V, F):
    UV, FUV = corner_uvs(len(F))
    return [{"colors": colours(len(V))}, {"uvs": UV, "triangle_uvs": FUV, "texture": random_texture()}]


def existing(V, F, shading, views, W, H):
    if "colors" in shading:
        return R.shade_reference(V, F, shading["colors"], views, W, H)
    return R.shade_textured_reference(V, F, shading["uvs"], shading["triangle_uvs"], shading["texture"], views, W, H)


def test_supersample_1_is_the_existing_rule_on_every_output():
    V, F, v, W, H = scene()
    for shading in shadings(V, F):
        rgba, u8, depth, nz, _, rec = existing(V, F, shading, v[None], W, H)
        got = R.frame_reference(V, F, shading, [(v, W, H, 1, R.FRAME_OUTPUTS)])[0]
        assert sorted(got) == ["depth", "depth_nz", "records", "rgb_u8", "rgba"]
        for name, want in (("rgba", rgba), ("rgb_u8", u8), ("depth", depth), ("depth_nz", nz)):
            assert got[name].dtype == want.dtype and np.array_equal(bits(got[name]), bits(want[0])), name
        assert np.array_equal(got["records"], rec[0]) and rec[0, R.W_COVERED] > 100


@pytest.mark.parametrize("S", [2, 4])
def test_supersampled_renders_are_the_box_sum_written_out(S):
    V, F, v, W, H = scene()
    f32 = np.float32
    for shading in shadings(V, F):
        fine = existing(V, F, shading, R.supersampled_view(v, S)[None], W * S, H * S)
        rgba = fine[0][0]
        want = np.zeros((H, W, 4), np.float32)
        for j in range(H):
            for i in range(W):
                for ch in range(4):
                    acc = rgba[S * j, S * i, ch]
                    for b in range(S):
                        for a in range(S):
                            if a or b:
                                acc = f32(acc + rgba[S * j + b, S * i + a, ch])
                    want[j, i, ch] = f32(acc * f32(1.0 / (S * S)))
        got = R.frame_reference(V, F, shading, [(v, W, H, S, ("rgba", "rgb_u8"))])[0]
        assert sorted(got) == ["records", "rgb_u8", "rgba"]
        assert np.array_equal(got["rgba"].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got["rgb_u8"], ((want[..., :3] * f32(255.0)).astype(np.int64) & 255).astype(np.uint8))
        assert np.array_equal(got["records"], fine[5][0]) and got["records"][R.W_COVERED] > 100 * S * S
        # premultiplied over black: no colour without coverage, none above it
        assert (got["rgba"][..., :3] <= got["rgba"][..., 3:]).all() and got["rgb_u8"].max() > 100


def test_requests_are_independent_and_checked():
    V, F, v, W, H = scene()
    shading = shadings(V, F)[0]
    a = (v, W, H, 2, ("rgba",))
    b = (view(**SPHERE_VIEW), 17, 21, 1, ("depth_nz", "rgb_u8"))
    both = R.frame_reference(V, F, shading, [a, b])
    for got, solo in zip(both, (R.frame_reference(V, F, shading, [a])[0], R.frame_reference(V, F, shading, [b])[0])):
        assert sorted(got) == sorted(solo) and all(np.array_equal(bits(got[k]), bits(solo[k])) for k in got)
    for bad in ((v, W, H, 3, ("rgba",)), (v, W, H, 2, ("depth",)), (v, W, H, 4, ("rgb_u8", "depth_nz")), (v, W, H, 1, ()),
                (v, W, H, 1, ("ids",)), (v, 0, H, 1, ("rgba",)), (v, 1 << 13, (1 << 11) + 1, 4, ("rgba",))):
        with pytest.raises(ValueError):
            R.frame_reference(V, F, shading, [bad])


def probe(S):
    # an icosphere(2) of radius 0.1 wider than the 23 x 41 image: a silhouette that leaves it left and right (the
    # principal point is this test's choice)
    V, F = R.icosphere(2)
    v = view(fx=60.0, fy=58.0, cx=11.3, cy=19.6, t=(0.01, -0.02, 0.45))
    return R.frame_reference(V * 0.1, F, {"colors": colours(len(V))}, [(v, 23, 41, S, ("rgba",))])[0]


def test_the_probe_scene_has_a_fractional_silhouette():
    covered = int(probe(1)["records"][R.W_COVERED])
    assert covered > 450
    for S in (2, 4):
        got = probe(S)
        alpha = got["rgba"][..., 3]
        steps = alpha * np.float32(S * S)
        assert np.array_equal(steps, np.rint(steps)) and steps.min() >= 0 and steps.max() == S * S  # multiples of 1 / S^2
        fractional = (alpha > 0) & (alpha < 1)
        print(f"S={S}: {int(fractional.sum())} fractional pixels, {int((alpha == 1).sum())} full, alpha sum {float(alpha.sum())}, "
              f"S=1 covered {covered}")
        assert fractional.sum() >= 40
        assert abs(float(alpha.sum(dtype=np.float64)) - covered) <= 0.02 * covered
        assert got["records"][R.W_COVERED] == int(steps.sum(dtype=np.float64))  # the record counts fine pixels
    assert set(np.unique(probe(4)["rgba"][..., 3] * 16).astype(int)) == set(range(17))  # every sixteenth is there


def test_the_entry_points_and_the_op_are_declared():
    from pixtrack_amd import _lib, ops

    assert _lib.ABI_VERSION == 13
    assert {"pxt_mesh_render_frame", "pxt_mesh_render_frame_workspace_bytes"} <= set(_lib.PROTOTYPES)
    assert "mesh_render_frame" in ops.op_names()
    L = _lib.lib()
    one = lambda *g: L.pxt_mesh_render_frame_workspace_bytes(len(g) // 3, 20, (_lib.C.c_int32 * len(g))(*g))
    assert one(8, 8, 1) > 0 and one(8, 8, 4) > one(8, 8, 2) > one(8, 8, 1)
    assert one(8, 8, 1, 5, 7, 2) > one(8, 8, 1)
    assert one(8, 8, 3) == -1 and one(1 << 13, (1 << 11) + 1, 4) == -1 and one(*([4, 4, 1] * 9)) == -1
    assert ops.mesh_frame_planes([8, 8, 2, 5, 7, 1], [0, -1, -1, -1, -1, 0, -1, 0]) == (2, [8 * 8 * 16, 5 * 7 * 3, 0, 5 * 7])
    for geometry, offsets in (([8, 8, 3], [0, -1, -1, -1]), ([8, 8, 2], [-1, -1, -1, 0]), ([8, 8, 1], [-1, -1, -1, -1]),
                              ([8, 8, 1], [8, -1, -1, -1]), ([8, 8, 1], [-1, 2, -1, -1]), ([8, 8, 1] * 9, [0, -1, -1, -1] * 9),
                              ([8, 8, 1, 8, 8, 1], [0, -1, -1, -1, 16, -1, -1, -1]), ([8, 8], [0, -1, -1, -1])):
        with pytest.raises(_lib.PxtError):
            ops.mesh_frame_planes(geometry, offsets)


class _Unbuilt:
    """Stands in for a MeshTemplate where the constructor must refuse before it builds anything."""


def test_the_tracker_refuses_what_a_mesh_template_is_not_combined_with():
    from pixtrack_amd import mesh_template
    from pixtrack_amd.depth_refinement import DepthRefine
    from pixtrack_amd.occlusion import OcclusionMask
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.pose_trackers.pixloc_tracker_ycb import PixLocPoseTrackerYCB

    template = object.__new__(mesh_template.MeshTemplate)  # never drawn with: the refusals come first
    lookup = lambda name: None
    kw = dict(object_path="/nonexistent", data_path="/nonexistent", loc_path="/nonexistent", eval_path="/nonexistent")
    for option, word in ((dict(relocalizer="views"), "relocalizer"), (dict(reference_points="render"), "reference_points"),
                         (dict(depth_refine=DepthRefine(lookup=lookup, sensor_depth_scale=0.001)), "depth_refine"),
                         (dict(occlusion=OcclusionMask(lookup=lookup, sensor_depth_scale=0.001)), "occlusion")):
        with pytest.raises(ValueError, match="mesh template.*" + word):
            PixLocPoseTrackerR9(template=template, **option, **kw)
    with pytest.raises(ValueError, match="template must be"):  # the YCB policy hands the option on
        PixLocPoseTrackerYCB(template="mesh", **kw)
    for bad in ("mesh", "ngp", 3, _Unbuilt()):
        with pytest.raises(ValueError, match="template must be"):
            PixLocPoseTrackerR9(template=bad, **kw)
    with pytest.raises(ValueError, match="supersample"):
        mesh_template.MeshTemplate(None, supersample=3)


def test_lock_step_tracking_refuses_a_mesh_template_tracker():
    import torch

    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    tr = object.__new__(PixLocPoseTrackerR9)
    tr.device, tr.reference_points, tr.depth_refine, tr.occlusion, tr.template = torch.device("cpu"), "sfm", None, None, object()
    with pytest.raises(ValueError, match="mesh template"):
        MultiObjectTracker([tr])


def test_parser_defaults_leave_the_command_line_as_it_is():
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import build_parser, template_from_args

    args = build_parser().parse_args(["--object_path", "o", "--query", "q", "--out_dir", "d"])
    assert args.template == "nerf" and args.mesh is None and args.texture is None and args.mesh_scale == 1.0
    assert args.mesh_supersample == 2 and args.reference_sfm is None and args.upright_ref_img is None
    assert template_from_args(args) is None
    args = build_parser().parse_args(["--template", "mesh", "--mesh", "m.ply", "--mesh_supersample", "4", "--reference_sfm", "r",
                                      "--upright_ref_img", "mapping/0001.png", "--mesh_scale", "0.001", "--texture", "t.png"])
    assert (args.template, str(args.mesh), args.mesh_supersample, str(args.reference_sfm), args.upright_ref_img, args.mesh_scale,
            str(args.texture)) == ("mesh", "m.ply", 4, "r", "mapping/0001.png", 0.001, "t.png")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--mesh_supersample", "3"])
    with pytest.raises(ValueError, match="--mesh"):
        template_from_args(build_parser().parse_args(["--template", "mesh"]))
    with pytest.raises(ValueError, match="--template mesh"):
        template_from_args(build_parser().parse_args(["--mesh", "m.ply"]))
