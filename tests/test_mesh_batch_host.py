"""pxt_mesh_render_frame_batch's declarations, the ctypes mirror of its descriptor, the tensor-free argument checks of the
op, the lock-step tracker's template check and its command line.  No GPU."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_entry_points_the_constants_and_the_op_are_declared():
    from pixtrack_amd import _lib, ops

    header = (ROOT / "include" / "pixtrack_hip.h").read_text()
    assert _lib.ABI_VERSION == 13 and re.search(r"int pxt_version\(void\);\s*/\* ABI version \(13\)", header)
    for name in ("pxt_mesh_render_frame_batch", "pxt_mesh_render_frame_batch_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    assert re.search(r"#define\s+PXT_MESH_BATCH_MAX_MESHES\s+16\b", header) and _lib.PXT_MESH_BATCH_MAX_MESHES == 16
    assert re.search(r"#define\s+PXT_MESH_BATCH_MAX_VIEWS\s+32\b", header) and _lib.PXT_MESH_BATCH_MAX_VIEWS == 32
    assert "mesh_render_frame_batch" in ops.op_names()
    L, C = _lib.lib(), _lib.C
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)
    size = lambda counts, vm, geo: int(L.pxt_mesh_render_frame_batch_workspace_bytes(len(counts), i32(counts), len(vm), i32(vm), i32(geo)))
    one = size([20], [0], [8, 8, 1])
    assert one > 0 and size([20], [0], [8, 8, 4]) > size([20], [0], [8, 8, 2]) > one
    assert size([20, 1280], [0, 1], [8, 8, 1, 8, 8, 1]) - size([20, 20], [0, 1], [8, 8, 1, 8, 8, 1]) == (1280 - 20) * 16  # a list per view
    assert size([20, 1 << 20], [0, 0], [8, 8, 1, 8, 8, 1]) == size([20, 20], [0, 1], [8, 8, 1, 8, 8, 1])  # an unnamed mesh has none
    assert size([1 << 20], [0], [8, 8, 1]) - one == (16384 - 20) * 16  # the cap
    assert size([20], [0], [8, 8, 3]) == -1 and size([20], [1], [8, 8, 1]) == -1 and size([20] * 17, [0], [8, 8, 1]) == -1
    assert size([20], [0] * 33, [8, 8, 1] * 33) == -1 and size([0], [0], [8, 8, 1]) == -1


def test_the_descriptor_mirror_has_the_header_structs_size(tmp_path):
    from pixtrack_amd import _lib

    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pixtrack_hip.h"\n'
                                  'int main(void) {\n  printf("%zu %zu %zu %zu\\n", sizeof(pxt_mesh_desc), '
                                  'offsetof(pxt_mesh_desc, texture), offsetof(pxt_mesh_desc, n_vertices), '
                                  'offsetof(pxt_mesh_desc, tex_height));\n  return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    D = _lib.MeshDesc
    assert got == [ctypes.sizeof(D), D.texture.offset, D.n_vertices.offset, D.tex_height.offset]


def test_mesh_batch_planes():
    from pixtrack_amd import _lib, ops

    assert ops.mesh_batch_planes([0, 1], 2, [8, 8, 2, 5, 7, 1], [0, -1, -1, -1, -1, 0, -1, 0]) == (2, [8 * 8 * 16, 5 * 7 * 3, 0, 5 * 7])
    assert ops.mesh_batch_planes([1, 1], 16, [8, 8, 1, 8, 8, 1], [0, -1, -1, -1, 8 * 8 * 16, -1, -1, -1])[0] == 2  # meshes no view names
    assert ops.mesh_batch_planes([0] * 32, 1, [4, 4, 1] * 32, [x for p in range(32) for x in (-1, -1, -1, 16 * p)])[0] == 32
    bad = [([0], 0, [8, 8, 1], [0, -1, -1, -1]), ([0], 17, [8, 8, 1], [0, -1, -1, -1]),                   # M = 0, M = 17
           ([0] * 33, 1, [4, 4, 1] * 33, [x for p in range(33) for x in (-1, -1, -1, 16 * p)]),          # P = 33
           ([], 1, [], []),                                                                              # P = 0
           ([1], 1, [8, 8, 1], [0, -1, -1, -1]), ([-1], 1, [8, 8, 1], [0, -1, -1, -1]),                  # view_mesh out of range
           ([0, 0], 1, [8, 8, 1], [0, -1, -1, -1]), ([], 1, [8, 8, 1], [0, -1, -1, -1]),                 # ... of the wrong length
           # every per-view refusal of mesh_frame_planes
           ([0], 1, [8, 8, 3], [0, -1, -1, -1]), ([0], 1, [8, 8, 2], [-1, -1, -1, 0]), ([0], 1, [8, 8, 2], [-1, -1, 0, -1]),
           ([0], 1, [8, 8, 1], [-1, -1, -1, -1]), ([0], 1, [8, 8, 1], [8, -1, -1, -1]), ([0], 1, [8, 8, 1], [-1, 2, -1, -1]),
           ([0], 1, [8, 8, 1], [-1, -1, 8, -1]), ([0], 1, [8, 8, 1], [-1, -1, -1, 2]),
           ([0], 1, [0, 8, 1], [0, -1, -1, -1]), ([0], 1, [8, -1, 1], [0, -1, -1, -1]),
           ([0], 1, [1 << 13, (1 << 11) + 1, 4], [0, -1, -1, -1]),
           ([0, 1], 2, [8, 8, 1, 8, 8, 1], [0, -1, -1, -1, 16, -1, -1, -1]),                             # overlapping planes
           ([0], 1, [8, 8], [0, -1, -1, -1]), ([0], 1, [8, 8, 1], [0, -1, -1])]
    for view_mesh, n_meshes, geometry, offsets in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_batch_planes(view_mesh, n_meshes, geometry, offsets)
    # the one-mesh call keeps its own bound on the views
    with pytest.raises(_lib.PxtError):
        ops.mesh_frame_planes([4, 4, 1] * 9, [x for p in range(9) for x in (-1, -1, -1, 16 * p)])


def stand_in(template):
    import torch

    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    tr = object.__new__(PixLocPoseTrackerR9)
    tr.device, tr.reference_points, tr.depth_refine, tr.occlusion, tr.template = torch.device("cpu"), "sfm", None, None, template
    return tr


def test_lock_step_tracking_takes_a_mesh_template_and_nothing_else():
    from pixtrack_amd.mesh_template import MeshTemplate
    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker

    for bad in (object(), "mesh", 3):
        with pytest.raises(ValueError, match="mesh template.*MeshTemplate"):
            MultiObjectTracker([stand_in(bad)])
    # a MeshTemplate passes the check: the stand-in then fails on the first attribute it lacks, not on its template
    with pytest.raises(Exception) as e:
        MultiObjectTracker([stand_in(object.__new__(MeshTemplate))])
    assert isinstance(e.value, AttributeError) and "mesh template" not in str(e.value), repr(e.value)
    # the other refusals of lock-step tracking stand, a mesh template or not
    for option, word in ((dict(reference_points="render"), "reference_points"), (dict(depth_refine=object()), "depth_refine"),
                         (dict(occlusion=object()), "occlusion")):
        tr = stand_in(object.__new__(MeshTemplate))
        for k, v in option.items():
            setattr(tr, k, v)
        with pytest.raises(ValueError, match=word):
            MultiObjectTracker([tr])


def test_parser_defaults_and_the_mesh_arguments():
    from pixtrack_amd.pose_trackers.multi_object_tracker import _per_object, build_parser

    base = ["--object_path", "a", "b", "--query", "qa", "qb", "--out_dir", "da", "db"]
    args = build_parser().parse_args(base)
    assert args.template == "nerf" and args.mesh is None and args.texture is None and args.mesh_scale == [1.0]
    assert args.mesh_supersample == [2] and args.reference_sfm is None and args.groups == 2 and args.obj_aabb is None
    args = build_parser().parse_args(base + ["--template", "mesh", "--mesh", "a.ply", "b.obj", "--texture", "t.png",
                                             "--mesh_scale", "0.001", "--mesh_supersample", "4", "1", "--reference_sfm", "ra", "rb",
                                             "--upright_ref_img", "mapping/0001.png", "mapping/0002.png"])
    assert args.template == "mesh" and [str(m) for m in args.mesh] == ["a.ply", "b.obj"] and args.mesh_supersample == [4, 1]
    per = lambda values, flag="--x": [_per_object(values, k, 2, flag) for k in range(2)]
    assert [str(m) for m in per(args.mesh)] == ["a.ply", "b.obj"] and [str(t) for t in per(args.texture)] == ["t.png", "t.png"]
    assert per(args.mesh_scale) == [0.001, 0.001] and per(args.mesh_supersample) == [4, 1] and per(None) == [None, None]
    assert [str(r) for r in per(args.reference_sfm)] == ["ra", "rb"]
    with pytest.raises(ValueError, match="--mesh takes one entry per object or one entry for all"):
        _per_object(["a", "b", "c"], 0, 2, "--mesh")
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--mesh_supersample", "3"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--template", "splat"])
