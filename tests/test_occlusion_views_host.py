"""The host side of the sensor options for mesh templates: the wrapper of pxt_occlusion_mask_views and the
library's own argument checks (which return before anything is launched or dereferenced, so they run without a GPU),
the scale rule of a mesh template's depth plane, the lifted and the standing refusals, and the exports."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import _lib, ops
from pixtrack_amd import occlusion as OC

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------ the exports
def test_the_library_exports_the_views_call():
    L = _lib.lib()
    assert not L._pxt_missing
    for name in ("pxt_occlusion_mask_views", "pxt_occlusion_mask_views_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    # an added entry point and an added struct keep the ABI version (include/pixtrack_hip.h, pxt_version)
    assert L.pxt_version() == _lib.ABI_VERSION == 13
    header = (ROOT / "include" / "pixtrack_hip.h").read_text()
    assert "#define PXT_OCCLUSION_MAX_VIEWS 16" in header and "int pxt_occlusion_mask_views(" in header
    assert re.search(r"typedef struct pxt_occlusion_view \{", header)
    assert _lib.PXT_OCCLUSION_MAX_VIEWS == OC.MAX_VIEWS == 16 and "occlusion_mask_views" in ops.op_names()
    assert C.sizeof(_lib.OcclusionView) == 64  # five pointers, four ints, two floats: the header's struct


def test_workspace_bytes():
    L = _lib.lib()
    size = lambda *s: int(L.pxt_occlusion_mask_views_workspace_bytes(len(s) // 2, (C.c_int32 * len(s))(*s)))
    single = lambda w, h: int(L.pxt_occlusion_mask_workspace_bytes(w, h))
    assert size(64, 16) == 32 == single(64, 16) and size(65, 17) == 4 * 32 == single(65, 17)
    assert size(1, 1, 161, 119, 1025, 2) == single(1, 1) + single(161, 119) + single(1025, 2)
    assert size(*([640, 480] * 16)) == 16 * single(640, 480)
    assert size(*([4, 4] * 17)) < 0 and size(0, 4) < 0 and size(4, 4, 4, -1) < 0 and size(1 << 15, 1 << 14) < 0
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(0, (C.c_int32 * 2)(4, 4))) < 0
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(1, None)) < 0


def test_the_library_refuses_bad_tables_before_any_launch():
    """Every PXT_E_ARG case returns before a pointer is followed: made-up, well-aligned addresses serve."""
    L = _lib.lib()
    base = 1 << 40

    def table(n=2, **edit):
        arr = (_lib.OcclusionView * max(n, 1))()
        for k in range(min(n, 2)):
            a, at = arr[k], base + k * (1 << 24)
            a.depth, a.sensor, a.mask_in, a.mask_out, a.occluder = at, at + (1 << 20), at + (2 << 20), at + (3 << 20), at + (4 << 20)
            a.width, a.height, a.shift_x, a.shift_y, a.sensor_q, a.delta_q = 65, 33, 0, 0, 0.25, 0.25
        for name, (k, value) in edit.items():
            setattr(arr[k], name, value)
        return arr

    rec, ws = base + (100 << 20), base + (101 << 20)
    call = lambda arr, n=2, ro=1, rg=3, rec=rec, ws=ws: L.pxt_occlusion_mask_views(arr, n, 0.5, ro, rg, rec, ws, None)
    v0 = table()[0]
    bad = [call(table(), n=0), call(table(), n=17), call(None), call(table(), rec=None), call(table(), ws=None),
           call(table(), ro=9, rg=8), call(table(), ro=-1), call(table(), rg=17), call(table(), rec=rec + 2),
           call(table(), ws=ws + 8)]
    bad += [call(table(**{name: (1, None)})) for name in ("depth", "sensor", "mask_in", "mask_out", "occluder")]
    bad += [call(table(width=(0, 0))), call(table(height=(1, -3))), call(table(width=(0, 1 << 15), height=(0, 1 << 14))),
            call(table(depth=(1, v0.depth + 8))), call(table(sensor=(0, v0.sensor + 1))),
            call(table(shift_x=(0, 40000))), call(table(shift_y=(1, -32768))),
            call(table(occluder=(0, v0.mask_out))),                 # one plane for both outputs
            call(table(mask_out=(1, v0.occluder + 100))),           # into another view's output
            call(table(occluder=(1, v0.mask_in))),                  # over another view's input
            call(table(occluder=(0, v0.mask_in))),                  # the occluder over the view's own mask_in
            call(table(mask_out=(0, v0.mask_in + 1))),              # mask_out may BE mask_in, not straddle it
            call(table(mask_out=(1, v0.sensor))), call(table(occluder=(1, v0.depth + 16))),
            call(table(mask_out=(0, rec))), call(table(occluder=(1, ws + 32))), call(table(), rec=ws)]
    assert all(code == -1 for code in bad), bad  # PXT_E_ARG


def test_the_wrapper_checks_its_arguments():
    import torch

    d = [torch.zeros(4, 6, 4), torch.zeros(3, 5, 4)]
    s = [torch.zeros(4, 6, dtype=torch.int16), torch.zeros(3, 5, dtype=torch.int16)]
    m = [torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(3, 5, dtype=torch.uint8)]
    sh, q = [(0, 0), (1, -1)], [(0.25, 0.25)] * 2
    for args in ((d, s, m, sh, 0.5, q, 9, 8), (d, s, m, sh, 0.5, q, -1, 0), (d, s, m, sh, 0.5, q, 1.5, 0),
                 ([], [], [], [], 0.5, [], 1, 3), (d * 9, s * 9, m * 9, sh * 9, 0.5, q * 9, 1, 3),
                 (d, s[:1], m, sh, 0.5, q, 1, 3), (d, s, m, sh[:1], 0.5, q, 1, 3), (d, s, m, sh, 0.5, q[:1], 1, 3),
                 (d, s, m, [(0, 0), (1,)], 0.5, q, 1, 3), (d, s, m, sh, 0.5, [(0.25, 0.25), (0.25,)], 1, 3),
                 ([d[0], torch.zeros(3, 5, 3)], s, m, sh, 0.5, q, 1, 3)):
        with pytest.raises(ValueError):
            OC.occlusion_mask_views(*args)
    with pytest.raises(ValueError):
        OC.occlusion_mask_views(d, s, m, sh, 0.5, q, 1, 3, masks=m[:1])


# ------------------------------------------------------------------------------------------- the mesh plane's scale
def test_mesh_quanta_follow_the_view_record():
    view = np.zeros(20, np.float32)
    view[17] = np.float32(0.37)
    dq = float(np.float32(0.37))  # the float32 word, taken to float64
    delta, s = 0.0125, 1.7e-4
    want = (float(np.float32(s / (1.0 / dq))), float(np.float32(delta / (1.0 / dq))))
    assert OC.mesh_quanta(delta, s, view) == want == OC.quantize(delta, s, 1.0 / dq)
    assert want != OC.quantize(delta, s, 1.0 / 0.37) or np.float32(s * 0.37) == np.float32(s * dq)  # (not the decimal 0.37)
    import torch

    assert OC.mesh_quanta(delta, s, torch.from_numpy(view)) == want
    for bad in (0.0, -1.0, np.inf, np.nan):
        view[17] = bad
        with pytest.raises(ValueError):
            OC.mesh_quanta(delta, s, view)
    with pytest.raises(ValueError):
        OC.mesh_quanta(delta, s, np.zeros(12, np.float32))


def test_the_rule_on_a_scaled_plane_is_the_rule_in_sfm_units():
    """A 9 x 7 plane of a mesh frame call (depths times depth_q = 0.37): the restatement, given the plane and the quanta
    of the mesh rule, flags exactly the pixels a float64 statement in SfM units flags.  Depths, sensor distances and the
    tolerance are quarter-integers whose differences from the tolerance are 0.25 or more, so that the rounding of the
    scaled float32 values (relative 1e-7) decides no comparison."""
    Wp, Hp, depth_q = 9, 7, np.float32(0.37)
    rng = np.random.default_rng(5)
    z = rng.integers(8, 40, size=(Hp, Wp)) * 0.25             # the mesh's depths in SfM units: 2 .. 9.75
    covered = rng.random((Hp, Wp)) < 0.8
    scale, delta = 0.25, 1.125                                 # SfM units per count; never equal to a z - d_s
    raw = rng.integers(0, 40, size=(Hp, Wp)).astype(np.uint16)
    raw[rng.random((Hp, Wp)) < 0.15] = 0
    raw[2:5, 3:7] = 4                                          # a solid occluder at distance 1
    covered[2:5, 3:7] = True
    d = (z.astype(np.float32) * depth_q).astype(np.float32)
    plane = np.zeros((Hp, Wp, 4), np.float32)
    plane[covered] = np.stack([d, d, d, np.ones_like(d)], -1)[covered]
    view = np.zeros(20, np.float32)
    view[17] = depth_q
    sensor_q, delta_q = OC.mesh_quanta(delta, scale, view)
    mask = np.ones((Hp, Wp), np.uint8)
    for min_alpha in (0.01, 0.5, 1.0):  # any value in (0, 1] selects the covered pixels
        ref = OC.occlusion_mask_reference(plane, raw, mask, (0, 0), min_alpha, sensor_q, delta_q, 0, 0)
        want = covered & (raw != 0) & (z - raw.astype(np.float64) * scale > delta)
        assert np.array_equal(ref["sil"], covered)
        assert np.array_equal(ref["occluded"], want) and want[2:5, 3:7].all() and 12 <= want.sum() < covered.sum()
        assert np.abs((z - raw * scale) - delta)[covered & (raw != 0)].min() >= 0.125
    opened = OC.occlusion_mask_reference(plane, raw, mask, (0, 0), 0.5, sensor_q, delta_q, 1, 1)
    assert opened["opened"][3, 4:6].all() and opened["occluder"][2:5, 3:7].all()


# --------------------------------------------------------------------------------------------------- the refusals
def _mesh_template():
    from pixtrack_amd.mesh_template import MeshTemplate

    return object.__new__(MeshTemplate)  # (no attribute of the template is read by the check)


def test_template_points_lift_the_refusals():
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9 as T

    t = _mesh_template()
    assert T._check_template(t, None, "template", object(), None) is t
    assert T._check_template(t, None, "template", None, object()) is t
    assert T._check_template(t, None, "template", object(), object()) is t
    assert T._check_template(t, "off", "template", object(), object()) is t


def test_sfm_points_keep_them_and_say_what_to_pass():
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9 as T

    t = _mesh_template()
    with pytest.raises(ValueError, match="mesh template is not combined with occlusion unless reference_points='template'"):
        T._check_template(t, None, "sfm", None, object())
    with pytest.raises(ValueError, match="mesh template is not combined with depth_refine unless reference_points='template'"):
        T._check_template(t, None, "sfm", object(), None)
    with pytest.raises(ValueError, match="reference_points='render'"):
        T._check_template(t, None, "render", object(), None)
    with pytest.raises(ValueError, match="relocalizer"):
        T._check_template(t, "views", "template", object(), None)
    with pytest.raises(ValueError, match="needs template=MeshTemplate"):
        T._check_template(None, None, "template", object(), None)


def test_lock_step_takes_the_options_with_template_points_only():
    import torch

    from pixtrack_amd.pose_trackers.multi_object_tracker import MultiObjectTracker
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9

    def stand_in(points, **options):
        tr = object.__new__(PixLocPoseTrackerR9)
        tr.device, tr.reference_points, tr.depth_refine, tr.occlusion = torch.device("cpu"), points, None, None
        tr.template = _mesh_template()
        for k, v in options.items():
            setattr(tr, k, v)
        return tr

    for name in ("depth_refine", "occlusion"):
        with pytest.raises(ValueError, match=f"{name}.*reference_points='template'"):
            MultiObjectTracker([stand_in("sfm", **{name: object()})])
        # with "template" points the option passes: the stand-in then fails on the first attribute it lacks
        with pytest.raises(AttributeError):
            MultiObjectTracker([stand_in("template", **{name: object()})])
    multi = object.__new__(MultiObjectTracker)
    assert "sensor's plane already contains the other objects" in " ".join(MultiObjectTracker.__init__.__doc__.split())
    assert not hasattr(multi, "occlusion_view_calls")  # (set by __init__, beside points_calls and mesh_prime_calls)
