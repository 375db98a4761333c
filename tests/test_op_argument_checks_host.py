"""The argument checks of the op bodies in pixtrack_amd/ops.py, characterised on host tensors.

For every op body the table below holds one well-formed call on small CPU tensors and the mutants of it that the body
refuses.  Two assertions per body:

  * the well-formed call ends in ``Reached`` (the body got as far as its native entry point) or in the device refusal
    ("... must live on a ROCm device"): both mean that every argument check was passed;
  * each mutant raises ``PxtError`` with a message that is not the device refusal.

Nothing here can launch anything, on any machine: ``ops._lib.lib`` returns a proxy of the real library that passes
through only ``pxt_version`` and the pure ``*_workspace_bytes`` size queries (those that take no context handle); every
other entry point raises ``Reached``.  ``ops._stream`` returns 0, and ``Tensor.is_pinned`` says yes for the tensors
under a body's HOST_RECORDS arguments alone, so that a host tensor stands in for a pinned record and the checks behind
the record's are reached; a mutant made with ``unpinned`` leaves a record in plain host memory.

Five bodies test a device before their last argument check - lm_information, lm_point_report and depth_refine their
workspace's ahead of the per-problem checks, mask_exclude and occlusion_mask_views per tensor and per view; their rows
run with ``_lib.require_gpu`` lifted so that the checks behind are reached.  ngp_render_frame_batch words its
workspace's check together with ``is_cuda``: on host tensors its well-formed call ends there, and only the mutants it
refuses before are listed.

Not covered: ``unet_forward_batch`` (its size query needs a live context handle) and ``conv3x3_nhwc_f16`` (no checks).
Checks that a body words together with ``is_cuda`` (the tile guard's flags of lm_refine, the 8-bit planes of
ngp_render_frame[_batch]) cannot be told from the device refusal on host tensors; their mutants are listed where the
message is the body's own.  Rows marked NEW are refusals the shared check vocabulary added; a tensor on
another device than its call's anchor cannot be built from host tensors and has no row.
"""
import pytest
import torch

from pixtrack_amd import _lib, ops

DEVICE_REFUSAL = "must live on a ROCm device"
PURE = {"pxt_version", "pxt_lm_workspace_bytes", "pxt_lm_batch_workspace_bytes", "pxt_lm_information_workspace_bytes",
        "pxt_lm_point_report_workspace_bytes", "pxt_ngp_batch_workspace_bytes", "pxt_points_from_depth_workspace_bytes",
        "pxt_points_from_depth_views_workspace_bytes", "pxt_pose_errors_workspace_bytes",
        "pxt_depth_agreement_workspace_bytes", "pxt_symmetric_pose_errors_workspace_bytes",
        "pxt_sensor_vsd_workspace_bytes", "pxt_depth_refine_workspace_bytes", "pxt_occlusion_mask_workspace_bytes",
        "pxt_occlusion_mask_views_workspace_bytes", "pxt_iso_surface_workspace_bytes",
        "pxt_max_pairwise_distance_workspace_bytes", "pxt_mesh_raster_workspace_bytes",
        "pxt_mesh_render_frame_workspace_bytes", "pxt_mesh_render_frame_batch_workspace_bytes",
        "pxt_mesh_render_scene_batch_workspace_bytes"}


class Reached(Exception):
    """A body passed its checks and called a native entry point."""


class Proxy:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in PURE:
            return getattr(self._real, name)

        def entry(*_args, **_kw):
            raise Reached(name)

        entry.__name__ = name
        return entry


@pytest.fixture
def no_launch(monkeypatch):
    proxy = Proxy(_lib.lib())
    monkeypatch.setattr(ops._lib, "lib", lambda: proxy)
    monkeypatch.setattr(ops, "_stream", lambda t: 0)
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: id(self) in PINNED)


PINNED = set()  # the ids of the host tensors that stand in for pinned memory during one call (see ``call``)
# body -> the arguments that are records the host reads: device memory or pinned host memory
HOST_RECORDS = {
    "lm_refine": ("record", "cam_out"), "lm_refine_batch": ("records", "cam_outs"), "lm_information": ("poses", "records"),
    "lm_point_report": ("poses", "summaries"), "ngp_render_both_from_pose": ("pose_record", "cam_out"),
    "points_from_depth": ("record",), "points_from_depth_views": ("record",), "depth_refine": ("poses", "records", "logs"),
    "occlusion_mask": ("record",), "occlusion_mask_views": ("records",), "mask_exclude": ("record",),
    "points_visible": ("record",), "iso_surface_count": ("counts",), "max_pairwise_distance": ("out",),
    "mesh_render_frame_batch_posed": ("pose_records", "views_out"),
}


def f(*s):
    return torch.zeros(*s, dtype=torch.float32)


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def u16(*s):
    return torch.zeros(*s, dtype=torch.uint16)


def nc(t):
    """The same shape and dtype, not contiguous."""
    return t.new_zeros(*t.shape, 2)[..., 0]


def ws():
    return u8(1 << 22)


def put(key, value):
    return lambda a: a.__setitem__(key, value)


def at(key, i, value):
    def mutate(a):
        a[key] = list(a[key])
        a[key][i] = value(a[key][i]) if callable(value) else value
    return mutate


def unpinned(*keys):
    """The records under ``keys`` are plain host memory: neither device nor pinned."""
    return lambda a: a.__setitem__("unpinned", keys)


def cut(key, n=1):
    return lambda a: a.__setitem__(key, list(a[key])[:-n])


def both(*ms):
    def mutate(a):
        for m in ms:
            m(a)
    return mutate


H, W, N, CS, NI = 4, 6, 5, 8, 3  # planes of 4 x 6, 5 points, records of 8 floats, 3 iterations
NH = 16 + _lib.PXT_MAX_LEVELS
CAM = [float(W), float(H), 5.0, 5.0, 3.0, 2.0, 0.0, 0.0, 0.0, 0.0]
T12 = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 1.0]
LM_CONF = dict(num_iters=NI, pad=1, loss=2, loss_alpha=0.0, loss_scale=0.1, grad_stop=1e-4, dt_stop=5e-3, dR_stop=5e-2,
               min_valid=3, n_workgroups=0)
EVAL_CONF = dict(pad=1, loss=2, loss_alpha=0.0, loss_scale=0.1, min_valid=3)
VIEW = [0.0] * ops.VIEW_FLOATS


def lm_refine():
    return dict(p3d=f(N, 3), point_mask=u8(N), fmaps=[f(H, W, CS), f(H, W, CS)], frefs=[f(N, CS), f(N, CS)],
                channels=[7, 7], cameras=CAM * 2, ndist=[0, 0], lambdas=[0.1] * 12, T_init=T12, **LM_CONF,
                record=f(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE), workspace=ws(), want_log=True)


def lm_refine_batch():
    K = 2
    return dict(p3d=[f(N, 3)] * K, point_masks=[u8(N), None], n_levels=[2, 2], fmaps=[f(H, W, CS)] * 4,
                frefs=[f(N, CS)] * 4, channels=[7] * 4, cameras=CAM * 4, ndist=[0] * 4, lambdas=[0.1] * 24, T_init=T12 * K,
                **LM_CONF, records=[f(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE) for _ in range(K)], workspaces=[ws(), ws()],
                batch_workspace=ws(), want_log=True)


def lm_evaluate(**more):
    K = 2
    return dict(p3d=[f(N, 3)] * K, point_masks=[u8(N), None], fmaps=[f(H, W, CS)] * K, frefs=[f(N, CS)] * K,
                channels=[7] * K, cameras=CAM * K, ndist=[0] * K, poses=[f(12), f(12)], pose_is_lm_record=False,
                **EVAL_CONF, **more, workspace=ws())


def lm_information():
    return lm_evaluate(records=[f(_lib.PXT_LM_INFO_RECORD) for _ in range(2)])


def lm_point_report():
    return lm_evaluate(inlier_weights=[0.5, 0.5], points=[f(N, _lib.PXT_LM_POINT_RECORD), None],
                       summaries=[f(_lib.PXT_LM_REPORT_SUMMARY) for _ in range(2)])


def sample_sparse():
    return dict(p3d=f(N, 3), T=T12, fmaps=[f(H, W, CS), f(H, W, CS)], channels=[7, 7], cameras=CAM * 2, ndist=[0, 0],
                pad=1, normalize=False, outs=[f(N, CS), f(N, CS)], valid=u8(N))


def score_pose_hypotheses():
    return dict(fmap=f(H, W, CS), channels=7, camera=CAM, ndist=0, p3d=f(N, 3), fref=f(N, CS), valid=u8(N), poses=f(2, 12),
                ranges=i32(2, 2), pad=1, loss=2, loss_alpha=0.0, loss_scale=0.1, out=f(2, 4))


def ngp_render():
    return dict(ctx=0, view=VIEW, width=W, height=H, spp=1, mode=0, out=f(H, W, 4), stats=None)


def ngp_render_both():
    return dict(ctx=0, view=VIEW, width=W, height=H, spp=1, rgba=f(H, W, 4), depth=f(H, W, 4), stats=None)


def ngp_render_both_from_pose():
    return dict(ctx=0, view=VIEW, pose_record=f(NH), conv=[0.0] * 27, width=W, height=H, spp=1, mode=0, rgba=f(H, W, 4),
                depth=f(H, W, 4), cam_out=f(16), stats=None)


def ngp_render_frame():
    return dict(ctx=0, view=VIEW, width=W, height=H, spp=1, mode=2, camera_from_slot=False, rgba=f(H, W, 4),
                depth=f(H, W, 4), rgb_u8=None, depth_nz=None, stats=None)


def ngp_render_frame_batch():
    return dict(ctxs=[0, 0], views=VIEW * 2, sizes=[W, H, W, H], spp=1, modes=[0, 1], camera_from_slot=False,
                rgb_u8=[u8(H, W, 3)], depth_nz=[u8(H, W)], workspace=ws(), stats=[])


def depth_mask_plane():
    return dict(depth_nz=u8(H, W), n_erode=1, n_dilate=5, mask=u8(H, W))


def depth_mask():
    return dict(depth_rgba=f(H, W, 4), n_erode=1, n_dilate=5, mask=u8(H, W), scratch=u8(2 * H * W))


def rgba_to_u8():
    return dict(rgba=f(H, W, 4), alpha_thresh=0.5, out=u8(H, W, 3))


def resize_linear():
    return dict(src=f(H, W, 3), dst=f(2, 3, 3))


def resize_activity():
    return dict(mask=u8(H, W), image_u8=None, H=H, W=W, active=u8(2, 3))


def points_from_depth():
    return dict(depth=f(H, W, 4), xform=T12, focal=5.0, depth_scale=1.0, min_alpha=0.5, erode=1, n_max=N, p3d=f(N, 3),
                slot_valid=u8(N), record=i32(4), workspace=ws())


def points_from_depth_views():
    return dict(depth=[f(H, W, 4), f(3, 5, 4)], views=[0.0] * (2 * _lib.PXT_MESH_VIEW), min_alpha=0.5, erode=1, n_max=N,
                p3d=f(2, N, 3), slot_valid=u8(2, N), record=i32(2, 4), workspace=ws())


def pose_errors():
    return dict(vertices=f(N, 3), rel_poses=f(2, 12), want_adds=True, records=f(2, _lib.PXT_POSE_ERR_RECORD), workspace=ws())


def depth_agreement():
    return dict(depth_est=f(2, H, W, 4), depth_gt=f(2, H, W, 4), min_alpha=0.5, tq=[1.0, 2.0],
                records=i32(2, _lib.PXT_DEPTH_AGREE_RECORD), workspace=ws())


def symmetric_pose_errors():
    return dict(vertices=f(N, 3), syms=f(2, 12), frames=f(2, _lib.PXT_SYM_ERR_FRAME),
                records=f(2, _lib.PXT_SYM_ERR_RECORD), workspace=ws())


def sensor_vsd():
    return dict(depth_est=f(2, H, W, 4), depth_gt=f(2, H, W, 4), sensor=u16(2, H, W), ray=f(H, W), shift=[1, -1],
                min_alpha=0.5, sensor_q=1.0, delta_q=1.0, tq=[1.0], records=i32(2, _lib.PXT_SENSOR_VSD_RECORD),
                workspace=ws())


def depth_refine():
    K = 2
    return dict(p3d=[f(N, 3)] * K, point_masks=[u8(N), None], sensors=[u16(H, W)] * K, sensor_scales=[1.0] * K,
                cameras=CAM * K, ndist=[0] * K, poses=[f(12), f(12)], pose_is_lm_record=False, priors=[0.0] * (21 * K),
                num_iters=NI, pad=1, loss=2, loss_alpha=0.0, loss_scale=0.1, lambdas=[0.1] * 6, max_residual=1.0,
                max_edge=1.0, grad_stop=1e-4, dt_stop=5e-3, dR_stop=5e-2, min_valid=3,
                records=[f(_lib.PXT_DEPTH_RECORD) for _ in range(K)], logs=[f(NI, _lib.PXT_DEPTH_LOG_STRIDE), None],
                codes=[u8(NI + 1, N), None], workspace=ws())


def occlusion_mask():
    return dict(depth=f(H, W, 4), sensor=u16(H, W), mask_in=u8(H, W), shift=[1, -1], min_alpha=0.5, sensor_q=1.0,
                delta_q=1.0, radii=[1, 2], mask=u8(H, W), occluder=u8(H, W), record=i32(_lib.PXT_OCCLUSION_RECORD),
                workspace=ws())


def occlusion_mask_views():
    return dict(depth=[f(H, W, 4), f(3, 5, 4)], sensors=[u16(H, W), u16(3, 5)], masks_in=[u8(H, W), u8(3, 5)],
                shifts=[1, -1, 0, 0], min_alpha=0.5, quanta=[1.0] * 4, radii=[1, 2], masks=[u8(H, W), u8(3, 5)],
                occluders=[u8(H, W), u8(3, 5)], records=i32(2, _lib.PXT_OCCLUSION_RECORD), workspace=ws())


def mask_exclude():
    return dict(mask_in=u8(H, W), occluder=u8(H, W), mask=u8(H, W), record=i32(2))


def points_visible():
    return dict(p3d=f(N, 3), valid_in=u8(N), pose=T12, camera=CAM, ndist=0, occluder=u8(H, W), valid=u8(N),
                record=i32(_lib.PXT_OCCLUSION_RECORD))


def ngp_query():
    return dict(ctx=0, pos=f(N, 3), dir=f(N, 3), out=f(N, 4))


GRID = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]


def iso_surface_count():
    return dict(values=f(3, 4, 5), grid=GRID, workspace=ws(), counts=i32(2))


def iso_surface_emit():
    return dict(values=f(3, 4, 5), grid=GRID, workspace=ws(), vertices=f(7, 3), normals=f(7, 3), triangles=i32(4, 3))


def max_pairwise_distance():
    return dict(points=f(N, 3), out=i32(4), workspace=ws())


NV, NT, P = 4, 2, 2  # a mesh of 4 vertices and 2 triangles, 2 views
REC = _lib.PXT_MESH_RASTER_RECORD


def mesh_raster():
    return dict(vertices=f(NV, 3), triangles=i32(NT, 3), views=f(P, _lib.PXT_MESH_VIEW), depth=f(P, H, W, 4),
                triangle_ids=i32(P, H, W), records=i32(P, REC), workspace=ws())


def mesh_outputs():
    return dict(rgba=f(P, H, W, 4), rgb_u8=u8(P, H, W, 3), depth=f(P, H, W, 4), depth_nz=u8(P, H, W),
                triangle_ids=i32(P, H, W), records=i32(P, REC), workspace=ws())


def mesh_render():
    return dict(vertices=f(NV, 3), triangles=i32(NT, 3), colors=f(NV, 3), views=f(P, _lib.PXT_MESH_VIEW), width=W, height=H,
                **mesh_outputs())


def mesh_render_textured():
    return dict(vertices=f(NV, 3), triangles=i32(NT, 3), uvs=f(6, 2), triangle_uvs=i32(NT, 3), texture=u8(3, 5, 4),
                views=f(P, _lib.PXT_MESH_VIEW), width=W, height=H, **mesh_outputs())


PX = H * W
GEOMETRY = [W, H, 1, W, H, 1]
OFFSETS = [0, 0, 0, 0, 16 * PX, 3 * PX, 16 * PX, PX]  # (rgba, rgb_u8, depth, depth_nz) byte offsets per view


def frame_buffers():
    return dict(rgba=f(2 * 4 * PX), rgb_u8=u8(2 * 3 * PX), depth=f(2 * 4 * PX), depth_nz=u8(2 * PX), records=i32(P, REC),
                workspace=ws())


def mesh_render_frame():
    return dict(vertices=f(NV, 3), triangles=i32(NT, 3), colors=f(NV, 3), uvs=None, triangle_uvs=None, texture=None,
                views=f(P, _lib.PXT_MESH_VIEW), geometry=GEOMETRY, offsets=OFFSETS, **frame_buffers())


def mesh_batch(**more):
    """Two meshes, the first coloured and the second textured; view p draws mesh p."""
    a = dict(vertices=[f(NV, 3), f(NV, 3)], triangles=[i32(NT, 3), i32(NT, 3)], colors=[f(NV, 3), None],
             uvs=[None, f(6, 2)], triangle_uvs=[None, i32(NT, 3)], texture=[None, u8(3, 5, 4)], view_mesh=[0, 1],
             views=f(P, _lib.PXT_MESH_VIEW), geometry=GEOMETRY, offsets=OFFSETS)
    a.update(more)
    a.update(frame_buffers())
    return a


def mesh_render_frame_batch():
    return mesh_batch()


def mesh_render_frame_batch_posed():
    a = mesh_batch(pose_records=[f(NH), None], radii=[0.1, 0.1])
    a["views_out"] = f(P, _lib.PXT_MESH_VIEW_OUT)
    return a


def mesh_render_scene_batch():
    a = mesh_batch(view_scene=[0, 0], r_grow=2, occluder_offsets=[0, 24])
    records, workspace = a.pop("records"), a.pop("workspace")
    a.update(occluder=u8(2 * PX), records=records, workspace=workspace)
    return a


dbl = torch.Tensor.double

# the mutants of the per-level / per-problem LM arguments that the three LM bodies share
LM_LEVELS = [
    ("fmap of float64", at("fmaps", 1, dbl)),
    ("fmap not contiguous", at("fmaps", 0, nc)),
    ("fref of float64", at("frefs", 0, dbl)),
    ("fref not contiguous", at("frefs", 1, nc)),
    ("fref of another width", at("frefs", 1, f(N, CS + 4))),
    ("fref of another length", at("frefs", 0, f(N + 1, CS))),
]
SENSOR = [("sensor of float32", f), ("sensor of uint8", u8), ("sensor of int32", i32)]

# body -> (the well-formed call, True: lift the device check / text: where a host call ends at best,
#          [(what is wrong, mutation of the call's arguments)])
TABLE = {
    "lm_refine": (lm_refine, False, LM_LEVELS + [
        ("no level", both(put("fmaps", []), put("frefs", []), put("channels", []), put("cameras", []), put("ndist", []),
                          put("lambdas", []))),
        ("nine levels", both(put("fmaps", [f(H, W, CS)] * 9), put("frefs", [f(N, CS)] * 9), put("channels", [7] * 9),
                             put("cameras", CAM * 9), put("ndist", [0] * 9), put("lambdas", [0.1] * 54))),
        ("a fref short", cut("frefs")), ("a channel count short", cut("channels")), ("cameras short", cut("cameras")),
        ("lambdas short", cut("lambdas")), ("ndist short", cut("ndist")), ("T_init of 11", cut("T_init")),
        ("p3d of float64", put("p3d", f(N, 3).double())), ("p3d not contiguous", put("p3d", nc(f(N, 3)))),
        ("record short", put("record", f(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE - 1))),
        ("record of int32", put("record", i32(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE))),
        ("record not contiguous", put("record", nc(f(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE)))),
        ("point_mask of int32", put("point_mask", i32(N))), ("point_mask not contiguous", put("point_mask", nc(u8(N)))),
        ("cam_conv of 26", both(put("cam_conv", [0.0] * 26), put("cam_slots", [1]))),
        ("three camera slots", both(put("cam_conv", [0.0] * 27), put("cam_slots", [1, 2, 3]))),
        ("a camera with no slot and no cam_out", put("cam_conv", [0.0] * 27)),
        ("cam_out short", both(put("cam_conv", [0.0] * 27), put("cam_out", f(12)))),
        ("cam_out of float64", both(put("cam_conv", [0.0] * 27), put("cam_out", f(16).double()))),
        ("guard flags without geometry", put("guard_flags", u8(64))),
        ("guard geometry of three", both(put("guard_flags", u8(64)), put("guard_geo", [4, 4, 0]))),
        ("record in unpinned host memory", unpinned("record")),
        ("cam_out in unpinned host memory", both(put("cam_conv", [0.0] * 27), put("cam_out", f(16)), unpinned("cam_out"))),
        ("NEW (a): point_mask of another length", put("point_mask", u8(N + 1))),
        ("NEW (c): cam_out not contiguous", both(put("cam_conv", [0.0] * 27), put("cam_out", nc(f(16))))),
    ]),
    "lm_refine_batch": (lm_refine_batch, False, [
        ("fmap of float64", at("fmaps", 3, dbl)), ("fmap not contiguous", at("fmaps", 0, nc)),
        ("fref of float64", at("frefs", 0, dbl)), ("fref not contiguous", at("frefs", 2, nc)),
        ("fref of another width", at("frefs", 3, f(N, CS + 4))), ("fref of another length", at("frefs", 0, f(N + 1, CS))),
        ("no problem", both(put("p3d", []), put("point_masks", []), put("n_levels", []), put("records", []),
                            put("workspaces", []), put("T_init", []))),
        ("seventeen problems", both(put("p3d", [f(N, 3)] * 17), put("point_masks", [None] * 17), put("n_levels", [0] * 17),
                                    put("records", [f(NH)] * 17), put("workspaces", [ws()] * 17), put("T_init", T12 * 17))),
        ("a record short", cut("records")), ("a workspace short", cut("workspaces")), ("a mask slot short", cut("point_masks")),
        ("T_init short", cut("T_init")), ("a fmap short", cut("fmaps")), ("a fref short", cut("frefs")),
        ("a channel count short", cut("channels")), ("cameras short", cut("cameras")), ("lambdas short", cut("lambdas")),
        ("ndist short", cut("ndist")), ("a problem of no level", put("n_levels", [0, 4])),
        ("a problem of nine levels", both(put("n_levels", [9, 2]), put("fmaps", [f(H, W, CS)] * 11),
                                          put("frefs", [f(N, CS)] * 11), put("channels", [7] * 11), put("cameras", CAM * 11),
                                          put("ndist", [0] * 11), put("lambdas", [0.1] * 66))),
        ("p3d of float64", at("p3d", 1, dbl)), ("p3d not contiguous", at("p3d", 0, nc)),
        ("record short", at("records", 1, f(NH + 2 * NI * _lib.PXT_LM_LOG_STRIDE - 1))),
        ("record of float64", at("records", 0, dbl)), ("record not contiguous", at("records", 0, nc)),
        ("point mask of int32", at("point_masks", 0, i32(N))), ("point mask not contiguous", at("point_masks", 0, nc)),
        ("point mask of another length", at("point_masks", 1, u8(N - 1))),
        ("cam_conv of 27 for two", both(put("cam_conv", [0.0] * 27), put("cam_slots", [0] * 4))),
        ("cam_slots of 2 for two", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 2))),
        ("one cam_out for two", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 4), put("cam_outs", [f(16)]))),
        ("cam_out short", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 4), put("cam_outs", [f(16), f(12)]))),
        ("cam_out of int32", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 4), put("cam_outs", [i32(16), f(16)]))),
        ("batch_workspace short", put("batch_workspace", u8(16))),
        ("records in unpinned host memory", unpinned("records")),
        ("cam_outs in unpinned host memory", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 4),
                                                  put("cam_outs", [f(16), f(16)]), unpinned("cam_outs"))),
        ("NEW (c): cam_out not contiguous", both(put("cam_conv", [0.0] * 54), put("cam_slots", [0] * 4),
                                                 put("cam_outs", [f(16), nc(f(16))]))),
    ]),
    "sample_sparse": (sample_sparse, False, [
        ("an out short", cut("outs")), ("cameras short", cut("cameras")), ("T of 11", cut("T")),
        ("windows of 7", put("windows", [0] * 7)), ("p3d of float64", put("p3d", f(N, 3).double())),
        ("p3d not contiguous", put("p3d", nc(f(N, 3)))), ("fmap of float64", at("fmaps", 0, dbl)),
        ("fmap not contiguous", at("fmaps", 1, nc)), ("out of float64", at("outs", 0, dbl)),
        ("out not contiguous", at("outs", 1, nc)), ("out of another width", at("outs", 0, f(N, CS + 4))),
        ("out of another length", at("outs", 1, f(N - 1, CS))), ("valid of int32", put("valid", i32(N))),
        ("valid of another length", put("valid", u8(N + 1))),
    ]),
    "score_pose_hypotheses": (score_pose_hypotheses, False, [
        ("fmap of float64", put("fmap", f(H, W, CS).double())), ("p3d not contiguous", put("p3d", nc(f(N, 3)))),
        ("fref of float64", put("fref", f(N, CS).double())), ("poses not contiguous", put("poses", nc(f(2, 12)))),
        ("out of float64", put("out", f(2, 4).double())), ("fmap of two dimensions", put("fmap", f(H, W))),
        ("camera of 9", cut("camera")), ("p3d of [N, 4]", put("p3d", f(N, 4))), ("fref of another width", put("fref", f(N, 4))),
        ("fref of another length", put("fref", f(N + 1, CS))), ("valid of int32", put("valid", i32(N))),
        ("valid not contiguous", put("valid", nc(u8(N)))), ("valid of another length", put("valid", u8(N + 1))),
        ("poses of one dimension", put("poses", f(24))), ("poses of [M, 11]", put("poses", f(2, 11))),
        ("no pose", both(put("poses", f(0, 12)), put("ranges", i32(0, 2)), put("out", f(0, 4)))),
        ("ranges of int64", put("ranges", i32(2, 2).long())), ("ranges not contiguous", put("ranges", nc(i32(2, 2)))),
        ("ranges of another length", put("ranges", i32(3, 2))), ("out of another length", put("out", f(3, 4))),
    ]),
    "ngp_render": (ngp_render, False, [
        ("out of float64", put("out", f(H, W, 4).double())), ("out not contiguous", put("out", nc(f(H, W, 4)))),
        ("out of another size", put("out", f(W, H, 4))), ("a view of 24 floats", cut("view")),
    ]),
    "ngp_render_both": (ngp_render_both, False, [
        ("rgba of float64", put("rgba", f(H, W, 4).double())), ("depth not contiguous", put("depth", nc(f(H, W, 4)))),
        ("depth of another size", put("depth", f(H, W, 3))), ("a view of 24 floats", cut("view")),
    ]),
    "ngp_render_both_from_pose": (ngp_render_both_from_pose, False, [
        ("rgba of another size", put("rgba", f(H + 1, W, 4))), ("depth of float64", put("depth", f(H, W, 4).double())),
        ("pose_record short", put("pose_record", f(11))), ("pose_record of float64", put("pose_record", f(NH).double())),
        ("cam_out short", put("cam_out", f(12))), ("cam_out of int32", put("cam_out", i32(16))), ("conv of 26", cut("conv")),
        ("pose_record in unpinned host memory", unpinned("pose_record")), ("cam_out in unpinned host memory", unpinned("cam_out")),
        ("a view of 24 floats", cut("view")),
    ]),
    "ngp_render_frame": (ngp_render_frame, False, [
        ("mode 3", put("mode", 3)), ("rgba of another size", put("rgba", f(H, W, 3))),
        ("depth not contiguous", put("depth", nc(f(H, W, 4)))), ("rgb_u8 of float32", put("rgb_u8", f(H, W, 3))),
        ("rgb_u8 of another size", put("rgb_u8", u8(H, W, 4))), ("depth_nz of another size", put("depth_nz", u8(W, H))),
        ("no output", both(put("rgba", None), put("depth", None))), ("a view of 24 floats", cut("view")),
    ]),
    "ngp_render_frame_batch": (ngp_render_frame_batch, "workspace is a contiguous device uint8 tensor", [
        ("no render", both(put("ctxs", []), put("views", []), put("sizes", []), put("modes", []))),
        ("views short", cut("views")), ("sizes short", cut("sizes")), ("modes short", cut("modes")),
        ("mode 3", put("modes", [0, 3])), ("an rgb_u8 too many", put("rgb_u8", [u8(H, W, 3)] * 2)),
        ("no depth_nz", put("depth_nz", [])), ("two depth_float for one", put("depth_float", [f(H, W, 4)] * 2)),
        ("workspace of float32", put("workspace", f(64))),
    ]),
    "depth_mask_plane": (depth_mask_plane, False, [
        ("depth_nz of float32", put("depth_nz", f(H, W))), ("depth_nz of three dimensions", put("depth_nz", u8(H, W, 1))),
        ("depth_nz not contiguous", put("depth_nz", nc(u8(H, W)))), ("mask of float32", put("mask", f(H, W))),
        ("mask of another size", put("mask", u8(W, H))), ("mask not contiguous", put("mask", nc(u8(H, W)))),
        ("mask misaligned", both(put("depth_nz", u8(H, 8)), put("mask", u8(H * 8 + 4)[1:1 + H * 8].view(H, 8)))),
    ]),
    "depth_mask": (depth_mask, False, [
        ("depth_rgba of float64", put("depth_rgba", f(H, W, 4).double())),
        ("depth_rgba not contiguous", put("depth_rgba", nc(f(H, W, 4)))), ("mask of int32", put("mask", i32(H, W))),
        ("mask of another size", put("mask", u8(H, W + 1))), ("mask not contiguous", put("mask", nc(u8(H, W)))),
        ("scratch short", put("scratch", u8(2 * H * W - 1))),
    ]),
    "rgba_to_u8": (rgba_to_u8, False, [
        ("rgba of float64", put("rgba", f(H, W, 4).double())), ("rgba not contiguous", put("rgba", nc(f(H, W, 4)))),
        ("out of float32", put("out", f(H, W, 3))), ("out of another size", put("out", u8(H, W, 4))),
    ]),
    "resize_linear": (resize_linear, False, [
        ("src of float64", put("src", f(H, W, 3).double())), ("dst not contiguous", put("dst", nc(f(2, 3, 3)))),
        ("channel counts differ", put("dst", f(2, 3, 4))),
    ]),
    "resize_activity": (resize_activity, False, [
        ("mask and image", put("image_u8", u8(H, W, 3))), ("neither mask nor image", put("mask", None)),
        ("mask of float32", put("mask", f(H, W))), ("mask not contiguous", put("mask", nc(u8(H, W)))),
        ("active of float32", put("active", f(2, 3))), ("active not contiguous", put("active", nc(u8(2, 3)))),
    ]),
    "points_from_depth": (points_from_depth, False, [
        ("depth of float64", put("depth", f(H, W, 4).double())), ("depth not contiguous", put("depth", nc(f(H, W, 4)))),
        ("p3d of float64", put("p3d", f(N, 3).double())), ("depth of [H, W, 3]", put("depth", f(H, W, 3))),
        ("depth of two dimensions", put("depth", f(H, W))), ("xform of 11", cut("xform")), ("erode 3", put("erode", 3)),
        ("n_max 0", both(put("n_max", 0), put("p3d", f(0, 3)), put("slot_valid", u8(0)))),
        ("p3d of another length", put("p3d", f(N + 1, 3))), ("slot_valid of int32", put("slot_valid", i32(N))),
        ("slot_valid of another length", put("slot_valid", u8(N - 1))), ("slot_valid not contiguous", put("slot_valid", nc(u8(N)))),
        ("record of float32", put("record", f(4))), ("record short", put("record", i32(3))),
        ("record not contiguous", put("record", nc(i32(4)))), ("workspace short", put("workspace", u8(8))),
        ("workspace of float32", put("workspace", f(1 << 16))), ("workspace not contiguous", put("workspace", nc(u8(1 << 16)))),
    ]),
    "points_from_depth_views": (points_from_depth_views, False, [
        ("no plane", put("depth", [])), ("seventeen planes", put("depth", [f(H, W, 4)] * 17)),
        ("a plane of float64", at("depth", 1, dbl)), ("a plane not contiguous", at("depth", 0, nc)),
        ("a plane of [H, W, 3]", at("depth", 1, f(H, W, 3))), ("p3d of float64", put("p3d", f(2, N, 3).double())),
        ("views short", cut("views")), ("erode -1", put("erode", -1)), ("p3d of another shape", put("p3d", f(2 * N, 3))),
        ("slot_valid of another shape", put("slot_valid", u8(2 * N))), ("slot_valid of float32", put("slot_valid", f(2, N))),
        ("record of another shape", put("record", i32(8))), ("record of int64", put("record", i32(2, 4).long())),
        ("record not contiguous", put("record", nc(i32(2, 4)))), ("workspace short", put("workspace", u8(8))),
        ("workspace of int32", put("workspace", i32(1 << 16))),
    ]),
    "pose_errors": (pose_errors, False, [
        ("vertices of float64", put("vertices", f(N, 3).double())), ("rel_poses not contiguous", put("rel_poses", nc(f(2, 12)))),
        ("records of int32", put("records", i32(2, 8))), ("vertices of [V, 4]", put("vertices", f(N, 4))),
        ("rel_poses of one dimension", put("rel_poses", f(24))), ("records of another length", put("records", f(3, 8))),
        ("no vertex", put("vertices", f(0, 3))), ("workspace short", put("workspace", u8(8))),
        ("workspace of float32", put("workspace", f(1 << 16))),
    ]),
    "depth_agreement": (depth_agreement, False, [
        ("depth_est of float64", put("depth_est", f(2, H, W, 4).double())),
        ("depth_gt not contiguous", put("depth_gt", nc(f(2, H, W, 4)))), ("depth_est of three dimensions", put("depth_est", f(H, W, 4))),
        ("depth_gt of another shape", put("depth_gt", f(2, W, H, 4))), ("no threshold", put("tq", [])),
        ("seventeen thresholds", put("tq", [1.0] * 17)), ("records of float32", put("records", f(2, 24))),
        ("records of another shape", put("records", i32(2, 32))), ("records not contiguous", put("records", nc(i32(2, 24)))),
        ("no pixel", both(put("depth_est", f(2, 0, W, 4)), put("depth_gt", f(2, 0, W, 4)))),
        ("workspace short", put("workspace", u8(8))), ("workspace not contiguous", put("workspace", nc(u8(1 << 16)))),
    ]),
    "symmetric_pose_errors": (symmetric_pose_errors, False, [
        ("vertices not contiguous", put("vertices", nc(f(N, 3)))), ("syms of float64", put("syms", f(2, 12).double())),
        ("frames of float64", put("frames", f(2, 40).double())), ("records of int32", put("records", i32(2, 8))),
        ("syms of [S, 16]", put("syms", f(2, 16))), ("frames of [F, 12]", put("frames", f(2, 12))),
        ("records of another length", put("records", f(1, 8))), ("no symmetry", put("syms", f(0, 12))),
        ("workspace short", put("workspace", u8(8))), ("workspace of int32", put("workspace", i32(1 << 16))),
    ]),
    "sensor_vsd": (sensor_vsd, False, [
        ("depth_est of float64", put("depth_est", f(2, H, W, 4).double())), ("depth_gt of another shape", put("depth_gt", f(1, H, W, 4))),
        *[(what, put("sensor", make(2, H, W))) for what, make in SENSOR],
        ("sensor of another shape", put("sensor", u16(H, W))), ("sensor not contiguous", put("sensor", nc(u16(2, H, W)))),
        ("ray of float64", put("ray", f(H, W).double())), ("ray of another shape", put("ray", f(W, H))),
        ("shift of one", put("shift", [1])), ("shift out of range", put("shift", [32768, 0])), ("no threshold", put("tq", [])),
        ("records of another shape", put("records", i32(2, 24))), ("records of float32", put("records", f(2, 32))),
        ("workspace short", put("workspace", u8(8))), ("workspace of float32", put("workspace", f(1 << 16))),
    ]),
    "depth_refine": (depth_refine, True, [
        ("no problem", put("p3d", [])), ("seventeen problems", put("p3d", [f(N, 3)] * 17)),
        ("a sensor short", cut("sensors")), ("a scale short", cut("sensor_scales")), ("a record short", cut("records")),
        ("a log slot short", cut("logs")), ("a codes slot short", cut("codes")), ("cameras short", cut("cameras")),
        ("priors short", cut("priors")), ("lambdas of 5", cut("lambdas")), ("num_iters 33", put("num_iters", 33)),
        ("num_iters -1", put("num_iters", -1)), ("p3d of float64", at("p3d", 0, dbl)), ("p3d of [N, 4]", at("p3d", 1, f(N, 4))),
        ("no point", at("p3d", 1, f(0, 3))), ("too many points", at("p3d", 1, f(4097, 3))),
        ("point mask of another length", at("point_masks", 0, u8(N + 1))), ("point mask of int32", at("point_masks", 0, i32(N))),
        *[(what, at("sensors", 1, make(H, W))) for what, make in SENSOR],
        ("sensor of three dimensions", at("sensors", 0, u16(1, H, W))), ("sensor of three rows", at("sensors", 0, u16(3, W))),
        ("sensor not contiguous", at("sensors", 0, nc(u16(H, W)))), ("log of another shape", at("logs", 0, f(NI + 1, 20))),
        ("log of float64", at("logs", 0, dbl)), ("codes of another shape", at("codes", 0, u8(NI, N))),
        ("codes of int32", at("codes", 0, i32(NI + 1, N))), ("pose short", at("poses", 0, f(11))),
        ("pose of float64", at("poses", 1, dbl)), ("record short", at("records", 1, f(31))),
        ("record not contiguous", at("records", 0, nc)), ("workspace short", put("workspace", u8(8))),
        ("poses in unpinned host memory", unpinned("poses")), ("records in unpinned host memory", unpinned("records")),
        ("logs in unpinned host memory", unpinned("logs")),
    ]),
    "occlusion_mask": (occlusion_mask, False, [
        ("depth of float64", put("depth", f(H, W, 4).double())), ("depth of [H, W, 3]", put("depth", f(H, W, 3))),
        *[(what, put("sensor", make(H, W))) for what, make in SENSOR],
        ("sensor of another shape", put("sensor", u16(W, H))), ("sensor not contiguous", put("sensor", nc(u16(H, W)))),
        ("mask_in of float32", put("mask_in", f(H, W))), ("mask_in of another shape", put("mask_in", u8(H, W + 2))),
        ("mask of another shape", put("mask", u8(W, H))), ("occluder not contiguous", put("occluder", nc(u8(H, W)))),
        ("mask is occluder", lambda a: a.__setitem__("mask", a["occluder"])), ("shift of three", put("shift", [0, 0, 0])),
        ("shift out of range", put("shift", [0, -32768])), ("radii of one", put("radii", [1])),
        ("a negative radius", put("radii", [-1, 2])), ("radii too large", put("radii", [9, 8])),
        ("record short", put("record", i32(15))), ("record of float32", put("record", f(16))),
        ("record not contiguous", put("record", nc(i32(16)))), ("workspace short", put("workspace", u8(8))),
        ("workspace of float32", put("workspace", f(1 << 16))), ("record in unpinned host memory", unpinned("record")),
    ]),
    "occlusion_mask_views": (occlusion_mask_views, True, [
        ("no view", put("depth", [])), ("seventeen views", put("depth", [f(H, W, 4)] * 17)), ("a sensor short", cut("sensors")),
        ("an occluder short", cut("occluders")), ("shifts short", cut("shifts")), ("quanta short", cut("quanta")),
        ("radii too large", put("radii", [16, 1])), ("a negative radius", put("radii", [0, -1])),
        ("a shift out of range", put("shifts", [0, 0, 0, 40000])), ("a plane of float64", at("depth", 0, dbl)),
        ("a plane of [H, W, 3]", at("depth", 1, f(3, 5, 3))),
        *[(what, at("sensors", 0, make(H, W))) for what, make in SENSOR],
        ("a sensor of another shape", at("sensors", 1, u16(H, W))), ("a mask_in of float32", at("masks_in", 0, f(H, W))),
        ("a mask of another shape", at("masks", 1, u8(H, W))), ("an occluder not contiguous", at("occluders", 0, nc)),
        ("two views write one plane", lambda a: a.__setitem__("occluders", [a["masks"][0], a["occluders"][1]])),
        ("records of another shape", put("records", i32(32))), ("records of float32", put("records", f(2, 16))),
        ("workspace short", put("workspace", u8(8))), ("records in unpinned host memory", unpinned("records")),
    ]),
    "mask_exclude": (mask_exclude, True, [
        ("mask_in of float32", put("mask_in", f(H, W))), ("mask_in of three dimensions", put("mask_in", u8(H, W, 1))),
        ("mask_in not contiguous", put("mask_in", nc(u8(H, W)))), ("occluder of another shape", put("occluder", u8(W, H))),
        ("occluder of int32", put("occluder", i32(H, W))), ("mask not contiguous", put("mask", nc(u8(H, W)))),
        ("record short", put("record", i32(1))), ("record of float32", put("record", f(2))),
        ("record in unpinned host memory", unpinned("record")),
    ]),
    "points_visible": (points_visible, False, [
        ("p3d of float64", put("p3d", f(N, 3).double())), ("p3d of [N, 4]", put("p3d", f(N, 4))),
        ("occluder of float32", put("occluder", f(H, W))), ("occluder of three dimensions", put("occluder", u8(1, H, W))),
        ("pose of 11", cut("pose")), ("camera of 9", cut("camera")), ("camera of another size", put("camera", [8.0] + CAM[1:])),
        ("valid_in of another length", put("valid_in", u8(N + 1))), ("valid of int32", put("valid", i32(N))),
        ("valid not contiguous", put("valid", nc(u8(N)))), ("record short", put("record", i32(15))),
        ("record of float32", put("record", f(16))), ("record in unpinned host memory", unpinned("record")),
    ]),
    "ngp_query": (ngp_query, False, [
        ("pos of float64", put("pos", f(N, 3).double())), ("dir not contiguous", put("dir", nc(f(N, 3)))),
        ("out of float64", put("out", f(N, 4).double())), ("dir of another length", put("dir", f(N + 1, 3))),
        ("out of [n, 3]", put("out", f(N, 3))), ("no point", both(put("pos", f(0, 3)), put("dir", f(0, 3)), put("out", f(0, 4)))),
    ]),
    "iso_surface_count": (iso_surface_count, False, [
        ("values of float64", put("values", f(3, 4, 5).double())), ("values not contiguous", put("values", nc(f(3, 4, 5)))),
        ("values of two dimensions", put("values", f(4, 5))), ("grid of 6", cut("grid")), ("an empty lattice", put("values", f(3, 0, 5))),
        ("workspace short", put("workspace", u8(8))), ("workspace of float32", put("workspace", f(1 << 16))),
    ]),
    "iso_surface_emit": (iso_surface_emit, False, [
        ("values of float64", put("values", f(3, 4, 5).double())), ("grid of 8", put("grid", GRID + [0.0])),
        ("workspace short", put("workspace", u8(8))),
    ]),
    "max_pairwise_distance": (max_pairwise_distance, False, [
        ("points of float64", put("points", f(N, 3).double())), ("points not contiguous", put("points", nc(f(N, 3)))),
        ("points of [n, 2]", put("points", f(N, 2))), ("no point", put("points", f(0, 3))), ("workspace short", put("workspace", u8(8))),
        ("workspace of int32", put("workspace", i32(1 << 16))), ("out short", put("out", i32(3))), ("out of float32", put("out", f(4))),
        ("out not contiguous", put("out", nc(i32(4)))), ("out in unpinned host memory", unpinned("out")),
    ]),
}

# what mesh_raster, mesh_render and mesh_render_textured refuse alike
MESH_COMMON = [
    ("vertices of float64", put("vertices", f(NV, 3).double())), ("views not contiguous", put("views", nc(f(P, 20)))),
    ("vertices of [V, 2]", put("vertices", f(NV, 2))), ("triangles of int64", put("triangles", i32(NT, 3).long())),
    ("triangles of [T, 4]", put("triangles", i32(NT, 4))), ("triangles not contiguous", put("triangles", nc(i32(NT, 3)))),
    ("views of [P, 16]", put("views", f(P, 16))), ("triangle_ids of int64", put("triangle_ids", i32(P, H, W).long())),
    ("triangle_ids of another shape", put("triangle_ids", i32(P, W, H))), ("records of float32", put("records", f(P, REC))),
    ("records of another shape", put("records", i32(P + 1, REC))), ("records not contiguous", put("records", nc(i32(P, REC)))),
    ("no triangle", put("triangles", i32(0, 3))), ("workspace short", put("workspace", u8(8))),
    ("workspace of float32", put("workspace", f(1 << 16))), ("workspace not contiguous", put("workspace", nc(u8(1 << 16)))),
]
MESH_OUTPUTS = [
    ("rgba of float64", put("rgba", f(P, H, W, 4).double())), ("rgb_u8 of another shape", put("rgb_u8", u8(P, H, W, 4))),
    ("depth not contiguous", put("depth", nc(f(P, H, W, 4)))), ("depth_nz of float32", put("depth_nz", f(P, H, W))),
    ("no output", both(*[put(k, None) for k in ("rgba", "rgb_u8", "depth", "depth_nz", "triangle_ids")])),
    ("no pixel", put("width", 0)),
]
TEXTURED = [
    ("uvs of float64", put("uvs", f(6, 2).double())), ("uvs of [n, 3]", put("uvs", f(6, 3))), ("no uv", put("uvs", f(0, 2))),
    ("triangle_uvs of int64", put("triangle_uvs", i32(NT, 3).long())), ("triangle_uvs of another length", put("triangle_uvs", i32(NT + 1, 3))),
    ("texture of float32", put("texture", f(3, 5, 4))), ("texture of three channels", put("texture", u8(3, 5, 3))),
    ("texture not contiguous", put("texture", nc(u8(3, 5, 4)))), ("an empty texture", put("texture", u8(0, 5, 4))),
]
# what the frame ops refuse alike: planes in flat buffers
FRAME = [
    ("geometry of 5", cut("geometry")), ("offsets of 7", cut("offsets")), ("supersample 3", put("geometry", [W, H, 3, W, H, 1])),
    ("a view of no pixel", put("geometry", [0, H, 1, W, H, 1])), ("a view of no output", put("offsets", [-1] * 4 + OFFSETS[4:])),
    ("depth of a supersampled view", put("geometry", [W, H, 2, W, H, 1])),
    ("an offset not aligned", put("offsets", [0, 0, 0, 0, 16 * PX, 3 * PX + 1, 16 * PX, PX])),
    ("two planes overlap", put("offsets", [0, 0, 0, 0, 16 * PX, 3 * PX, 16 * PX, PX - 4])),
    ("rgba of float64", put("rgba", f(2 * 4 * PX).double())), ("rgba short", put("rgba", f(2 * 4 * PX - 1))),
    ("rgb_u8 of float32", put("rgb_u8", f(2 * 3 * PX))), ("depth missing", put("depth", None)),
    ("depth_nz short", put("depth_nz", u8(PX))), ("depth_nz not contiguous", put("depth_nz", nc(u8(2 * PX)))),
    ("records of float32", put("records", f(P, REC))), ("records of another shape", put("records", i32(P * REC))),
    ("workspace short", put("workspace", u8(8))), ("workspace of float32", put("workspace", f(1 << 16))),
]
BATCH = FRAME + [
    ("a triangles entry short", cut("triangles")), ("a texture entry short", cut("texture")),
    ("seventeen meshes", both(*[put(k, [None] * 17) for k in ("vertices", "triangles", "colors", "uvs", "triangle_uvs", "texture")])),
    ("view_mesh of one", cut("view_mesh")), ("a view of mesh 2", put("view_mesh", [0, 2])),
    ("a view of mesh -1", put("view_mesh", [-1, 1])), ("views of float64", put("views", f(P, 20).double())),
    ("views of another shape", put("views", f(P, 24))), ("views not contiguous", put("views", nc(f(P, 20)))),
    ("vertices of float64", at("vertices", 0, dbl)), ("vertices of [V, 4]", at("vertices", 1, f(NV, 4))),
    ("triangles of int64", at("triangles", 1, torch.Tensor.long)), ("triangles not contiguous", at("triangles", 0, nc)),
    ("no vertex", both(at("vertices", 0, f(0, 3)), at("colors", 0, f(0, 3)))), ("no triangle", at("triangles", 0, i32(0, 3))),
    ("colors and texture", at("colors", 1, f(NV, 3))), ("neither colors nor texture", at("colors", 0, None)),
    ("colors of another length", at("colors", 0, f(NV + 1, 3))), ("colors of float64", at("colors", 0, dbl)),
    ("a textured mesh without uvs", at("uvs", 1, None)), ("uvs of [n, 3]", at("uvs", 1, f(6, 3))),
    ("triangle_uvs of another length", at("triangle_uvs", 1, i32(NT + 1, 3))), ("texture of float32", at("texture", 1, f(3, 5, 4))),
    ("texture of three channels", at("texture", 1, u8(3, 5, 3))),
]
TABLE.update({
    "mesh_raster": (mesh_raster, False, MESH_COMMON + [
        ("depth of float64", put("depth", f(P, H, W, 4).double())), ("depth of another length", put("depth", f(P + 1, H, W, 4))),
        ("depth of three channels", put("depth", f(P, H, W, 3))), ("no pixel", put("depth", f(P, 0, W, 4))),
    ]),
    "mesh_render": (mesh_render, False, MESH_COMMON + MESH_OUTPUTS + [
        ("colors of float64", put("colors", f(NV, 3).double())), ("colors of another length", put("colors", f(NV - 1, 3))),
    ]),
    "mesh_render_textured": (mesh_render_textured, False, MESH_COMMON + MESH_OUTPUTS + TEXTURED),
    "mesh_render_frame": (mesh_render_frame, False, FRAME + [
        ("vertices not contiguous", put("vertices", nc(f(NV, 3)))), ("triangles of [T, 2]", put("triangles", i32(NT, 2))),
        ("views of [P, 16]", put("views", f(P, 16))), ("three views for two", put("views", f(P + 1, 20))),
        ("colors and uvs", put("uvs", f(6, 2))), ("neither colors nor texture", put("colors", None)),
        ("colors of another length", put("colors", f(NV + 1, 3))),
        ("a textured mesh without texture", both(put("colors", None), put("uvs", f(6, 2)), put("triangle_uvs", i32(NT, 3)))),
        ("no triangle", put("triangles", i32(0, 3))),
    ]),
    "mesh_render_frame_batch": (mesh_render_frame_batch, False, BATCH),
    "mesh_render_frame_batch_posed": (mesh_render_frame_batch_posed, False, BATCH),
    "mesh_render_scene_batch": (mesh_render_scene_batch, False, BATCH + [
        ("view_scene of one", cut("view_scene")), ("occluder_offsets of one", cut("occluder_offsets")),
        ("r_grow 9", put("r_grow", 9)), ("r_grow -1", put("r_grow", -1)), ("a scene id out of range", put("view_scene", [0, 2])),
        ("an occluder plane in no scene", put("view_scene", [0, -1])),
        ("an occluder offset not aligned", put("occluder_offsets", [0, 26])),
        ("two occluder planes overlap", put("occluder_offsets", [0, 20])),
        ("a scene of two sizes", put("geometry", [W, H, 1, W + 2, H, 1])),
        ("a scene of two cameras", lambda a: a["views"].__setitem__((1, 12), 2.0)),
        ("occluder of float32", put("occluder", f(2 * PX))), ("occluder short", put("occluder", u8(2 * PX - 1))),
        ("occluder missing", put("occluder", None)),
    ]),
})
EVALUATE = [
    ("no problem", put("p3d", [])), ("sixty-five problems", put("p3d", [f(N, 3)] * 65)), ("a mask slot short", cut("point_masks")),
    ("a fmap short", cut("fmaps")), ("a fref short", cut("frefs")), ("a channel count short", cut("channels")),
    ("ndist short", cut("ndist")), ("a pose short", cut("poses")), ("cameras short", cut("cameras")),
    ("p3d of float64", at("p3d", 0, dbl)), ("p3d not contiguous", at("p3d", 1, nc)), ("p3d of [N, 4]", at("p3d", 0, f(N, 4))),
    ("fmap of float64", at("fmaps", 1, dbl)), ("fmap of two dimensions", at("fmaps", 0, f(H, W))),
    ("fref not contiguous", at("frefs", 0, nc)), ("fref of another width", at("frefs", 1, f(N, CS + 4))),
    ("fref of another length", at("frefs", 0, f(N - 1, CS))), ("point mask of int32", at("point_masks", 0, i32(N))),
    ("point mask not contiguous", at("point_masks", 0, nc)), ("point mask of another length", at("point_masks", 1, u8(N + 1))),
    ("pose short", at("poses", 0, f(11))), ("pose of float64", at("poses", 1, dbl)), ("pose not contiguous", at("poses", 0, nc)),
    ("a 12-float pose for an LM record", put("pose_is_lm_record", True)), ("workspace short", put("workspace", u8(8))),
    ("poses in unpinned host memory", unpinned("poses")),
]
TABLE.update({
    "lm_information": (lm_information, True, EVALUATE + [
        ("a record short", cut("records")), ("record short", at("records", 0, f(47))), ("record of float64", at("records", 1, dbl)),
        ("record not contiguous", at("records", 1, nc)), ("records in unpinned host memory", unpinned("records")),
    ]),
    "lm_point_report": (lm_point_report, True, EVALUATE + [
        ("a summary short", cut("summaries")), ("an inlier weight short", cut("inlier_weights")), ("a points slot short", cut("points")),
        ("summary short", at("summaries", 1, f(15))), ("summary of int32", at("summaries", 0, i32(16))),
        ("points of another length", at("points", 0, f(N + 1, 8))), ("points of [N, 4]", at("points", 0, f(N, 4))),
        ("points of float64", at("points", 0, dbl)), ("points not contiguous", at("points", 0, nc)),
        ("summaries in unpinned host memory", unpinned("summaries")),
    ]),
})


def call(body, args):
    """Calls the body with the tensors under its HOST_RECORDS keys - whatever a mutant put there - standing in for
    pinned memory, but for the keys a mutant names with ``unpinned``."""
    plain = args.pop("unpinned", ())
    PINNED.clear()
    for key in HOST_RECORDS.get(body, ()):
        held = args.get(key)
        if key not in plain:
            PINNED.update(id(t) for t in (held if isinstance(held, (list, tuple)) else [held]) if torch.is_tensor(t))
    return getattr(ops, "_" + body)(**args)


@pytest.mark.parametrize("body", sorted(TABLE))
def test_the_well_formed_call_passes_every_check_and_each_mutant_is_refused(no_launch, monkeypatch, body):
    make, how, mutants = TABLE[body]
    ends = how if isinstance(how, str) else DEVICE_REFUSAL
    if how is True:
        monkeypatch.setattr(ops._lib, "require_gpu", lambda t, name: None)
    try:
        call(body, make())
        pytest.fail(f"{body}: the well-formed call returned without reaching its entry point")
    except Reached:
        pass
    except _lib.PxtError as e:
        assert ends in str(e), f"{body}: the well-formed call was refused: {e}"
    assert len({what for what, _ in mutants}) == len(mutants), f"{body}: two mutants of one name"
    for what, mutate in mutants:
        args = make()
        mutate(args)
        try:
            call(body, args)
        except _lib.PxtError as e:
            assert DEVICE_REFUSAL not in str(e), f"{body}: {what}: met the device refusal first: {e}"
        except Reached as e:
            pytest.fail(f"{body}: {what}: passed every check and reached {e}")
        else:
            pytest.fail(f"{body}: {what}: returned")


def test_every_op_body_has_a_row():
    assert set(ops.op_names()) - set(TABLE) == {"unet_forward_batch", "conv3x3_nhwc_f16"}
