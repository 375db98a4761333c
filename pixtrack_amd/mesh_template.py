"""The tracker's per-frame template from a mesh instead of a NeRF.

Per frame ``PixLocPoseTrackerR9`` asks its renderer for two images at one pose: a ``depth_nz`` plane at the query camera
(``depth_mask_plane`` makes the query mask of it) and an 8-bit image at the reference camera (SfM camera 1 x
``reference_scale``), which the UNet encodes as the frame's reference.  ``MeshTemplate`` draws both from a coloured or
textured mesh in one ``MeshRenderer.render_frame`` call (pxt_mesh_render_frame, four launches): view 0 is the query camera
at one sample per pixel and gives ``depth_nz``; view 1 is the reference camera, anti-aliased by ``supersample`` x
``supersample`` samples per pixel, and gives ``rgb_u8``.  The SfM model ``mesh_dataset`` builds from the same mesh is in the
mesh's own frame, so the tracker's pose goes into the view record as it is: no ``nerf2sfm``, no snapshot.

``supersample`` defaults to 2.  That is an untuned starting value: the NeRF template is rendered with ``spp = 8``, and
which of 1, 2 and 4 tracks best on real sequences has not been measured.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import mesh_render as R
from .geometry import Camera


class MeshTemplate:
    """``renderer``: a ``MeshRenderer`` with vertex colours or a texture map.  ``near``: the near plane of the view
    records (a triangle with a vertex at or behind it is culled whole, as in pxt_mesh_raster)."""

    def __init__(self, renderer: R.MeshRenderer, supersample: int = 2, near: float = 1e-6, render_ahead: bool = False):
        if int(supersample) not in (1, 2, 4):
            raise ValueError(f"supersample is 1, 2 or 4 (got {supersample})")
        if renderer.colors is None and renderer.texture is None:
            raise ValueError("a mesh template needs a MeshRenderer with vertex colours or a texture map")
        self.renderer = renderer
        self.supersample = int(supersample)
        self.near = float(near)
        # opt-in: a tracker queues the next frame's views behind this frame's LM launch (frames_ahead)
        self.render_ahead = bool(render_ahead)
        # the farthest a vertex lies from the mesh frame's origin: bounds a frame's depths, see depth_q
        self.radius = float(np.linalg.norm(renderer.vertices_host.astype(np.float64), axis=1).max())

    @classmethod
    def from_files(cls, mesh, texture=None, mesh_scale: float = 1.0, device="cuda:0", supersample: int = 2,
                   near: float = 1e-6, render_ahead: bool = False) -> "MeshTemplate":
        """A mesh file as ``mesh_dataset`` reads it: vertex colours (``read_mesh_colors``) or, without them, texture
        coordinates and a map (``read_mesh_textured``; ``texture`` names another image for the same UVs)."""
        V, F, C = R.read_mesh_colors(mesh)
        if C is not None:
            if texture:
                raise ValueError(f"{mesh} has vertex colours; a texture goes with a mesh that has texture coordinates")
            return cls(R.MeshRenderer(V * float(mesh_scale), F, device, colors=C), supersample, near, render_ahead)
        textured = R.read_mesh_textured(mesh, require_image=texture is None)
        if textured is None:
            raise ValueError(f"{mesh} has no vertex colours and no texture coordinates")
        V, F, uvs, triangle_uvs, image = textured
        return cls(R.MeshRenderer(V * float(mesh_scale), F, device, uvs=uvs, triangle_uvs=triangle_uvs,
                                  texture=R.read_texture(texture or image)), supersample, near, render_ahead)

    def depth_q(self, pose) -> float:
        """The factor on a frame's depths: 1 / (the origin's distance + the mesh's radius), so that every depth d lies in
        (0, 1] and the ``depth_nz`` rule ``uint8(d * 255) != 0`` never wraps to 0 on a covered pixel farther than 1 / 255
        of that bound."""
        _, t = R._pose_Rt(pose)
        return 1.0 / (float(np.linalg.norm(t)) + self.radius)

    @staticmethod
    def _same_view(a: Camera, b: Camera) -> bool:
        da, db = (c._data.detach().cpu().double().numpy() for c in (a, b))
        return da.ndim == 1 and db.ndim == 1 and np.array_equal(np.rint(da[:2]), np.rint(db[:2])) and np.array_equal(da[2:6], db[2:6])

    def requests(self, pose, query_camera: Camera, reference_camera: Camera, want_depth: bool = False) -> list:
        """The frame's ``render_frame`` requests: one view with both outputs when ``supersample`` is 1 and the two
        cameras agree in size, fx, fy, cx and cy; else the query view (S = 1) and the reference view.  A camera with
        lens terms is refused (``view_record``)."""
        q = self.depth_q(pose)
        size = lambda cam: tuple(int(round(float(x))) for x in cam.size.tolist())
        vq = R.view_record(query_camera, pose, self.near, q)
        vr = R.view_record(reference_camera, pose, self.near, q)
        depth_outputs = ("depth_nz", "depth") if want_depth else ("depth_nz",)
        if self.supersample == 1 and self._same_view(query_camera, reference_camera):
            return [(vq, *size(query_camera), 1, depth_outputs + ("rgb_u8",))]
        return [(vq, *size(query_camera), 1, depth_outputs), (vr, *size(reference_camera), self.supersample, ("rgb_u8",))]

    def requests_ahead(self, query_camera: Camera, reference_camera: Camera, want_depth: bool = False) -> list:
        """The requests of ``requests`` for a frame whose pose is not known on the host yet: the same views, sizes,
        supersample and outputs, each with a pose-free view record - intrinsics and near filled, the pose and
        ``depth_q`` zero (pxt_mesh_render_frame_batch_posed takes those from the LM's output record on the device)."""
        size = lambda cam: tuple(int(round(float(x))) for x in cam.size.tolist())

        def record(cam):
            v = R.view_record(cam, np.eye(4), self.near, 0.0)
            v[:12] = 0.0
            return v

        depth_outputs = ("depth_nz", "depth") if want_depth else ("depth_nz",)
        if self.supersample == 1 and self._same_view(query_camera, reference_camera):
            return [(record(query_camera), *size(query_camera), 1, depth_outputs + ("rgb_u8",))]
        return [(record(query_camera), *size(query_camera), 1, depth_outputs),
                (record(reference_camera), *size(reference_camera), self.supersample, ("rgb_u8",))]

    def frame(self, pose, query_camera: Camera, reference_camera: Camera, want_depth: bool = False, requests=None):
        """-> ``(depth_nz uint8 [Hq, Wq], rgb_u8 uint8 [Hr, Wr, 3])`` device tensors at ``pose`` (world -> camera, a
        ``Pose`` or 4x4), and with ``want_depth`` the query view's float depth image [Hq, Wq, 4] (depths times
        ``depth_q(pose)``) as a third.  One call, four launches, nothing downloaded.  ``requests``: what ``requests``
        returned for these arguments, for a caller that also reads the view records (``requests[0][0]``: the query
        view's 20 floats, which ``mesh_render.points_reference`` / pxt_points_from_depth_views back-project through)."""
        if requests is None:
            requests = self.requests(pose, query_camera, reference_camera, want_depth)
        out = self.renderer.render_frame(requests, download_records=False)
        res = (out[0]["depth_nz"], out[-1]["rgb_u8"])
        return res + (out[0]["depth"],) if want_depth else res

    @staticmethod
    def frames(templates, poses, query_cameras, reference_cameras, workspace=None, scenes=None, r_grow: int = 0,
               records: bool = False, want_depth=None) -> list:
        """``frame`` for several templates - K objects tracked in lock-step - in ONE ``mesh_render.render_frame_batch``
        call: every template's ``requests`` as ``frame`` forms them, one chain of launches, one upload of all views ->
        ``[(depth_nz, rgb_u8)]`` per template, the planes ``frame`` returns bit for bit.  ``workspace``: the calling
        stream's ``mesh_render.FrameBatchWorkspace`` (None: one for this call).

        ``scenes`` (one scene id or None per template; None: exactly the call above): templates that name one id are
        objects in one image.  The scene view is the query view, view 0 of ``requests``; the templates of a scene share
        the query camera.  -> ``[(depth_nz, rgb_u8, occluder or None)]``: ``occluder`` uint8 [Hq, Wq] marks the pixels
        where another template of the scene lies in front of this one, grown by the ``(2 r_grow + 1)^2`` box
        (pxt_mesh_render_scene_batch, one more launch).  ``records``: the query view's record (int32 [16] on the
        device; words 0, 10, 11: covered, hidden, occluder pixels) is appended to every tuple.

        ``want_depth`` (one bool per template; None: exactly the calls above): a template that asks also gets its query
        view's float depth plane, as ``frame(..., want_depth=True)`` returns it.  Every tuple then ends in ``(depth or
        None, view20 or None)``: the plane and the 20 floats of the view record it was drawn with."""
        if want_depth is None:
            reqs = [t.requests(pose, qc, rc) for t, pose, qc, rc in zip(templates, poses, query_cameras, reference_cameras)]
        else:
            reqs = [t.requests(pose, qc, rc, bool(d))
                    for t, pose, qc, rc, d in zip(templates, poses, query_cameras, reference_cameras, want_depth)]
        items = [(t.renderer, q) for t, q in zip(templates, reqs)]
        tail = lambda out, q: () if want_depth is None else ((out[0]["depth"], q[0][0]) if "depth" in q[0][4] else (None, None))
        if scenes is None:
            outs = R.render_frame_batch(items, workspace=workspace, download_records=False)
            return [(out[0]["depth_nz"], out[-1]["rgb_u8"]) + ((out[0]["records"],) if records else ()) + tail(out, q)
                    for out, q in zip(outs, reqs)]
        view_scenes = [[s] + [None] * (len(q) - 1) for s, q in zip(scenes, reqs)]
        outs = R.render_frame_batch(items, workspace=workspace, download_records=False, scenes=view_scenes, r_grow=r_grow)
        return [(out[0]["depth_nz"], out[-1]["rgb_u8"], out[0].get("occluder")) + ((out[0]["records"],) if records else ())
                + tail(out, q) for out, q in zip(outs, reqs)]

    @staticmethod
    def frames_ahead(templates, pose_records, query_cameras, reference_cameras, workspace, views_out, want_depth=None,
                     requests=None) -> list:
        """``frames`` for poses that are still on their way: template k's views take their pose on the device from
        ``pose_records[k]`` - the float32 output record of the LM launch queued ahead on this stream (device or pinned
        host memory) - and ``depth_q`` from that pose and the template's radius (``mesh_render.posed_view_reference``).
        ONE ``mesh_render.render_frame_batch(poses=)`` call (split only by the 16-mesh / 32-view limits); the query and
        the reference view of a template share its record.  ``views_out``: float32 [all views, 24], pinned host or device
        - per view, in request order, the 20 floats it was drawn with and the completion word (1.0: the refinement
        succeeded, -1.0: it did not; stored last): the caller compares them with its own ``view_record`` once it knows the
        pose and keeps the planes only if they are the same bits.  ``requests``: per template what ``requests_ahead``
        returned.  -> ``[(depth_nz, rgb_u8)]``, with ``want_depth`` ``[(depth_nz, rgb_u8, depth or None)]``."""
        want = [False] * len(templates) if want_depth is None else [bool(d) for d in want_depth]
        if requests is None:
            requests = [t.requests_ahead(qc, rc, d) for t, qc, rc, d in zip(templates, query_cameras, reference_cameras, want)]
        items = [(t.renderer, q) for t, q in zip(templates, requests)]
        poses = [[(rec, t.radius)] * len(q) for t, rec, q in zip(templates, pose_records, requests)]
        outs = R.render_frame_batch(items, workspace=workspace, download_records=False, poses=poses, views_out=views_out)
        tail = lambda out, q: () if want_depth is None else (out[0].get("depth"),)
        return [(out[0]["depth_nz"], out[-1]["rgb_u8"]) + tail(out, q) for out, q in zip(outs, requests)]
