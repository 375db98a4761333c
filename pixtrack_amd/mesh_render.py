"""Depth and colour renders of a triangle mesh: the GPU rasteriser (pxt_mesh_raster, pxt_mesh_render;
csrc/pxt_raster.hip), its numpy restatement and the readers that feed it.

The reference draws meshes with pytorch3d (``pixtrack/utils/pytorch3d_render_utils.py:55-93``, ``render_image``;
``scripts/create_sfm_from_obj.py``; the YCB ground-truth notebook).  Here the renders serve the evaluation stack: BOP's
VSD compares depth renders of the model's mesh at the estimated and the ground-truth pose through the camera's real
intrinsics (``mesh_evaluation.py``), and the mesh ``mesh.py`` extracts can be held against the NeRF it came from.

``rasterize_reference`` restates the rule of ``include/pixtrack_hip.h`` in numpy float32 / int64 arithmetic; the kernel
is held to it bit for bit on the depth image, the triangle ids and the records.  There is no CPU product path: the
restatement draws a few thousand triangles per second and exists for the tests.

Colour (``MeshRenderer.render``, ``shade_reference``): the vertex colours of the winning triangle, interpolated
perspective-correctly, no lighting term and a black background - the reference's ambient-lit ``render_image`` as
``scripts/create_sfm_from_obj.py`` uses it - written as the float image and as the 8-bit planes the tracker takes from
the NeRF renderer (``rgb_u8``, ``depth_nz``).  ``mesh_dataset.py`` builds a reference model from such renders.

Texture (``MeshRenderer(V, F, device, uvs=, triangle_uvs=, texture=)``, ``shade_textured_reference``,
pxt_mesh_render_textured): the same call with the colour read from one texture map through per-corner UVs, by
pytorch3d's ``TexturesUV`` defaults as the reference's ``load_objs_as_meshes`` + ``render_image`` use them - row 0 of the
map is v = 1, corners aligned, bilinear, the border clamped.  ``read_mesh_textured`` reads YCB's ``textured.obj`` with its
``.mtl`` and BOP's ``texture_u`` / ``texture_v`` PLYs.

A frame's views (``MeshRenderer.render_frame``, ``supersampled_view``, ``frame_reference``, pxt_mesh_render_frame): up to
eight views of the mesh in one call, each with its own size, its own outputs and ``supersample`` x ``supersample``
samples per pixel, box-filtered in a fixed order - the tracker's ``depth_nz`` plane and its anti-aliased reference image
from one call (``mesh_template.py``).

Several meshes' frames in one call (``render_frame_batch``, ``frame_batch_reference``, pxt_mesh_render_frame_batch), and
with ``scenes=`` the objects of one image hiding each other (``scene_reference``, pxt_mesh_render_scene_batch): per view
of a scene the pixels where another member has the smaller z bits in the call's own key planes, grown by a box.

Views whose pose is still on its way (``render_frame_batch(poses=)``, ``posed_view_reference``,
pxt_mesh_render_frame_batch_posed): the batch call with one small launch ahead of it that forms the views' records on the
device from the output record of an LM launch queued before it - render-ahead for mesh templates.
"""
from __future__ import annotations

import struct
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .geometry import Camera, Pose

VIEW = _lib.PXT_MESH_VIEW
RECORD = _lib.PXT_MESH_RASTER_RECORD
SUB = 256  # sub-pixel steps per pixel
GUARD = float(1 << 23)
# record words
W_COVERED, W_DRAWN, W_NEAR, W_GUARD, W_ZERO, W_INDEX, W_OFF, W_ZMIN, W_ZMAX, W_STATUS = range(10)
W_HIDDEN, W_OCCLUDER = 10, 11  # pxt_mesh_render_scene_batch's
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# view records
# ---------------------------------------------------------------------------------------------------------------------
def _pose_Rt(T) -> Tuple[np.ndarray, np.ndarray]:
    if isinstance(T, Pose):
        R, t = T.R, T.t
        return R.detach().cpu().double().numpy().reshape(3, 3), t.detach().cpu().double().numpy().reshape(3)
    M = T.detach().cpu().double().numpy() if torch.is_tensor(T) else np.asarray(T, np.float64)
    if M.shape != (4, 4):
        raise ValueError(f"a pose is a Pose or a 4x4 matrix (got {M.shape})")
    return M[:3, :3].copy(), M[:3, 3].copy()


def pack_view(R, t, fx, fy, cx, cy, near, depth_q) -> np.ndarray:
    """The 20 floats of one view, formed in float64 and rounded once."""
    v = np.zeros(VIEW, np.float64)
    v[:9] = np.asarray(R, np.float64).reshape(9)
    v[9:12] = np.asarray(t, np.float64).reshape(3)
    v[12:18] = [fx, fy, cx, cy, near, depth_q]
    return v.astype(np.float32)


def view_record(camera: Camera, T, near: float = 1e-6, depth_q: float = 1.0) -> np.ndarray:
    """A project ``Camera`` (pixel centres at integer coordinates) and a world-to-camera pose (``Pose`` or 4x4) -> the
    20 floats.  A camera with lens terms is refused: the rasteriser is a pinhole."""
    d = camera._data.detach().cpu().double().numpy()
    if d.ndim != 1:
        raise ValueError("view_record takes one camera")
    if d.shape[0] > 6 and np.any(d[6:] != 0.0):
        raise ValueError(f"the mesh rasteriser is a pinhole; this camera has lens terms {d[6:].tolist()}")
    R, t = _pose_Rt(T)
    return pack_view(R, t, d[2], d[3], d[4], d[5], near, depth_q)


def ngp_view_record(cam_to_world, focal: float, width: int, height: int, near: float = 1e-6,
                    depth_q: float = 1.0) -> np.ndarray:
    """The same for the NeRF renderer's own pixel rule: ``cam_to_world`` is the renderer's 3x4 camera (ngp coordinates;
    a ray through pixel ``(i, j)`` has the camera-frame direction ``((i + 0.5 - W/2) / focal, (j + 0.5 - H/2) / focal,
    1)``), so ``fy = fx = focal`` and the principal point is ``(W/2 - 0.5, H/2 - 0.5)`` in the Camera convention.  A mesh
    in the ``ngp`` frame then lands on the pixels a Depth render of the same camera writes; ``depth_q`` = the model's
    depth scale makes the values comparable."""
    C = np.asarray(cam_to_world.detach().cpu().double().numpy() if torch.is_tensor(cam_to_world) else cam_to_world,
                   np.float64).reshape(3, 4)
    R = C[:, :3].T
    t = -R @ C[:, 3]
    return pack_view(R, t, focal, focal, width / 2.0 - 0.5, height / 2.0 - 0.5, near, depth_q)


# ---------------------------------------------------------------------------------------------------------------------
# the rule in numpy
# ---------------------------------------------------------------------------------------------------------------------
def _evaluate(x, y, iz, area, px, py):
    """Coverage and depth of pixels ``(px, py)`` (sub-pixel units, int64) for triangles given as ``x, y`` [3] int64
    arrays, ``iz`` [3] float32 arrays and ``area`` (all broadcastable against the pixels).  -> inside, valid, z bits."""
    e, ins = [], True
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = x[b] - x[a], y[b] - y[a]
        ek = dx * (py - y[a]) - dy * (px - x[a])
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        ins = ins & ((ek > 0) | ((ek == 0) & top_left))
        e.append(ek)
    with np.errstate(all="ignore"):
        A = np.asarray(area).astype(_F)
        l0, l1, l2 = (np.asarray(ek).astype(_F) / A for ek in e)
        inv = (l0 * iz[0] + l1 * iz[1]).astype(_F) + (l2 * iz[2]).astype(_F)
        z = (_F(1.0) / inv.astype(_F)).astype(_F)
        valid = ins & (z > 0) & np.isfinite(z)
    return ins, valid, np.ascontiguousarray(np.broadcast_to(z, np.broadcast(ins, z).shape)).view(np.uint32)


def _project_vertices(V, view):
    """The per-vertex part of the rule for a finite view -> near, guard, X, Y (int64, 0 where not fine), iz."""
    R, t = view[:9].reshape(3, 3), view[9:12]
    fx, fy, cx, cy, near = view[12], view[13], view[14], view[15], view[16]
    with np.errstate(all="ignore"):
        p = np.stack([(((R[k, 0] * V[:, 0] + R[k, 1] * V[:, 1]).astype(_F) + R[k, 2] * V[:, 2]).astype(_F) + t[k]).astype(_F)
                      for k in range(3)], 1)
        p_ok = np.isfinite(p).all(1)
        is_near = p_ok & (p[:, 2] <= near)
        x = (fx * (p[:, 0] / p[:, 2]).astype(_F)).astype(_F) + cx
        y = (fy * (p[:, 1] / p[:, 2]).astype(_F)).astype(_F) + cy
        xs, ys = np.rint((x * _F(SUB)).astype(_F)), np.rint((y * _F(SUB)).astype(_F))
        in_guard = (np.abs(xs) < GUARD) & (np.abs(ys) < GUARD)  # False for a NaN
        is_guard = ~p_ok | (~is_near & ~in_guard)
        fine = ~is_guard & ~is_near
        X = np.where(fine, xs, 0).astype(np.int64)
        Y = np.where(fine, ys, 0).astype(np.int64)
        iz = (_F(1.0) / p[:, 2]).astype(_F)
    return is_near, is_guard, X, Y, iz


def _raster_view(V, F, view, W, H, want_cov):
    key = np.full(H * W, _EMPTY, np.uint64)
    cov = np.zeros(H * W, np.int32) if want_cov else None
    rec = np.zeros(RECORD, np.uint32)
    rec[W_ZMIN] = 0xFFFFFFFF
    if not np.all(np.isfinite(view)):
        rec[W_STATUS] = 0xFFFFFFFF
        return key, cov, rec
    nV = len(V)
    is_near, is_guard, X, Y, iz = _project_vertices(V, view)
    idx_ok = ((F >= 0) & (F < nV)).all(1)
    Fc = np.clip(F, 0, nV - 1)
    guard = idx_ok & is_guard[Fc].any(1)
    nearc = idx_ok & ~guard & is_near[Fc].any(1)
    live = idx_ok & ~guard & ~nearc
    x3 = [X[Fc[:, k]] for k in range(3)]
    y3 = [Y[Fc[:, k]] for k in range(3)]
    z3 = [iz[Fc[:, k]] for k in range(3)]
    area = (x3[1] - x3[0]) * (y3[2] - y3[0]) - (y3[1] - y3[0]) * (x3[2] - x3[0])
    zero = live & (area == 0)
    live = live & ~zero
    flip = area < 0
    for a3 in (x3, y3, z3):
        a3[1], a3[2] = np.where(flip, a3[2], a3[1]), np.where(flip, a3[1], a3[2])
    area = np.abs(area)
    lo_x, hi_x = np.minimum(np.minimum(x3[0], x3[1]), x3[2]), np.maximum(np.maximum(x3[0], x3[1]), x3[2])
    lo_y, hi_y = np.minimum(np.minimum(y3[0], y3[1]), y3[2]), np.maximum(np.maximum(y3[0], y3[1]), y3[2])
    off = live & ((hi_x < 0) | (hi_y < 0) | (lo_x > SUB * (W - 1)) | (lo_y > SUB * (H - 1)))
    live = live & ~off
    rec[W_INDEX], rec[W_GUARD], rec[W_NEAR] = (~idx_ok).sum(), guard.sum(), nearc.sum()
    rec[W_ZERO], rec[W_OFF], rec[W_DRAWN] = zero.sum(), off.sum(), live.sum()
    ix0, ix1 = np.maximum(0, (lo_x + SUB - 1) >> 8), np.minimum(W - 1, hi_x >> 8)
    iy0, iy1 = np.maximum(0, (lo_y + SUB - 1) >> 8), np.minimum(H - 1, hi_y >> 8)
    bw, bh = ix1 - ix0 + 1, iy1 - iy0 + 1
    boxed = live & (bw > 0) & (bh > 0)

    def offer(pix, ins, valid, zbits, tri):
        if want_cov:
            np.add.at(cov, pix[ins], 1)
        k = (zbits.astype(np.uint64) << np.uint64(32)) | np.broadcast_to(tri, zbits.shape).astype(np.uint64)
        np.minimum.at(key, pix[valid], k[valid])

    # the small boxes together, one box offset at a time; the others one triangle at a time
    small = np.nonzero(boxed & (bw <= 8) & (bh <= 8))[0]
    if len(small):
        sx, sy, sz = [a[small] for a in x3], [a[small] for a in y3], [a[small] for a in z3]
        for oy in range(int(bh[small].max())):
            for ox in range(int(bw[small].max())):
                i, j = ix0[small] + ox, iy0[small] + oy
                inside_box = (ox < bw[small]) & (oy < bh[small])
                ins, valid, zb = _evaluate(sx, sy, sz, area[small], i * SUB, j * SUB)
                offer(np.where(inside_box, j * W + i, 0), ins & inside_box, valid & inside_box, zb, small)
    for ti in np.nonzero(boxed & ~((bw <= 8) & (bh <= 8)))[0]:
        i, j = np.meshgrid(np.arange(ix0[ti], ix1[ti] + 1), np.arange(iy0[ti], iy1[ti] + 1))
        ins, valid, zb = _evaluate([a[ti] for a in x3], [a[ti] for a in y3], [a[ti] for a in z3], area[ti], i * SUB, j * SUB)
        offer((j * W + i).ravel(), ins.ravel(), valid.ravel(), zb.ravel(), np.int64(ti))
    covered = key != _EMPTY
    if covered.any():
        zb = (key[covered] >> np.uint64(32)).astype(np.uint32)
        rec[W_COVERED], rec[W_ZMIN], rec[W_ZMAX] = covered.sum(), zb.min(), zb.max()
    return key, cov, rec


def rasterize_reference(V, F, views, width: int, height: int, coverage: bool = False):
    """The rule of pxt_mesh_raster in numpy.  ``V`` [n, 3], ``F`` [m, 3], ``views`` [P, 20] float32 ->
    ``(depth [P, H, W, 4] float32, triangle ids [P, H, W] int32, records [P, 16] uint32)``, and with ``coverage`` also the
    number of triangles that cover each pixel (before the depth test; int32 [P, H, W])."""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    F = np.asarray(F).reshape(-1, 3).astype(np.int64)
    views = np.asarray(views, np.float32).reshape(-1, VIEW)
    P, W, H = len(views), int(width), int(height)
    depth = np.zeros((P, H, W, 4), np.float32)
    ids = np.full((P, H, W), -1, np.int32)
    recs = np.zeros((P, RECORD), np.uint32)
    cov = np.zeros((P, H, W), np.int32) if coverage else None
    for p in range(P):
        key, c, recs[p] = _raster_view(V, F, views[p], W, H, coverage)
        covered = (key != _EMPTY).reshape(H, W)
        z = (key >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(H, W)
        with np.errstate(all="ignore"):
            d = (z * views[p, 17]).astype(np.float32)
        depth[p, ..., :3] = np.where(covered, d, np.float32(0))[..., None]
        depth[p, ..., 3] = covered
        ids[p] = np.where(covered, (key & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(H, W), -1)
        if coverage:
            cov[p] = c.reshape(H, W)
    return (depth, ids, recs, cov) if coverage else (depth, ids, recs)


def _shade_setup(V, F, view, ids, W):
    """What the two colour rules share for the covered pixels of one view, all at once: ``ids`` [H * W] -> (pixels,
    their triangles, exchanged [n] bool, the corners' vertex indices after the exchange [3][n], w [3][n] float32, inv
    [n] float32)."""
    pix = np.nonzero(ids >= 0)[0]
    _, _, X, Y, iz = _project_vertices(V, view)
    tri = ids[pix]
    idx = F[tri]
    idx = [idx[:, 0], idx[:, 1], idx[:, 2]]
    x3, y3, z3 = [X[i] for i in idx], [Y[i] for i in idx], [iz[i] for i in idx]
    area = (x3[1] - x3[0]) * (y3[2] - y3[0]) - (y3[1] - y3[0]) * (x3[2] - x3[0])
    flip = area < 0
    for a3 in (x3, y3, z3, idx):  # the corner attributes follow the exchange through their indices
        a3[1], a3[2] = np.where(flip, a3[2], a3[1]), np.where(flip, a3[1], a3[2])
    px, py = (pix % W) * SUB, (pix // W) * SUB
    with np.errstate(all="ignore"):
        A = np.abs(area).astype(_F)
        w = []
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            e = (x3[b] - x3[a]) * (py - y3[a]) - (y3[b] - y3[a]) * (px - x3[a])
            w.append(((e.astype(_F) / A).astype(_F) * z3[k]).astype(_F))
        inv = ((w[0] + w[1]).astype(_F) + w[2]).astype(_F)
    return pix, tri, flip, idx, w, inv


def _interpolate(w, inv, c):
    """``((w_0 c_0 + w_1 c_1) + w_2 c_2) / inv`` per column of the corner attributes ``c`` [3][n, m], float32."""
    num = ((w[0][:, None] * c[0]).astype(_F) + (w[1][:, None] * c[1]).astype(_F)).astype(_F) + (w[2][:, None] * c[2]).astype(_F)
    return (num.astype(_F) / inv[:, None]).astype(_F)


def _shade_view(V, F, C, view, ids, W):
    """The colour rule for the covered pixels of one view, all at once: ``ids`` [H * W] -> (pixels, rgb [n, 3] float32)."""
    if not (ids >= 0).any():
        return np.zeros(0, np.int64), np.zeros((0, 3), _F)
    pix, _, _, idx, w, inv = _shade_setup(V, F, view, ids, W)
    with np.errstate(all="ignore"):
        rgb = np.fmin(np.fmax(_interpolate(w, inv, [C[i] for i in idx]), _F(0)), _F(1))  # a NaN -> 0
    return pix, rgb.astype(_F)


def _texel_coordinate(x, n):
    """The clamp and split of one texture axis: x [m] float32 in texels, ``n`` texels -> (i0, i1 int64, the weight of i1)."""
    x = np.fmin(np.fmax(x, _F(0)), _F(n - 1))  # a NaN -> 0
    x0 = np.floor(x).astype(_F)
    i0 = x0.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), (x - x0).astype(_F)


def _shade_view_textured(V, F, UV, FUV, tex, view, ids, W):
    """The texture rule for the covered pixels of one view: ``tex`` [Ht, Wt, 3] uint8 -> (pixels, rgb [n, 3] float32)."""
    if not (ids >= 0).any():
        return np.zeros(0, np.int64), np.zeros((0, 3), _F)
    pix, tri, flip, _, w, inv = _shade_setup(V, F, view, ids, W)
    Ht, Wt = tex.shape[:2]
    k = FUV[tri]
    k = [k[:, 0], np.where(flip, k[:, 2], k[:, 1]), np.where(flip, k[:, 1], k[:, 2])]
    ok = np.all([(ki >= 0) & (ki < len(UV)) for ki in k], 0)
    with np.errstate(all="ignore"):
        uv = _interpolate(w, inv, [UV[np.clip(ki, 0, len(UV) - 1)] for ki in k])
        i0, i1, ax = _texel_coordinate((uv[:, 0] * _F(Wt - 1)).astype(_F), Wt)
        j0, j1, ay = _texel_coordinate(((_F(1.0) - uv[:, 1]).astype(_F) * _F(Ht - 1)).astype(_F), Ht)
        tau = lambda j, i: (tex[j, i].astype(_F) / _F(255.0)).astype(_F)
        t00, t01, t10, t11 = tau(j0, i0), tau(j0, i1), tau(j1, i0), tau(j1, i1)
        ax, ay = ax[:, None], ay[:, None]
        top = (t00 + (ax * (t01 - t00).astype(_F)).astype(_F)).astype(_F)
        bot = (t10 + (ax * (t11 - t10).astype(_F)).astype(_F)).astype(_F)
        c = (top + (ay * (bot - top).astype(_F)).astype(_F)).astype(_F)
        rgb = np.fmin(np.fmax(c, _F(0)), _F(1))
    return pix, np.where(ok[:, None], rgb, _F(0)).astype(_F)


def _u8(x):
    """``(long long)(x * 255.0f) & 255`` on float32 values."""
    with np.errstate(all="ignore"):
        return ((np.asarray(x, _F) * _F(255.0)).astype(_F).astype(np.int64) & 255).astype(np.uint8)


def _shade_all(V, F, views, width, height, shade_view):
    """``rasterize_reference`` plus ``shade_view(view, ids [H * W], W) -> (pixels, rgb)`` per view -> the six outputs."""
    views = np.asarray(views, np.float32).reshape(-1, VIEW)
    P, W, H = len(views), int(width), int(height)
    depth, ids, recs = rasterize_reference(V, F, views, W, H)
    rgba = np.zeros((P, H, W, 4), np.float32)
    for p in range(P):
        pix, rgb = shade_view(views[p], ids[p].reshape(-1), W)
        plane = rgba[p].reshape(-1, 4)
        plane[pix, :3] = rgb
        plane[pix, 3] = 1.0
    return rgba, _u8(rgba[..., :3]), depth, (_u8(depth[..., 0]) != 0).astype(np.uint8), ids, recs


def shade_reference(V, F, C, views, width: int, height: int):
    """The rule of pxt_mesh_render in numpy, on ``rasterize_reference``'s depth and ids.  ``C`` [n, 3] float32 vertex
    colours -> ``(rgba [P, H, W, 4] float32, rgb_u8 [P, H, W, 3] uint8, depth [P, H, W, 4] float32, depth_nz [P, H, W]
    uint8, triangle ids [P, H, W] int32, records [P, 16] uint32)``."""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    F = np.asarray(F).reshape(-1, 3).astype(np.int64)
    C = np.ascontiguousarray(np.asarray(C, np.float32).reshape(-1, 3))
    if len(C) != len(V):
        raise ValueError(f"{len(C)} colours for {len(V)} vertices")
    return _shade_all(V, F, views, width, height, lambda view, ids, W: _shade_view(V, F, C, view, ids, W))


def texture_rgb(texture) -> np.ndarray:
    """A texture map as uint8 [Ht, Wt, 3]: a uint8 [Ht, Wt, 3 or 4] array, the fourth byte dropped."""
    tex = np.asarray(texture)
    if tex.dtype != np.uint8 or tex.ndim != 3 or tex.shape[2] not in (3, 4) or not (1 <= tex.shape[0] <= 16384) \
            or not (1 <= tex.shape[1] <= 16384):
        raise ValueError(f"texture is {tex.shape} {tex.dtype}, expected uint8 [1..16384, 1..16384, 3 or 4]")
    return np.ascontiguousarray(tex[..., :3])


def shade_textured_reference(V, F, UV, FUV, texture, views, width: int, height: int):
    """The rule of pxt_mesh_render_textured in numpy, on ``rasterize_reference``'s depth and ids.  ``UV`` [n, 2] float32,
    ``FUV`` [m, 3] (corner k of triangle t uses ``UV[FUV[t, k]]``), ``texture`` uint8 [Ht, Wt, 3 or 4] (row 0 is v = 1)
    -> the six outputs of ``shade_reference``."""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    F = np.asarray(F).reshape(-1, 3).astype(np.int64)
    UV = np.ascontiguousarray(np.asarray(UV, np.float32).reshape(-1, 2))
    FUV = np.asarray(FUV).reshape(-1, 3).astype(np.int64)
    tex = texture_rgb(texture)
    if len(FUV) != len(F) or len(UV) < 1:
        raise ValueError(f"{len(FUV)} UV triangles for {len(F)} triangles, {len(UV)} UVs")
    return _shade_all(V, F, views, width, height,
                      lambda view, ids, W: _shade_view_textured(V, F, UV, FUV, tex, view, ids, W))


# ---------------------------------------------------------------------------------------------------------------------
# a frame's views: per-view sizes and supersampling (pxt_mesh_render_frame)
# ---------------------------------------------------------------------------------------------------------------------
FRAME_OUTPUTS = ("rgba", "rgb_u8", "depth", "depth_nz")
FRAME_MAX_VIEWS = _lib.PXT_MESH_FRAME_MAX_VIEWS


def supersampled_view(view20, S: int) -> np.ndarray:
    """The fine view of pxt_mesh_render_frame: the 20 floats of a view and ``S`` in {1, 2, 4} -> the 20 floats of the
    ``S W x S H`` view whose pixel ``(S i + a, S j + b)`` is the sample of pixel ``(i, j)`` at offset ``((a + 0.5) / S -
    0.5, (b + 0.5) / S - 0.5)``; each step one float32 operation."""
    if int(S) not in (1, 2, 4):
        raise ValueError(f"supersample is 1, 2 or 4 (got {S})")
    v = np.array(np.asarray(view20, np.float32).reshape(VIEW), np.float32)
    s, h = _F(int(S)), _F(0.5) * _F(int(S) - 1)
    with np.errstate(all="ignore"):
        v[12] = v[12] * s
        v[13] = v[13] * s
        v[14] = (v[14] * s).astype(_F) + h
        v[15] = (v[15] * s).astype(_F) + h
    return v


def _frame_request(request):
    view, W, H, S, want = request
    W, H, S, want = int(W), int(H), int(S), tuple(want)
    if S not in (1, 2, 4):
        raise ValueError(f"supersample is 1, 2 or 4 (got {S})")
    if W < 1 or H < 1 or W * S * H * S > 1 << 26:
        raise ValueError(f"{W} x {H} at supersample {S} is not supported (1..2^26 fine pixels)")
    if not want or any(w not in FRAME_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want names outputs of {FRAME_OUTPUTS} (got {want})")
    if S > 1 and ("depth" in want or "depth_nz" in want):
        raise ValueError(f"depth and depth_nz exist for supersample 1 alone (got {S})")
    return np.asarray(view, np.float32).reshape(VIEW), W, H, S, want


def box_sum(fine: np.ndarray, S: int) -> np.ndarray:
    """``fine`` [S H, S W, C] float32 -> [H, W, C]: the S x S blocks summed in row-major order from the first sample on,
    one float32 add each, then times ``1 / S^2``."""
    acc = None
    for b in range(S):
        for a in range(S):
            c = fine[b::S, a::S]
            acc = c.astype(_F) if acc is None else (acc + c).astype(_F)
    return (acc * _F(1.0 / (S * S))).astype(_F)


def frame_reference(V, F, shading: dict, requests) -> list:
    """The rule of pxt_mesh_render_frame in numpy: ``shade_reference`` (``shading = {"colors": C}``) or
    ``shade_textured_reference`` (``{"uvs": UV, "triangle_uvs": FUV, "texture": tex}``) on each request's fine view,
    then the ordered box sum.  ``requests``: ``(view20, width, height, supersample, want)`` each -> one dict per request
    with the outputs it names and ``records`` [16] uint32 (the fine view's)."""
    out = []
    for request in requests:
        view, W, H, S, want = _frame_request(request)
        fine = supersampled_view(view, S)
        if "colors" in shading:
            rgba, _, depth, nz, _, recs = shade_reference(V, F, shading["colors"], fine[None], W * S, H * S)
        else:
            triangle_uvs = shading.get("triangle_uvs")
            rgba, _, depth, nz, _, recs = shade_textured_reference(
                V, F, shading["uvs"], np.asarray(F) if triangle_uvs is None else triangle_uvs, shading["texture"],
                fine[None], W * S, H * S)
        image = box_sum(rgba[0], S)
        full = {"rgba": image, "rgb_u8": _u8(image[..., :3]), "depth": depth[0], "depth_nz": nz[0]}
        res = {k: full[k] for k in want}
        res["records"] = recs[0]
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# reference points from a frame's depth plane (pxt_points_from_depth_views)
# ---------------------------------------------------------------------------------------------------------------------
POINTS_MAX_VIEWS = _lib.PXT_POINTS_MAX_VIEWS


def _object_from_camera(view, q0, q1, q2) -> np.ndarray:
    """``p_j = (R_0j q_0 + R_1j q_1) + R_2j q_2`` in float32, one operation per step -> [n, 3]."""
    R = view[:9].reshape(3, 3)
    with np.errstate(all="ignore"):
        return np.stack([((R[0, j] * q0).astype(_F) + (R[1, j] * q1).astype(_F)).astype(_F) + (R[2, j] * q2).astype(_F)
                         for j in range(3)], -1).astype(_F)


def points_reference(depth, view20, min_alpha: float, erode: int, n_max: int):
    """The rule of pxt_points_from_depth_views for one view in numpy: ``depth`` [H, W, 4] float32 (the ``depth`` output
    of a frame call), ``view20`` the 20 floats it was drawn with -> ``(p3d float32 [n_max, 3], slot_valid uint8 [n_max],
    record int64 [4] = {accepted pixels, stride, points, candidates})``.  The selection works on whole boolean images
    (no segments, no ballot words); the back-projection is the header's, one float32 operation per step."""
    d = np.asarray(depth, np.float32)
    v = np.asarray(view20, np.float32).reshape(VIEW)
    H, W, e, n_max = int(d.shape[0]), int(d.shape[1]), int(erode), int(n_max)
    with np.errstate(invalid="ignore"):
        base = (d[..., 3] >= _F(min_alpha)) & (d[..., 0] > 0)
    accepted = np.zeros((H, W), bool)
    if H > 2 * e and W > 2 * e:  # a square that leaves the image fails
        inner = np.ones((H - 2 * e, W - 2 * e), bool)
        for dy in range(-e, e + 1):
            for dx in range(-e, e + 1):
                inner &= base[e + dy:H - e + dy, e + dx:W - e + dx]
        accepted[e:H - e, e:W - e] = inner
    A = int(accepted.sum())
    s = 1
    while s * s * n_max < A:
        s += 1
    ys, xs = np.nonzero(accepted)  # row-major order
    lattice = (xs % s == s // 2) & (ys % s == s // 2)
    xs, ys = xs[lattice], ys[lattice]
    n_candidates = len(xs)
    n = min(n_candidates, n_max)
    xs, ys = xs[:n], ys[:n]
    t = v[9:12]
    p3d = np.empty((n_max, 3), np.float32)
    with np.errstate(all="ignore"):
        z = (d[ys, xs, 0] / v[17]).astype(_F)
        xn = ((xs.astype(_F) - v[14]).astype(_F) / v[12]).astype(_F)
        yn = ((ys.astype(_F) - v[15]).astype(_F) / v[13]).astype(_F)
        c0, c1 = (z * xn).astype(_F), (z * yn).astype(_F)
        p3d[:n] = _object_from_camera(v, (c0 - t[0]).astype(_F), (c1 - t[1]).astype(_F), (z - t[2]).astype(_F))
        p3d[n:] = _object_from_camera(v, -t[0:1], -t[1:2], -t[2:3])  # the camera centre
    slot_valid = np.zeros(n_max, np.uint8)
    slot_valid[:n] = 1
    return p3d, slot_valid, np.array([A, s, n, n_candidates], np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU renderer
# ---------------------------------------------------------------------------------------------------------------------
class MeshRenderer:
    """Holds a mesh on the device and draws depth images of it (``torch.ops.pixtrack.mesh_raster``) and, given vertex
    colours, colour images and the tracker's 8-bit planes (``torch.ops.pixtrack.mesh_render``); given ``uvs`` [n, 2],
    ``triangle_uvs`` [T, 3] (default: the triangles, when there is one UV per vertex) and ``texture`` (uint8 [Ht, Wt, 3
    or 4], row 0 is v = 1) instead, the same from the texture map (``torch.ops.pixtrack.mesh_render_textured``)."""

    OUTPUTS = ("rgba", "rgb_u8", "depth", "depth_nz", "ids")

    def __init__(self, V, F, device="cuda:0", colors=None, uvs=None, triangle_uvs=None, texture=None):
        from . import ops  # registers the ops

        self._ops = ops.ops
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.PxtError("the mesh rasteriser runs on a ROCm device; no CPU path exists")
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else a
        Vn = np.ascontiguousarray(np.asarray(host(V), np.float32).reshape(-1, 3))
        Fn = np.asarray(host(F)).reshape(-1, 3)
        if len(Vn) < 1 or len(Fn) < 1:
            raise _lib.PxtError(f"a mesh needs vertices and triangles (got {len(Vn)}, {len(Fn)})")
        if Fn.min() < -(1 << 31) or Fn.max() >= (1 << 31):
            raise _lib.PxtError("triangle indices do not fit int32")
        if colors is not None:
            if uvs is not None or triangle_uvs is not None or texture is not None:
                raise _lib.PxtError("a mesh is drawn with vertex colours or with a texture map, not both")
            Cn = np.ascontiguousarray(np.asarray(host(colors), np.float32))
            if Cn.shape != Vn.shape:
                raise _lib.PxtError(f"colors is {Cn.shape}, expected one r g b per vertex {Vn.shape}")
            if not np.isfinite(Cn).all() or Cn.min() < 0.0 or Cn.max() > 1.0:
                raise _lib.PxtError("colors must be finite and inside [0, 1]")
        elif uvs is not None or triangle_uvs is not None or texture is not None:
            if uvs is None or texture is None:
                raise _lib.PxtError("a textured mesh needs uvs and texture (triangle_uvs defaults to the triangles)")
            Un = np.ascontiguousarray(np.asarray(host(uvs), np.float32))
            if Un.ndim != 2 or Un.shape[1] != 2 or not (1 <= len(Un) <= 1 << 24):
                raise _lib.PxtError(f"uvs is {Un.shape}, expected [1..2^24, 2]")
            if not np.isfinite(Un).all():
                raise _lib.PxtError("uvs must be finite")
            if triangle_uvs is None:
                if len(Un) != len(Vn):
                    raise _lib.PxtError(f"triangle_uvs is needed: {len(Un)} uvs for {len(Vn)} vertices")
                FUn = Fn
            else:
                FUn = np.asarray(host(triangle_uvs))
            if FUn.shape != Fn.shape or FUn.dtype.kind not in "iu":
                raise _lib.PxtError(f"triangle_uvs is {FUn.shape} {FUn.dtype}, expected integers {Fn.shape}")
            if FUn.min() < 0 or FUn.max() >= len(Un):
                raise _lib.PxtError(f"triangle_uvs holds indices outside the {len(Un)} uvs")
            try:
                Tn = texture_rgb(host(texture))
            except ValueError as e:
                raise _lib.PxtError(str(e)) from None
            Tn = np.concatenate([Tn, np.full(Tn.shape[:2] + (1,), 255, np.uint8)], 2)  # one texel, one dword
        self.device = dev
        self.vertices_host = Vn
        self.vertices = torch.from_numpy(Vn).to(dev)
        self.triangles = torch.from_numpy(np.ascontiguousarray(Fn.astype(np.int32))).to(dev)
        self._workspace: Optional[torch.Tensor] = None
        self._frame_plans: dict = {}
        self.colors = None if colors is None else torch.from_numpy(Cn).to(dev)
        self.uvs = self.triangle_uvs = self.texture = None
        if colors is None and uvs is not None:
            self.uvs = torch.from_numpy(Un).to(dev)
            self.triangle_uvs = torch.from_numpy(np.ascontiguousarray(FUn.astype(np.int32))).to(dev)
            self.texture = torch.from_numpy(np.ascontiguousarray(Tn)).to(dev)

    def _views_and_workspace(self, views, width, height, what):
        vh = views.detach().cpu().numpy() if torch.is_tensor(views) else views
        vh = np.ascontiguousarray(np.asarray(vh, np.float32).reshape(-1, VIEW))
        P, W, H = len(vh), int(width), int(height)
        need = int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, self.n_triangles, W, H)) if min(P, W, H) >= 1 else -1
        if need <= 0:
            raise _lib.PxtError(f"{what}: {P} views of {W} x {H} are not supported (1..4096 views, 1..2^26 pixels)")
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return torch.from_numpy(vh).to(self.device), P, W, H

    def render(self, views, width: int, height: int, want: Sequence[str] = ("rgb_u8", "depth_nz"),
               download_records: bool = True) -> dict:
        """``views`` [P, 20] -> a dict of device tensors for the outputs named in ``want`` (of ``rgba`` [P, H, W, 4],
        ``rgb_u8`` uint8 [P, H, W, 3], ``depth`` [P, H, W, 4], ``depth_nz`` uint8 [P, H, W], ``ids`` int32 [P, H, W]) and
        ``records`` ([P, 16] uint32 numpy, or the int32 device tensor with ``download_records=False``).  One call, four
        launches; the default is what the tracker takes from the NeRF renderer per frame."""
        if self.colors is None and self.texture is None:
            raise _lib.PxtError("render needs vertex colours or a texture map: MeshRenderer(V, F, device, colors=...) or "
                                "MeshRenderer(V, F, device, uvs=..., triangle_uvs=..., texture=...)")
        want = tuple(want)
        unknown = [w for w in want if w not in self.OUTPUTS]
        if unknown or not want:
            raise _lib.PxtError(f"render: want names outputs of {self.OUTPUTS} (got {want})")
        v, P, W, H = self._views_and_workspace(views, width, height, "mesh_render")
        shapes = {"rgba": ((P, H, W, 4), torch.float32), "rgb_u8": ((P, H, W, 3), torch.uint8),
                  "depth": ((P, H, W, 4), torch.float32), "depth_nz": ((P, H, W), torch.uint8),
                  "ids": ((P, H, W), torch.int32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=self.device) for k in want}
        records = torch.empty((P, RECORD), dtype=torch.int32, device=self.device)
        outs = (out.get("rgba"), out.get("rgb_u8"), out.get("depth"), out.get("depth_nz"), out.get("ids"))
        if self.texture is None:
            self._ops.mesh_render(self.vertices, self.triangles, self.colors, v, W, H, *outs, records, self._workspace)
        else:
            self._ops.mesh_render_textured(self.vertices, self.triangles, self.uvs, self.triangle_uvs, self.texture, v, W, H,
                                           *outs, records, self._workspace)
        out["records"] = records.cpu().numpy().view(np.uint32) if download_records else records
        return out

    def render_frame(self, requests, download_records: bool = True) -> list:
        """Several views of the mesh, each with its own size, supersampling and outputs, in one call of four launches
        (``torch.ops.pixtrack.mesh_render_frame``): ``requests`` = up to 8 of ``(view20, width, height, supersample in
        {1, 2, 4}, want)``, ``want`` naming outputs of ``rgba`` [H, W, 4], ``rgb_u8`` uint8 [H, W, 3] and, for supersample
        1, ``depth`` [H, W, 4] and ``depth_nz`` uint8 [H, W] -> one dict per request of device tensors and ``records``
        ([16] uint32 numpy, or the int32 device tensor with ``download_records=False``).  A supersampled view is drawn on
        the ``S W x S H`` lattice and box-filtered: colour premultiplied over black, alpha the covered fraction."""
        if self.colors is None and self.texture is None:
            raise _lib.PxtError("render_frame needs vertex colours or a texture map")
        try:
            reqs = [_frame_request(r) for r in requests]
        except ValueError as e:
            raise _lib.PxtError(f"render_frame: {e}") from None
        P = len(reqs)
        if not (1 <= P <= FRAME_MAX_VIEWS):
            raise _lib.PxtError(f"render_frame takes 1..{FRAME_MAX_VIEWS} views (got {P})")
        shape_key = tuple((W, H, S, want) for _, W, H, S, want in reqs)
        plan = self._frame_plans.get(shape_key)
        if plan is None:  # the planes' places in the four buffers and the workspace, once per shape set
            sizes, offsets, geometry = [0, 0, 0, 0], [], []
            for _, W, H, S, want in reqs:
                geometry += [W, H, S]
                for k, (name, px) in enumerate(zip(FRAME_OUTPUTS, (16, 3, 16, 1))):
                    if name in want:
                        offsets.append(sizes[k])
                        sizes[k] += (W * H * px + 15) // 16 * 16
                    else:
                        offsets.append(-1)
            need = int(_lib.lib().pxt_mesh_render_frame_workspace_bytes(P, self.n_triangles,
                                                                        (_lib.C.c_int32 * len(geometry))(*geometry)))
            if need <= 0:
                raise _lib.PxtError(f"render_frame: the views {geometry} are not supported")
            plan = (geometry, offsets, sizes, need)
            self._frame_plans[shape_key] = plan
        geometry, offsets, sizes, need = plan
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        views = torch.from_numpy(np.ascontiguousarray(np.stack([r[0] for r in reqs]))).to(self.device)
        bufs = [None if n == 0 else torch.empty(n // (4 if k in (0, 2) else 1),
                                                dtype=torch.float32 if k in (0, 2) else torch.uint8, device=self.device)
                for k, n in enumerate(sizes)]
        records = torch.empty((P, RECORD), dtype=torch.int32, device=self.device)
        self._ops.mesh_render_frame(self.vertices, self.triangles, self.colors, self.uvs, self.triangle_uvs, self.texture,
                                    views, geometry, offsets, *bufs, records, self._workspace)
        rec = records.cpu().numpy().view(np.uint32) if download_records else records
        return [_frame_planes(bufs, offsets, p, W, H, want, rec) for p, (_, W, H, S, want) in enumerate(reqs)]

    @property
    def n_vertices(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def n_triangles(self) -> int:
        return int(self.triangles.shape[0])

    def render_depth(self, views, width: int, height: int, out: Optional[torch.Tensor] = None, triangle_ids: bool = False,
                     download_records: bool = True):
        """``views`` [P, 20] (numpy or tensor) -> ``(depth [P, H, W, 4] device tensor, ids int32 [P, H, W] device tensor or
        None, records [P, 16] uint32 numpy)``.  Nothing but the records is downloaded; with ``download_records=False``
        not even those (the int32 device tensor is returned, and the host does not wait for the launches)."""
        v, P, W, H = self._views_and_workspace(views, width, height, "mesh_raster")
        if out is None:
            out = torch.empty((P, H, W, 4), dtype=torch.float32, device=self.device)
        ids = torch.empty((P, H, W), dtype=torch.int32, device=self.device) if triangle_ids else None
        records = torch.empty((P, RECORD), dtype=torch.int32, device=self.device)
        self._ops.mesh_raster(self.vertices, self.triangles, v, out, ids, records, self._workspace)
        return out, ids, (records.cpu().numpy().view(np.uint32) if download_records else records)


def frame_batch_reference(items) -> list:
    """The rule of pxt_mesh_render_frame_batch: ``frame_reference`` per item.  ``items`` = ``[(V, F, shading,
    requests)]`` -> one list of dicts per item.  A view of a batch is that view alone on its mesh: nothing is added."""
    return [frame_reference(V, F, shading, requests) for V, F, shading, requests in items]


def dilate_box(plane: np.ndarray, r: int) -> np.ndarray:
    """``plane`` bool [H, W] -> its dilation with the ``(2 r + 1)^2`` box, pixels outside the image ignored."""
    H, W = plane.shape
    padded = np.pad(np.asarray(plane, bool), int(r))
    out = np.zeros((H, W), bool)
    for dy in range(2 * int(r) + 1):
        for dx in range(2 * int(r) + 1):
            out |= padded[dy:dy + H, dx:dx + W]
    return out


SCENE_MAX_GROW = _lib.PXT_MESH_SCENE_MAX_GROW


def _scene_ids(scenes, counts, what):
    """``scenes`` = per item one scene id (an int >= 0, or None) per request -> the same as a list of lists."""
    scenes = [list(s) for s in scenes]
    if [len(s) for s in scenes] != list(counts):
        raise ValueError(f"{what}: scenes holds one id or None per item and request ({list(counts)}; got "
                         f"{[len(s) for s in scenes]})")
    for s in scenes:
        for v in s:
            if v is not None and (int(v) != v or int(v) < 0):
                raise ValueError(f"{what}: a scene id is None or an int >= 0 (got {v!r})")
    return [[None if v is None else int(v) for v in s] for s in scenes]


def scene_reference(items, scenes, r_grow: int = 0) -> list:
    """The rule of pxt_mesh_render_scene_batch in numpy: ``frame_batch_reference`` and, for every request with a scene id,
    ``"occluder"`` (uint8 [H, W]) and record words 10 (hidden pixels) and 11 (occluder pixels).  ``scenes``: per item, one
    scene id or None per request.  The views of one scene are one camera (same size, ``fx fy cx cy`` bit-equal,
    supersample 1; anything else is a ValueError).  View k is hidden at a pixel where it is covered and another member
    of its scene is covered with SMALLER z bits - read from the numpy rasteriser's own key planes, unscaled, so ``near``
    and ``depth_q`` may differ; equal bits do not hide.  The plane is that, grown by the ``(2 r_grow + 1)^2`` box inside
    the image."""
    items = [(V, F, shading, list(requests)) for V, F, shading, requests in items]
    scenes = _scene_ids(scenes, [len(it[3]) for it in items], "scene_reference")
    if not (0 <= int(r_grow) <= SCENE_MAX_GROW):
        raise ValueError(f"r_grow is 0..{SCENE_MAX_GROW} (got {r_grow})")
    out = frame_batch_reference(items)
    members: dict = {}
    for m, (V, F, _, requests) in enumerate(items):
        for q, request in enumerate(requests):
            if scenes[m][q] is None:
                continue
            view, W, H, S, _ = _frame_request(request)
            if S != 1:
                raise ValueError(f"a scene's views have supersample 1 (item {m}, request {q}: {S})")
            key, _, _ = _raster_view(np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3)),
                                     np.asarray(F).reshape(-1, 3).astype(np.int64), view, W, H, False)
            members.setdefault(scenes[m][q], []).append((m, q, view, W, H, key))
    for s, views in members.items():
        _, _, view0, W, H, _ = views[0]
        for m, q, view, Wv, Hv, _ in views:
            if (Wv, Hv) != (W, H) or view[12:16].tobytes() != view0[12:16].tobytes():
                raise ValueError(f"scene {s}: item {m}, request {q} is not the camera of the scene's first view")
        covered = [key != _EMPTY for *_, key in views]
        zbits = [(key >> np.uint64(32)).astype(np.uint32) for *_, key in views]
        for k, (m, q, *_rest) in enumerate(views):
            hidden = np.zeros(H * W, bool)
            for j in range(len(views)):
                if j != k:
                    hidden |= covered[j] & (zbits[j] < zbits[k])
            hidden &= covered[k]
            grown = dilate_box(hidden.reshape(H, W), r_grow)
            res = out[m][q]
            res["occluder"] = grown.astype(np.uint8)
            res["records"] = np.array(res["records"], np.uint32)
            res["records"][W_HIDDEN], res["records"][W_OCCLUDER] = hidden.sum(), grown.sum()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# several meshes' frames in one call (pxt_mesh_render_frame_batch, pxt_mesh_render_scene_batch)
# ---------------------------------------------------------------------------------------------------------------------
BATCH_MAX_MESHES = _lib.PXT_MESH_BATCH_MAX_MESHES
BATCH_MAX_VIEWS = _lib.PXT_MESH_BATCH_MAX_VIEWS
_BATCH_PLANS: dict = {}
_SCENE_PLANS: dict = {}


class FrameBatchWorkspace:
    """The device memory of ``render_frame_batch`` calls on ONE stream, grown to the largest batch seen.  The call's
    parameter record lives in it until the chain has finished: two streams must not share one."""

    def __init__(self):
        self.tensor: Optional[torch.Tensor] = None

    def ensure(self, n_bytes: int, device) -> torch.Tensor:
        if self.tensor is None or self.tensor.numel() < n_bytes or self.tensor.device != torch.device(device):
            self.tensor = torch.empty(int(n_bytes), dtype=torch.uint8, device=device)
        return self.tensor


def _batch_plan(shapes):
    """``shapes`` = per item (triangles, ((W, H, S, want), ...)) -> the consecutive calls that serve them: per call
    (first item, item count, view_mesh, geometry, offsets, buffer sizes, workspace bytes)."""
    calls, a = [], 0
    while a < len(shapes):
        b, P = a, 0
        while b < len(shapes) and b - a < BATCH_MAX_MESHES and P + len(shapes[b][1]) <= BATCH_MAX_VIEWS:
            P += len(shapes[b][1])
            b += 1
        if b == a:
            raise _lib.PxtError(f"render_frame_batch: an item takes 1..{BATCH_MAX_VIEWS} views (got {len(shapes[a][1])})")
        view_mesh, geometry, offsets, sizes = [], [], [], [0, 0, 0, 0]
        for m in range(a, b):
            for W, H, S, want in shapes[m][1]:
                view_mesh.append(m - a)
                geometry += [W, H, S]
                for k, (name, px) in enumerate(zip(FRAME_OUTPUTS, (16, 3, 16, 1))):
                    if name in want:
                        offsets.append(sizes[k])
                        sizes[k] += (W * H * px + 15) // 16 * 16
                    else:
                        offsets.append(-1)
        C = _lib.C
        need = int(_lib.lib().pxt_mesh_render_frame_batch_workspace_bytes(
            b - a, (C.c_int32 * (b - a))(*[shapes[m][0] for m in range(a, b)]), len(view_mesh),
            (C.c_int32 * len(view_mesh))(*view_mesh), (C.c_int32 * len(geometry))(*geometry)))
        if need <= 0:
            raise _lib.PxtError(f"render_frame_batch: the views {geometry} are not supported")
        calls.append((a, b - a, view_mesh, geometry, offsets, sizes, need))
        a = b
    return calls


def _scene_plan(shapes, plan, scenes):
    """What the calls of ``plan`` need for ``scenes`` (per item, one id or None per request): per call (view_scene,
    occluder offsets, occluder bytes, workspace bytes).  A scene whose views fall into two calls is refused."""
    call_of = {}
    out = []
    for c, (a, n, view_mesh, geometry, _offsets, _sizes, _need) in enumerate(plan):
        ids = [s for m in range(a, a + n) for s in scenes[m]]
        first, view_scene, occ_offsets, occ_bytes = {}, [], [], 0
        for p, s in enumerate(ids):
            if s is None:
                view_scene.append(-1)
                occ_offsets.append(-1)
                continue
            if call_of.setdefault(s, c) != c:
                raise _lib.PxtError(f"render_frame_batch: scene {s} would be split across two calls ({BATCH_MAX_MESHES} "
                                    f"meshes / {BATCH_MAX_VIEWS} views each): order the items so that it fits one")
            view_scene.append(first.setdefault(s, p))
            occ_offsets.append(occ_bytes)
            occ_bytes += (geometry[3 * p] * geometry[3 * p + 1] + 15) // 16 * 16
        C = _lib.C
        need = int(_lib.lib().pxt_mesh_render_scene_batch_workspace_bytes(
            n, (C.c_int32 * n)(*[shapes[m][0] for m in range(a, a + n)]), len(view_mesh),
            (C.c_int32 * len(view_mesh))(*view_mesh), (C.c_int32 * len(geometry))(*geometry)))
        if need <= 0:
            raise _lib.PxtError(f"render_frame_batch: the views {geometry} are not supported")
        out.append((view_scene, occ_offsets, occ_bytes, need))
    return out


VIEW_OUT = _lib.PXT_MESH_VIEW_OUT
W_VIEW_DONE = 20  # views_out's completion word


def posed_view_reference(pose_record, view20_host, radius) -> Tuple[np.ndarray, float]:
    """The rule of pxt_mesh_render_frame_batch_posed for one posed view: ``pose_record`` = the >= 16 floats of an LM
    output record ([0..11] the pose, [12] failed, [13] status), ``view20_host`` = the host floats of the view (fx fy cx
    cy near at [12..16] and [18..19] are taken), ``radius`` = the mesh's -> (the 20 float32 the view is drawn with, the
    completion word 1.0 / -1.0).  The pose is a bit copy; ``depth_q = 1 / (sqrt((t0 t0 + t1 t1) + t2 t2) + radius)``,
    every step one float64 operation in that order, rounded to float32 once.  The kernel's oracle: no tolerance."""
    rec = pose_record.detach().cpu().numpy() if torch.is_tensor(pose_record) else np.asarray(pose_record)
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1)
    if rec.shape[0] < 16:
        raise ValueError(f"an LM output record holds >= 16 floats (got {rec.shape[0]})")
    v = np.array(np.asarray(view20_host, np.float32).reshape(VIEW), np.float32)
    v[:12] = rec[:12]
    t0, t1, t2 = (np.float64(x) for x in rec[9:12])
    with np.errstate(all="ignore"):
        v[17] = np.float32(np.float64(1.0) / (np.sqrt((t0 * t0 + t1 * t1) + t2 * t2) + np.float64(radius)))
    return v, 1.0 if rec[12] == 0 and rec[13] == 0 else -1.0


def render_frame_batch(items, workspace: Optional[FrameBatchWorkspace] = None, download_records: bool = True,
                       scenes=None, r_grow: int = 0, poses=None, views_out: Optional[torch.Tensor] = None) -> list:
    """``MeshRenderer.render_frame`` for several meshes in one chain of launches
    (``torch.ops.pixtrack.mesh_render_frame_batch``): ``items`` = ``[(MeshRenderer, requests)]``, the requests as
    ``render_frame`` takes them -> one list of dicts per item, each dict what ``render_frame`` returns for that request,
    bit for bit.  The views' 20 floats travel in the call's parameter record: one upload for all items.  More than 16
    meshes or 32 views are served in consecutive calls.  ``workspace``: a ``FrameBatchWorkspace`` of the stream the
    call is made on (None: one for this call).

    ``scenes`` (per item, one scene id or None per request; None: exactly the call above): objects that share an image.
    The requests that name one id are one camera at supersample 1; each of their dicts gains ``"occluder"`` (uint8
    [H, W]: where another member of the scene lies in front, grown by the ``(2 r_grow + 1)^2`` box) and record words 10
    and 11 (hidden pixels, occluder pixels) - ``torch.ops.pixtrack.mesh_render_scene_batch``, one more launch,
    ``scene_reference`` bit for bit.  A scene that the 16-mesh / 32-view limits would split across two calls is a
    ``PxtError``: an incomplete scene is not drawn.

    ``poses`` (per item, per request ``None`` or ``(record, radius)``; None: exactly the call above): a request with a
    record takes its pose ON THE DEVICE from that float32 LM output record (device or pinned host memory, written by a
    launch queued ahead on this stream) and ``depth_q`` from the pose and ``radius`` - ``posed_view_reference``,
    ``torch.ops.pixtrack.mesh_render_frame_batch_posed``, one small launch more; the pose floats and ``depth_q`` of
    its host view record are ignored.  ``views_out``: float32 [all views, 24], device or pinned host - per posed view
    the 20 floats it was drawn with and the completion word (``W_VIEW_DONE``); rows in request order.  Not with
    ``scenes``."""
    items = [(r, list(requests)) for r, requests in items]
    if not items:
        return []
    if poses is None and views_out is not None:
        raise _lib.PxtError("render_frame_batch: views_out goes with poses")
    if poses is not None:
        if scenes is not None:
            raise _lib.PxtError("render_frame_batch: poses and scenes do not combine (a scene is not drawn ahead)")
        poses = [list(q) for q in poses]
        if [len(q) for q in poses] != [len(requests) for _, requests in items]:
            raise _lib.PxtError("render_frame_batch: poses holds None or (record, radius) per item and request")
        n_all = sum(len(q) for q in poses)
        if views_out is not None and tuple(views_out.shape) != (n_all, VIEW_OUT):
            raise _lib.PxtError(f"render_frame_batch: views_out is float32 [{n_all}, {VIEW_OUT}] (got {tuple(views_out.shape)})")
    device = items[0][0].device
    reqs = []
    for r, requests in items:
        if r.colors is None and r.texture is None:
            raise _lib.PxtError("render_frame_batch needs vertex colours or a texture map on every mesh")
        if r.device != device:
            raise _lib.PxtError(f"render_frame_batch: the meshes share one device (got {r.device} and {device})")
        try:
            reqs.append([_frame_request(q) for q in requests])
        except ValueError as e:
            raise _lib.PxtError(f"render_frame_batch: {e}") from None
        if not reqs[-1]:
            raise _lib.PxtError("render_frame_batch: an item without requests")
    shapes = tuple((r.n_triangles, tuple((W, H, S, want) for _, W, H, S, want in q)) for (r, _), q in zip(items, reqs))
    plan = _BATCH_PLANS.get(shapes)
    if plan is None:  # the planes' places, the calls and their workspace, once per shape set
        plan = _BATCH_PLANS[shapes] = _batch_plan(shapes)
    scene_plan = None
    if scenes is not None:
        try:
            scenes = _scene_ids(scenes, [len(q) for q in reqs], "render_frame_batch")
        except ValueError as e:
            raise _lib.PxtError(str(e)) from None
        scene_key = (shapes, tuple(tuple(s) for s in scenes))
        scene_plan = _SCENE_PLANS.get(scene_key)
        if scene_plan is None:
            scene_plan = _SCENE_PLANS[scene_key] = _scene_plan(shapes, plan, scenes)
    ws = (workspace or FrameBatchWorkspace()).ensure(max(c[-1] for c in (scene_plan or plan)), device)
    ops = items[0][0]._ops
    out = []
    for c, (a, n, view_mesh, geometry, offsets, sizes, _need) in enumerate(plan):
        part, part_reqs = [r for r, _ in items[a:a + n]], reqs[a:a + n]
        views = torch.from_numpy(np.ascontiguousarray(np.stack([q[0] for qs in part_reqs for q in qs])))
        bufs = [None if size == 0 else torch.empty(size // (4 if k in (0, 2) else 1),
                                                   dtype=torch.float32 if k in (0, 2) else torch.uint8, device=device)
                for k, size in enumerate(sizes)]
        records = torch.empty((len(view_mesh), RECORD), dtype=torch.int32, device=device)
        meshes = ([r.vertices for r in part], [r.triangles for r in part], [r.colors for r in part], [r.uvs for r in part],
                  [r.triangle_uvs for r in part], [r.texture for r in part])
        occluder, occ_offsets = None, None
        if poses is not None:
            flat = [q for qs in poses[a:a + n] for q in qs]
            row = sum(len(qs) for qs in poses[:a])
            ops.mesh_render_frame_batch_posed(
                *meshes, view_mesh, views, geometry, offsets, [None if q is None else q[0] for q in flat],
                [0.0 if q is None else float(q[1]) for q in flat], *bufs, records, ws,
                None if views_out is None else views_out[row:row + len(flat)])
        elif scene_plan is None:
            ops.mesh_render_frame_batch(*meshes, view_mesh, views, geometry, offsets, *bufs, records, ws)
        else:
            view_scene, occ_offsets, occ_bytes, _ = scene_plan[c]
            occluder = torch.empty(occ_bytes, dtype=torch.uint8, device=device) if occ_bytes else None
            ops.mesh_render_scene_batch(*meshes, view_mesh, views, geometry, offsets, view_scene, int(r_grow), occ_offsets,
                                        *bufs, occluder, records, ws)
        rec = records.cpu().numpy().view(np.uint32) if download_records else records
        p = 0
        for qs in part_reqs:
            res_item = []
            for _, W, H, S, want in qs:
                res = _frame_planes(bufs, offsets, p, W, H, want, rec)
                if occ_offsets is not None and occ_offsets[p] >= 0:
                    res["occluder"] = occluder[occ_offsets[p]:occ_offsets[p] + W * H].view(H, W)
                res_item.append(res)
                p += 1
            out.append(res_item)
    return out


def _frame_planes(bufs, offsets, p: int, W: int, H: int, want, rec) -> dict:
    """View p's planes in the four flat buffers of a frame call -> the dict ``render_frame`` returns for it."""
    res = {}
    for k, (name, px) in enumerate(zip(FRAME_OUTPUTS, (16, 3, 16, 1))):
        if name in want:
            o, ch = offsets[4 * p + k], (4, 3, 4, 1)[k]
            e = px // ch  # bytes per element
            plane = bufs[k][o // e:o // e + W * H * ch]
            res[name] = plane.view(H, W) if ch == 1 else plane.view(H, W, ch)
    res["records"] = rec[p]
    return res


# ---------------------------------------------------------------------------------------------------------------------
# procedural meshes (closed, outward-wound): the tests', the bench's and mesh_nerf_agreement's view directions
# ---------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The unit icosphere: ``(V [n, 3] float64, F [20 * 4^subdivisions, 3] int64)``."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
         (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    V = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(int(subdivisions)):
        cache, F2 = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.asarray(V, np.float64), np.asarray(F, np.int64)


def torus(major: float = 1.0, minor: float = 0.35, n_major: int = 24, n_minor: int = 12) -> Tuple[np.ndarray, np.ndarray]:
    """A torus about the z axis as ``2 * n_major * n_minor`` triangles."""
    u = np.arange(n_major) * (2 * np.pi / n_major)
    v = np.arange(n_minor) * (2 * np.pi / n_minor)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    r = major + minor * np.cos(vv)
    V = np.stack([r * np.cos(uu), r * np.sin(uu), minor * np.sin(vv)], -1).reshape(-1, 3)
    F = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b = i * n_minor + j, ((i + 1) % n_major) * n_minor + j
            c, d = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor, i * n_minor + (j + 1) % n_minor
            F += [(a, b, c), (a, c, d)]
    return V, np.asarray(F, np.int64)


def look_at_views(V, fx: float, fy: float, cx: float, cy: float, width: int, height: int, subdivisions: int = 2,
                  near: float = 1e-6, depth_q: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """Views around a mesh that look at it and hold all of it: ``(views [P, 20] float32, poses [P, 4, 4] float64,
    world -> camera)``, P = 12 / 42 / 162 for 0 / 1 / 2 subdivisions.

    The reference's rule (``create_look_at_poses_for_mesh``, ``scripts/create_sfm_from_obj.py``): the eyes sit on a
    sphere about the target in the directions of an icosphere's vertices, at the distance from which a sphere of the
    mesh's radius ``r`` (half the diagonal of its bounding box) fills the narrower field of view,
    ``max(r / sin(atan(W / 2 fx)), r / sin(atan(H / 2 fy)))``.  The camera frame is the project's: x right, y down, z
    forward; z points from the eye to the target, ``up`` is +y (+z where the direction's ``|y| > 0.999``), x =
    normalize(z x up), y = z x x; R has the rows x, y, z and t = -R eye.  ``cx, cy`` are in the ``Camera`` convention
    (pixel centres at integer coordinates).

    Two departures from the reference: the directions, and so the order of the views, are ``icosphere(subdivisions)``'s
    vertices, not trimesh's; and the target is the centre of the bounding box, not the origin - the same thing for
    BOP's centred models."""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    centre, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    dist = max(r / np.sin(np.arctan(width / (2.0 * fx))), r / np.sin(np.arctan(height / (2.0 * fy))))
    dirs, _ = icosphere(subdivisions)
    views, poses = [], []
    for d in dirs:
        eye = centre + dist * d
        z = -d
        up = np.asarray([0.0, 0.0, 1.0]) if abs(d[1]) > 0.999 else np.asarray([0.0, 1.0, 0.0])
        x = np.cross(z, up)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ eye
        poses.append(T)
        views.append(pack_view(R, T[:3, 3], fx, fy, cx, cy, near, depth_q))
    return np.stack(views), np.stack(poses)


# ---------------------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H",
              "uint16": "H", "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f",
              "double": "d", "float64": "d"}
_PLY_NUMPY = {"b": "i1", "B": "u1", "h": "<i2", "H": "<u2", "i": "<i4", "I": "<u4", "f": "<f4", "d": "<f8"}


def fan_triangles(polygons: Sequence[Sequence[int]]) -> np.ndarray:
    """Polygons -> triangles, fanned from each polygon's first vertex."""
    out = []
    for poly in polygons:
        if len(poly) < 3:
            raise ValueError(f"a face with {len(poly)} vertices")
        out.extend((poly[0], poly[k], poly[k + 1]) for k in range(1, len(poly) - 1))
    return np.asarray(out, np.int64).reshape(-1, 3)


def _read_ply(path, colors=False, uvs=False):
    with open(str(path), "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements, texture_file = None, [], None  # elements: [name, count, [(kind, name, types...)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if len(w) >= 3 and w[0] == "comment" and w[1] == "TextureFile" and texture_file is None:
            texture_file = line.split(None, 2)[2].strip()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property before any element")
            types = w[2:4] if w[1] == "list" else w[1:2]
            for ty in types:
                if ty not in _PLY_TYPES:
                    raise ValueError(f"{path}: element {elements[-1][0]}: property type {ty!r} is not supported")
            elements[-1][2].append(("list", w[-1], *types) if w[1] == "list" else ("scalar", w[-1], w[1]))
        else:
            raise ValueError(f"{path}: header line {line!r} is not supported")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: format {fmt!r} is not supported (ascii, binary_little_endian)")
    tokens = data[body:].split() if fmt == "ascii" else None
    pos = [0 if fmt == "ascii" else body]

    def scalar(ty):
        if fmt == "ascii":
            tok = tokens[pos[0]]
            pos[0] += 1
            return float(tok) if _PLY_TYPES[ty] in "fd" else int(tok)
        c = _PLY_TYPES[ty]
        (val,) = struct.unpack_from("<" + c, data, pos[0])
        pos[0] += struct.calcsize(c)
        return val

    V, C, UV, polys, seen = None, None, None, None, set()
    for name, count, props in elements:
        seen.add(name)
        if name == "vertex":
            names = [p[1] for p in props]
            if any(p[0] != "scalar" for p in props) or not all(k in names for k in "xyz"):
                raise ValueError(f"{path}: element vertex needs scalar properties x, y, z (got {names})")
            cols = [names.index(k) for k in "xyz"]
            if fmt == "binary_little_endian":  # fixed-size rows: one structured read
                dt = np.dtype([(n, _PLY_NUMPY[_PLY_TYPES[p[2]]]) for n, p in zip(names, props)])
                rows = np.frombuffer(data, dt, count, pos[0])
                pos[0] += count * dt.itemsize
                V = np.stack([rows[k].astype(np.float64) for k in "xyz"], 1).reshape(-1, 3)
                column = lambda k: rows[k].astype(np.float64)
            else:
                rows = np.asarray([[scalar(p[2]) for p in props] for _ in range(count)], np.float64).reshape(count, len(props))
                V = rows[:, cols]
                column = lambda k: rows[:, names.index(k)]
            if colors and all(k in names for k in ("red", "green", "blue")):  # integers are 0..255, floats 0..1
                C = np.stack([column(k) / (1.0 if _PLY_TYPES[props[names.index(k)][2]] in "fd" else 255.0)
                              for k in ("red", "green", "blue")], 1).reshape(-1, 3)
            for ku, kv in (("texture_u", "texture_v"), ("s", "t")):
                if uvs and UV is None and ku in names and kv in names:
                    UV = np.stack([column(ku), column(kv)], 1).reshape(-1, 2)
        elif name == "face":
            lists = [p for p in props if p[0] == "list"]
            if len(lists) != 1 or lists[0][1] not in ("vertex_indices", "vertex_index"):
                raise ValueError(f"{path}: element face needs one list property vertex_indices / vertex_index "
                                 f"(got {[p[1] for p in props]})")
            polys = []
            for _ in range(count):
                for p in props:
                    if p[0] == "list":
                        n = scalar(p[2])
                        polys.append([scalar(p[3]) for _ in range(n)])
                    else:
                        scalar(p[2])
        else:  # an element this reader has no use for: skipped when its rows can be walked, refused otherwise
            for _ in range(count):
                for p in props:
                    if p[0] == "list":
                        for _ in range(scalar(p[2])):
                            scalar(p[3])
                    else:
                        scalar(p[2])
    for need in ("vertex", "face"):
        if need not in seen:
            raise ValueError(f"{path}: no element {need}")
    if uvs:
        return V, fan_triangles(polys), UV, texture_file
    return (V, fan_triangles(polys), C) if colors else (V, fan_triangles(polys))


def _read_obj_polygons(path):
    V, polys = [], []
    with open(str(path)) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                V.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                polys.append([int(x.split("/")[0]) for x in w[1:]])
    n = len(V)
    polys = [[i - 1 if i > 0 else n + i for i in poly] for poly in polys]  # 1-based, negative = from the end
    return np.asarray(V, np.float64).reshape(-1, 3), fan_triangles(polys)


def read_mesh(path) -> Tuple[np.ndarray, np.ndarray]:
    """``(V [n, 3] float64, F [m, 3] int64)`` of an OBJ (what ``mesh.write_obj`` writes, through ``mesh.read_obj``; faces
    with more than three vertices are fanned) or a PLY (ASCII or binary_little_endian; vertex ``x y z``, faces as
    ``vertex_indices`` / ``vertex_index`` lists, fanned).  Anything else is refused by name."""
    from . import mesh

    suffix = Path(str(path)).suffix.lower()
    if suffix == ".obj":
        V, F, _ = mesh.read_obj(path)
        Vp, Fp = _read_obj_polygons(path)
        if len(Fp) != len(F):  # polygons or negative indices: read_obj keeps the first three corners only
            V, F = Vp, Fp
    elif suffix == ".ply":
        V, F = _read_ply(path)
    else:
        raise ValueError(f"{path}: mesh format {suffix!r} is not supported (.obj, .ply)")
    if len(V) == 0 or len(F) == 0:
        raise ValueError(f"{path}: {len(V)} vertices and {len(F)} triangles")
    if F.min() < 0 or F.max() >= len(V):
        raise ValueError(f"{path}: face indices outside the {len(V)} vertices")
    return V, F


def read_mesh_colors(path) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """``read_mesh`` plus the vertex colours: ``(V, F, C [n, 3] float64 in 0..1, or None for a file without them)``.
    PLY: the vertex properties ``red green blue`` - integer types (BOP's uchar) are divided by 255, float types are
    taken as 0..1; an ``alpha`` property is ignored.  OBJ: ``v x y z r g b`` (what ``mesh.write_obj`` writes).  Texture
    maps (OBJ ``vt`` / ``usemtl``, PLY ``texture_u``) are ``read_mesh_textured``'s: a textured model without vertex
    colours comes back with ``None`` here."""
    from . import mesh

    V, F = read_mesh(path)
    if Path(str(path)).suffix.lower() == ".ply":
        C = _read_ply(path, colors=True)[2]
    else:
        C = mesh.read_obj(path)[2]
        C = C if C is not None and len(C) == len(V) else None
    return V, F, C


def _read_obj_textured(path, require_image=True):
    """The textured half of an OBJ: ``v``, ``vt``, ``f v/vt[/vn]``, ``mtllib`` and ``usemtl`` -> (V, F, UV, FUV, the
    texture's path), or None for a file none of whose faces names a ``vt``."""
    path = Path(str(path))
    V, UV, faces, libs, used = [], [], [], [], []
    with open(str(path)) as f:
        for n, line in enumerate(f, 1):
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                V.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                UV.append([float(x) for x in w[1:3]])
            elif w[0] == "f":
                faces.append((n, [c.split("/") for c in w[1:]], len(V), len(UV)))
            elif w[0] == "mtllib":
                libs.append(line.split(None, 1)[1].strip())
            elif w[0] == "usemtl" and w[1:] and w[1] not in used:
                used.append(w[1])
    textured = [all(len(c) >= 2 and c[1] != "" for c in corners) for _, corners, _, _ in faces]
    if not any(textured):
        return None
    polys, uv_polys = [], []
    for (n, corners, nv, nt), has in zip(faces, textured):
        if not has:
            raise ValueError(f"{path}: line {n}: a face without vt in a file with textured faces")
        vi, ti = [int(c[0]) for c in corners], [int(c[1]) for c in corners]
        polys.append([i - 1 if i > 0 else nv + i for i in vi])  # 1-based; negative = from the last one read so far
        uv_polys.append([i - 1 if i > 0 else nt + i for i in ti])
    F, FUV = fan_triangles(polys), fan_triangles(uv_polys)
    V, UV = np.asarray(V, np.float64).reshape(-1, 3), np.asarray(UV, np.float64).reshape(-1, 2)
    if F.min() < 0 or F.max() >= len(V) or FUV.min() < 0 or FUV.max() >= len(UV):
        raise ValueError(f"{path}: face indices outside the {len(V)} vertices or the {len(UV)} texture coordinates")
    if not libs:
        raise ValueError(f"{path}: textured faces but no mtllib")
    maps = {}  # material -> map_Kd
    for lib in libs:
        mtl = path.parent / lib
        if not mtl.is_file():
            raise ValueError(f"{path}: material library {mtl} is missing")
        current = None
        for line in mtl.read_text().splitlines():
            w = line.split()
            if w[:1] == ["newmtl"] and len(w) > 1:
                current = w[1]
            elif w[:1] == ["map_Kd"] and len(w) > 1 and current is not None:
                maps[current] = w[-1]  # options (-clamp on ...) come before the file name
    wanted = used if used else sorted(maps)
    unknown = [m for m in wanted if m not in maps]
    names = sorted({maps[m] for m in wanted if m in maps})
    if len(names) > 1:
        raise ValueError(f"{path}: several texture maps ({', '.join(names)}); one map_Kd per mesh is supported")
    if not names or (unknown and used):
        raise ValueError(f"{path}: no map_Kd for material {(unknown or wanted or ['?'])[0]!r} in {', '.join(libs)}")
    image = path.parent / names[0]
    if require_image and not image.is_file():
        raise ValueError(f"{path}: texture map {image} is missing")
    return V, F, UV, FUV, image


def read_mesh_textured(path, require_image: bool = True):
    """``(V [n, 3], F [m, 3], UV [k, 2] float64, FUV [m, 3] int64, the texture map's path)`` of a textured mesh, or None
    for a file without texture coordinates.

    OBJ: ``vt`` lines and faces ``v/vt`` or ``v/vt/vn`` (1-based and negative indices, polygons fanned with their UVs);
    ``mtllib`` names the ``.mtl`` beside the OBJ and ``usemtl`` the material whose ``map_Kd`` is the map, relative to the
    OBJ's folder.  One map per mesh: materials with different maps, a missing ``.mtl`` or image and a face without ``vt``
    among textured ones are refused by name.  PLY: the vertex properties ``texture_u texture_v`` (or ``s t``) and
    ``comment TextureFile NAME`` (BOP's models); ``FUV = F``.  Texture coordinates in PLY face lists are not read.
    ``require_image=False`` returns the map's path without asking that the file be there (the caller has another)."""
    path = Path(str(path))
    suffix = path.suffix.lower()
    if suffix == ".obj":
        return _read_obj_textured(path, require_image)
    if suffix != ".ply":
        raise ValueError(f"{path}: mesh format {suffix!r} is not supported (.obj, .ply)")
    V, F, UV, name = _read_ply(path, uvs=True)
    if UV is None:
        return None
    if len(V) == 0 or len(F) == 0 or F.min() < 0 or F.max() >= len(V):
        raise ValueError(f"{path}: face indices outside the {len(V)} vertices")
    if name is None:
        raise ValueError(f"{path}: texture_u / texture_v but no comment TextureFile")
    image = path.parent / name
    if require_image and not image.is_file():
        raise ValueError(f"{path}: texture map {image} is missing")
    return V, F, UV, F.copy(), image


def read_texture(path) -> np.ndarray:
    """An image file as a uint8 [Ht, Wt, 3] texture map (row 0 on top, v = 1)."""
    from PIL import Image

    with Image.open(str(path)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))
