"""Depth renders of a triangle mesh: the GPU rasteriser (pxt_mesh_raster, csrc/pxt_raster.hip), its numpy restatement and
the readers that feed it.

The reference draws meshes with pytorch3d (``pixtrack/utils/pytorch3d_render_utils.py:55-93``, ``render_image``;
``scripts/create_sfm_from_obj.py``; the YCB ground-truth notebook).  Here the renders serve the evaluation stack: BOP's
VSD compares depth renders of the model's mesh at the estimated and the ground-truth pose through the camera's real
intrinsics (``mesh_evaluation.py``), and the mesh ``mesh.py`` extracts can be held against the NeRF it came from.

``rasterize_reference`` restates the rule of ``include/pixtrack_hip.h`` in numpy float32 / int64 arithmetic; the kernel
is held to it bit for bit on the depth image, the triangle ids and the records.  There is no CPU product path: the
restatement draws a few thousand triangles per second and exists for the tests.
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


def _raster_view(V, F, view, W, H, want_cov):
    key = np.full(H * W, _EMPTY, np.uint64)
    cov = np.zeros(H * W, np.int32) if want_cov else None
    rec = np.zeros(RECORD, np.uint32)
    rec[W_ZMIN] = 0xFFFFFFFF
    if not np.all(np.isfinite(view)):
        rec[W_STATUS] = 0xFFFFFFFF
        return key, cov, rec
    R, t = view[:9].reshape(3, 3), view[9:12]
    fx, fy, cx, cy, near = view[12], view[13], view[14], view[15], view[16]
    nV = len(V)
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


# ---------------------------------------------------------------------------------------------------------------------
# the GPU renderer
# ---------------------------------------------------------------------------------------------------------------------
class MeshRenderer:
    """Holds a mesh on the device and draws depth images of it (``torch.ops.pixtrack.mesh_raster``)."""

    def __init__(self, V, F, device="cuda:0"):
        from . import ops  # registers the ops

        self._ops = ops.ops
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.PxtError("the mesh rasteriser runs on a ROCm device; no CPU path exists")
        Vn = np.ascontiguousarray(np.asarray(V.detach().cpu().numpy() if torch.is_tensor(V) else V, np.float32).reshape(-1, 3))
        Fn = np.asarray(F.detach().cpu().numpy() if torch.is_tensor(F) else F).reshape(-1, 3)
        if len(Vn) < 1 or len(Fn) < 1:
            raise _lib.PxtError(f"a mesh needs vertices and triangles (got {len(Vn)}, {len(Fn)})")
        if Fn.min() < -(1 << 31) or Fn.max() >= (1 << 31):
            raise _lib.PxtError("triangle indices do not fit int32")
        self.device = dev
        self.vertices_host = Vn
        self.vertices = torch.from_numpy(Vn).to(dev)
        self.triangles = torch.from_numpy(np.ascontiguousarray(Fn.astype(np.int32))).to(dev)
        self._workspace: Optional[torch.Tensor] = None

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
        vh = views.detach().cpu().numpy() if torch.is_tensor(views) else views
        vh = np.ascontiguousarray(np.asarray(vh, np.float32).reshape(-1, VIEW))
        P, W, H = len(vh), int(width), int(height)
        need = int(_lib.lib().pxt_mesh_raster_workspace_bytes(P, self.n_triangles, W, H)) if min(P, W, H) >= 1 else -1
        if need <= 0:
            raise _lib.PxtError(f"mesh_raster: {P} views of {W} x {H} are not supported (1..4096 views, 1..2^26 pixels)")
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty((P, H, W, 4), dtype=torch.float32, device=self.device)
        ids = torch.empty((P, H, W), dtype=torch.int32, device=self.device) if triangle_ids else None
        records = torch.empty((P, RECORD), dtype=torch.int32, device=self.device)
        self._ops.mesh_raster(self.vertices, self.triangles, torch.from_numpy(vh).to(self.device), out, ids, records,
                              self._workspace)
        return out, ids, (records.cpu().numpy().view(np.uint32) if download_records else records)


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


def _read_ply(path):
    with open(str(path), "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []  # elements: [name, count, [(kind, name, types...)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
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

    V, polys, seen = None, None, set()
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
            else:
                rows = [[scalar(p[2]) for p in props] for _ in range(count)]
                V = np.asarray(rows, np.float64).reshape(count, len(props))[:, cols]
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
    return V, fan_triangles(polys)


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
