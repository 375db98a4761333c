"""NeRF mesh extraction: a triangle mesh, model points and BOP's diameter for an object that only has a NeRF snapshot.

The reference's users get their mesh from instant-ngp (``testbed.compute_and_save_marching_cubes_mesh("test.obj",
[128, 128, 128])``, pixtrack/pose_trackers/pixloc_tracker_ycb.py:94).  Here the density network is evaluated on a lattice
by the renderer's own device code (``pxt_ngp_query``), the iso-surface of that lattice is extracted on the GPU
(csrc/pxt_iso.hip: ``pxt_iso_surface_count`` / ``pxt_iso_surface_emit``) and its diameter - the largest distance between
two vertices, as BOP's ``models_info.json`` defines it - by ``pxt_max_pairwise_distance``.  The files written are the ones
the evaluation command lines read: ``points.xyz`` (``evaluation.read_vertices``) and ``models_info.json``
(``symmetry.read_models_info``).

The triangulation is marching TETRAHEDRA on the Freudenthal (Kuhn) split of every cell - about twice the triangles of
marching cubes, no ambiguous cases, closed and oriented wherever the surface stays inside the lattice.  The rule is
stated in include/pixtrack_hip.h and restated in numpy by ``iso_surface_reference`` below, which builds its own case
table from the unit cube; the GPU result equals it bit for bit.

    python -m pixtrack_amd.mesh --object_path P [--obj_aabb B] [--resolution 128] [--thresh 2.5] [--keep largest|all]
                                [--frame sfm|ngp] --out_dir D

``thresh`` applies to the density LOGIT as ``pxt_ngp_query`` returns it.  2.5 is instant-ngp's default number for its own
density scale; it is an untuned starting value here.
"""
from __future__ import annotations

import argparse
import itertools
import json
import time
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

F32 = np.float32
# edge type -> (dx, dy, dz) of its far end
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
_EDGE_TYPE = {d: e for e, d in enumerate(EDGE_DIRS)}
QUERY_DIR = (0.0, 0.0, 1.0)  # the fixed view direction of density queries (the density does not depend on it)
_SLAB_POINTS = 1 << 21


# ---------------------------------------------------------------------------------------------------------------------
# the rule, in numpy
# ---------------------------------------------------------------------------------------------------------------------
def case_table() -> np.ndarray:
    """int32 [6, 16, 7], the layout of ``pxt_iso_case_table``: per (tetrahedron, code) the number of triangles and their
    vertices as ``(owner corner << 3) | edge type``, -1 where unused.  Built here from the geometry of the unit cube."""
    table = np.full((6, 16, 7), -1, np.int32)
    for t, perm in enumerate(itertools.permutations(range(3))):
        corners = [np.zeros(3, int)]
        for axis in perm:
            nxt = corners[-1].copy()
            nxt[axis] = 1
            corners.append(nxt)
        corners = [corners[0], corners[1], corners[2], corners[3]]  # c, c + e_a, c + e_a + e_b, c + (1, 1, 1)

        def edge(u, w):
            lo, hi = min(u, w), max(u, w)
            owner = int(corners[lo] @ (1, 2, 4))
            return (owner << 3) | _EDGE_TYPE[tuple(corners[hi] - corners[lo])], 0.5 * (corners[lo] + corners[hi])

        for code in range(16):
            ins = [i for i in range(4) if (code >> i) & 1]
            outs = [i for i in range(4) if not (code >> i) & 1]
            if len(ins) in (0, 4):
                table[t, code, 0] = 0
                continue
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(i, outs[0]) for i in ins]]
            else:
                (a, b), (c, d) = ins, outs
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            outward = np.mean([corners[i] for i in outs], axis=0) - np.mean([corners[i] for i in ins], axis=0)
            table[t, code, 0] = len(tris)
            for i, tri in enumerate(tris):
                refs, mids = zip(*(edge(u, w) for u, w in tri))
                refs = list(refs)
                if np.dot(np.cross(mids[1] - mids[0], mids[2] - mids[0]), outward) < 0:
                    refs[1], refs[2] = refs[2], refs[1]
                table[t, code, 1 + 3 * i:4 + 3 * i] = refs
    return table


def _lattice_gradient(v: np.ndarray, spacing) -> np.ndarray:
    """float32 [3, nz, ny, nx]: central differences, one-sided at the border, 0 along an axis of extent 1."""
    out = np.zeros((3,) + v.shape, F32)
    for ax_xyz, ax in ((0, 2), (1, 1), (2, 0)):
        n = v.shape[ax]
        i = np.arange(n)
        hi, lo = np.minimum(i + 1, n - 1), np.maximum(i - 1, 0)
        diff = np.take(v, hi, axis=ax) - np.take(v, lo, axis=ax)
        den = (hi - lo).astype(F32) * F32(spacing[ax_xyz])
        shape = [1, 1, 1]
        shape[ax] = n
        den = den.reshape(shape)
        with np.errstate(all="ignore"):
            out[ax_xyz] = np.where(den != 0, diff / np.where(den != 0, den, F32(1)), F32(0))
    return out


def iso_surface_reference(values, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals: bool = False):
    """The iso-surface rule of include/pixtrack_hip.h in numpy float32: ``(V [n, 3] float32, F [m, 3] int32)`` and, with
    ``normals``, ``N [n, 3] float32``.  ``values`` is [nz, ny, nx]."""
    v = np.ascontiguousarray(np.asarray(values, F32))
    assert v.ndim == 3 and min(v.shape) >= 1
    nz, ny, nx = v.shape
    n_pts = v.size
    iso, origin, spacing = F32(iso), np.asarray(origin, F32), np.asarray(spacing, F32)
    with np.errstate(invalid="ignore"):
        inside = v >= iso
    carry = np.zeros((n_pts, 7), bool)
    cv = carry.reshape(nz, ny, nx, 7)
    for e, (dx, dy, dz) in enumerate(EDGE_DIRS):
        cv[:nz - dz, :ny - dy, :nx - dx, e] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    vid = (np.cumsum(carry.ravel(), dtype=np.int64) - 1).reshape(n_pts, 7)
    p, e = np.nonzero(carry)  # lexicographic in (p, edge type)
    d = np.asarray(EDGE_DIRS, np.int64)[e]
    far = p + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny
    flat = v.ravel()
    va, vb = flat[p], flat[far]
    with np.errstate(all="ignore"):
        t = (iso - va) / (vb - va)
        t = np.where(np.isnan(t), F32(0.5), np.clip(t, F32(0), F32(1))).astype(F32)
    xyz = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], axis=1).astype(F32)
    V = (origin[None, :] + (xyz + t[:, None] * d.astype(F32)) * spacing[None, :]).astype(F32)

    N = None
    if normals:
        g = _lattice_gradient(v, spacing).reshape(3, n_pts)
        with np.errstate(all="ignore"):
            ga, gb = g[:, p], g[:, far]
            nrm = -(ga + t[None, :] * (gb - ga))
            length = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
            ok = (length > 0) & np.isfinite(length)
            N = np.where(ok[None, :], nrm / np.where(ok, length, F32(1))[None, :], F32(0)).T.astype(F32)
        N = np.ascontiguousarray(N)

    # triangles: by cell, tetrahedron, triangle within the case
    F = np.zeros((0, 3), np.int32)
    if min(nx, ny, nz) >= 2:
        corner_in, corner_off = [], []
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
            corner_in.append(inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx])
            corner_off.append(dx + dy * nx + dz * nx * ny)
        n_in = np.sum(corner_in, axis=0)
        mixed = (n_in > 0) & (n_in < 8)
        zc, yc, xc = np.nonzero(mixed)  # ascending in p
        base = (zc * ny + yc) * nx + xc
        cin = np.stack([c[mixed] for c in corner_in], axis=1)  # [cells, 8]
        table = case_table()
        corner_off = np.asarray(corner_off, np.int64)
        ids = np.zeros((len(base), 6, 2, 3), np.int64)
        live = np.zeros((len(base), 6, 2), bool)
        for ti, perm in enumerate(itertools.permutations(range(3))):
            c1 = 1 << perm[0]
            c2 = c1 | (1 << perm[1])
            code = cin[:, 0] * 1 + cin[:, c1] * 2 + cin[:, c2] * 4 + cin[:, 7] * 8
            entry = table[ti][code]  # [cells, 7]
            for i in range(2):
                live[:, ti, i] = entry[:, 0] > i
                for j in range(3):
                    ref = np.maximum(entry[:, 1 + 3 * i + j], 0)
                    ids[:, ti, i, j] = vid[base + corner_off[ref >> 3], ref & 7]
        F = ids[live].astype(np.int32)
    return (V, F, N) if normals else (V, F)


def native_case_table() -> np.ndarray:
    """The table the kernels use (``pxt_iso_case_table``; host only, needs no GPU)."""
    import ctypes as C

    out = (C.c_int32 * _lib.PXT_ISO_CASE_TABLE_WORDS)()
    _lib.check(_lib.lib().pxt_iso_case_table(out), "pxt_iso_case_table")
    return np.array(out, np.int32).reshape(6, 16, 7)


# ---------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------
def _grid7(iso, origin, spacing):
    o, s = np.asarray(origin, F32).reshape(3), np.asarray(spacing, F32).reshape(3)
    return [float(F32(iso))] + [float(x) for x in o] + [float(x) for x in s]


def iso_surface(values: torch.Tensor, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals: bool = False):
    """``values`` [nz, ny, nx] float32 on the device -> ``(V [n, 3] float32, F [m, 3] int32)`` device tensors and, with
    ``normals``, ``N``.  One host synchronisation: the two counts are read before the arrays are allocated."""
    from .ops import ops

    _lib.require_gpu(values, "values")
    if values.dim() != 3 or values.dtype != torch.float32:
        raise _lib.PxtError(f"iso_surface: values is a float32 [nz, ny, nx] tensor (got {tuple(values.shape)}, {values.dtype})")
    values = values.contiguous()
    nz, ny, nx = (int(s) for s in values.shape)
    need = int(_lib.lib().pxt_iso_surface_workspace_bytes(nx, ny, nz)) if min(nx, ny, nz) >= 1 else -1
    if need <= 0:
        raise _lib.PxtError(f"iso_surface: a {nz} x {ny} x {nx} lattice is not supported (every extent >= 1, <= 2^27 points)")
    dev = values.device
    grid = _grid7(iso, origin, spacing)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.iso_surface_count(values, grid, workspace, counts)
    n, m = (int(c) for c in counts.cpu().tolist())
    V = torch.empty(n, 3, dtype=torch.float32, device=dev)
    F = torch.empty(m, 3, dtype=torch.int32, device=dev)
    N = torch.empty(n, 3, dtype=torch.float32, device=dev) if normals else None
    ops.iso_surface_emit(values, grid, workspace, V, N, F)
    return (V, F, N) if normals else (V, F)


def max_pairwise_distance(points: torch.Tensor) -> Tuple[float, int, int]:
    """BOP's diameter of a point set: ``(d, i, j)``, the largest fp32 distance between two of ``points`` [n, 3] (device)
    and the lowest pair (i <= j) that has it."""
    from .ops import ops

    _lib.require_gpu(points, "points")
    points = points.to(torch.float32).contiguous()
    need = int(_lib.lib().pxt_max_pairwise_distance_workspace_bytes(int(points.shape[0])))
    if need <= 0:
        raise _lib.PxtError(f"max_pairwise_distance: {int(points.shape[0])} points is not supported (1..2^22)")
    workspace = torch.empty(need, dtype=torch.uint8, device=points.device)
    out = torch.zeros(4, dtype=torch.int32, device=points.device)
    ops.max_pairwise_distance(points, out, workspace)
    host = out.cpu().numpy()
    return float(host[:1].view(np.float32)[0]), int(host[1]), int(host[2])


# ---------------------------------------------------------------------------------------------------------------------
# host: invariants, components
# ---------------------------------------------------------------------------------------------------------------------
def mesh_invariants(V, F) -> Dict:
    """What a closed oriented mesh must satisfy, counted on the host: ``directed_edges_repeated`` (directed edges used
    more than once), ``directed_edges_unpaired`` (directed edges without their reverse), ``euler`` (referenced vertices -
    edges + triangles), ``volume`` (signed; positive when the normals point outwards), ``area``, ``zero_area_triangles``
    and ``unreferenced_vertices``."""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    n = max(len(V), 1)
    a = F[:, [0, 1, 2]].ravel()
    b = F[:, [1, 2, 0]].ravel()
    key, count = np.unique(a * n + b, return_counts=True)
    rev = (key % n) * n + key // n
    undirected = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    used = np.unique(F)
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    cross = np.cross(p1 - p0, p2 - p0)
    area = 0.5 * np.linalg.norm(cross, axis=1)
    return {"directed_edges_repeated": int((count > 1).sum()),
            "directed_edges_unpaired": int((~np.isin(rev, key)).sum()),
            "euler": int(len(used) - len(undirected) + len(F)),
            "volume": float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0),
            "area": float(area.sum()),
            "zero_area_triangles": int((area == 0).sum()),
            "unreferenced_vertices": int(len(V) - len(used))}


def triangle_components(n_vertices: int, F) -> Tuple[int, np.ndarray]:
    """(number of connected components among the referenced vertices, component label per triangle)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return 0, np.zeros(0, np.int64)
    rows = np.concatenate([F[:, 0], F[:, 1]])
    cols = np.concatenate([F[:, 1], F[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
    _, labels = connected_components(graph, directed=False)
    tri = labels[F[:, 0]]
    uniq, tri = np.unique(tri, return_inverse=True)
    return len(uniq), tri


def keep_triangles(arrays: Sequence[Optional[np.ndarray]], F: np.ndarray, keep: np.ndarray):
    """The triangles ``F[keep]`` with the vertex arrays cut down to what they reference (vertex order kept)."""
    F = np.asarray(F)[keep]
    used = np.unique(F)
    remap = np.full(max(len(arrays[0]), 1), -1, np.int64)
    remap[used] = np.arange(len(used))
    return [None if a is None else a[used] for a in arrays], remap[F].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# NeRF -> lattice -> mesh
# ---------------------------------------------------------------------------------------------------------------------
def _box(testbed, aabb):
    if aabb is None:
        aabb = testbed.render_aabb
    if hasattr(aabb, "min"):
        aabb = (aabb.min, aabb.max)
    lo, hi = np.asarray(aabb[0], np.float64).reshape(3), np.asarray(aabb[1], np.float64).reshape(3)
    if not (hi > lo).all():
        raise ValueError(f"the box {lo.tolist()} .. {hi.tolist()} is empty")
    return lo, hi


def lattice_frame(resolution, lo, hi, pad: float = 0.05):
    """``(shape (nz, ny, nx), origin float32 [3], spacing float32 [3])`` of a lattice whose points span the box
    ``lo .. hi`` grown by ``pad`` of its extent per side, from end to end."""
    res = [int(resolution)] * 3 if np.isscalar(resolution) else [int(r) for r in resolution]
    if len(res) != 3 or min(res) < 2:
        raise ValueError(f"resolution is one number or (nx, ny, nz), each >= 2 (got {resolution})")
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    lo, hi = lo - pad * ext, hi + pad * ext
    spacing = ((hi - lo) / (np.asarray(res) - 1)).astype(F32)
    return (res[2], res[1], res[0]), lo.astype(F32), spacing


def lattice_points_host(shape, origin, spacing, z0: int = 0, z1: Optional[int] = None) -> np.ndarray:
    """float32 [n, 3] positions of the lattice's slab z0 .. z1, x fastest: origin + index * spacing in float32 - the
    arithmetic ``density_lattice`` does with torch."""
    nz, ny, nx = shape
    z1 = nz if z1 is None else z1
    ax = [origin[k] + np.arange(n, dtype=F32) * spacing[k] for k, n in ((0, nx), (1, ny), (2, nz))]
    zz, yy, xx = np.meshgrid(ax[2][z0:z1], ax[1], ax[0], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(F32)


def density_lattice(testbed, resolution, aabb=None, pad: float = 0.05):
    """The density logit of ``testbed``'s NeRF on a lattice over the render box (or ``aabb``), grown by ``pad`` of its
    extent per side: ``(values [nz, ny, nx] float32 on the device, origin, spacing)``.  The network is evaluated by
    ``pxt_ngp_query`` in z-slabs of bounded size with a fixed view direction; channel 0 is kept."""
    from .ops import ops

    assert testbed._ctx is not None, "load_snapshot first"
    lo, hi = _box(testbed, aabb)
    shape, origin, spacing = lattice_frame(resolution, lo, hi, pad)
    nz, ny, nx = shape
    dev = testbed.device
    o, s = torch.from_numpy(origin).to(dev), torch.from_numpy(spacing).to(dev)
    ax = [o[k] + torch.arange(n, dtype=torch.float32, device=dev) * s[k] for k, n in ((0, nx), (1, ny), (2, nz))]
    values = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
    slab = max(1, _SLAB_POINTS // (nx * ny))
    dirs = torch.tensor(QUERY_DIR, dtype=torch.float32, device=dev).expand(slab * nx * ny, 3).contiguous()
    for z0 in range(0, nz, slab):
        z1 = min(nz, z0 + slab)
        zz, yy, xx = torch.meshgrid(ax[2][z0:z1], ax[1], ax[0], indexing="ij")
        pos = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).contiguous()
        out = torch.empty(pos.shape[0], 4, dtype=torch.float32, device=dev)
        ops.ngp_query(testbed._ctx_int(), pos, dirs[:pos.shape[0]], out)
        values[z0:z1] = out[:, 0].reshape(z1 - z0, ny, nx)
    return values, origin, spacing


def close_lattice_border(values: torch.Tensor, thresh: float) -> torch.Tensor:
    """A copy of ``values`` whose outer layer is ``min(v, thresh - 1)``: the iso-surface closes at the box."""
    v = values.clone()
    cap = float(thresh) - 1.0
    for dim in range(3):
        for idx in (0, v.shape[dim] - 1):
            face = v.select(dim, idx)
            face.copy_(torch.clamp(face, max=cap))
    return v


def extract_mesh(testbed, resolution=128, thresh: float = 2.5, aabb=None, close_border: bool = True, keep: str = "largest",
                 colors: bool = True, nerf2sfm=None, pad: float = 0.05) -> Dict:
    """The NeRF's surface as a mesh.  Returns host arrays ``V`` [n, 3], ``F`` [m, 3] int32, ``N`` [n, 3] (unit normals,
    pointing out of the object), ``C`` [n, 3] (the colour network at the vertices seen along -N; None without
    ``colors``), and ``frame`` ("ngp", or "sfm" when ``nerf2sfm`` is given: vertices in SfM units through
    ``ngp.ngp_to_sfm_affine``), ``n_components`` (before ``keep``), ``diameter`` (``max_pairwise_distance`` of V),
    ``diameter_pair``, ``bbox`` (min xyz, size xyz), ``invariants`` (``mesh_invariants``) and ``times`` (seconds of
    lattice, extraction, diameter).

    ``thresh`` is a density LOGIT (instant-ngp's default 2.5 is an untuned starting value here); ``close_border`` caps
    the lattice's outer layer below it so that the mesh closes at the box; ``keep="largest"`` keeps the connected
    component with the most triangles (NeRF floaters would inflate the diameter), ``"all"`` everything.  The
    triangulation is tetrahedral: about twice the triangles of marching cubes."""
    from .ops import ops

    if keep not in ("largest", "all"):
        raise ValueError(f"keep is 'largest' or 'all' (got {keep!r})")
    dev = testbed.device
    times = {}

    def clock(name, t0):
        torch.cuda.synchronize(dev)
        times[name] = time.perf_counter() - t0

    t0 = time.perf_counter()
    lattice, origin, spacing = density_lattice(testbed, resolution, aabb, pad)
    clock("lattice", t0)
    t0 = time.perf_counter()
    if close_border:
        lattice = close_lattice_border(lattice, thresh)
    Vd, Fd, Nd = iso_surface(lattice, thresh, origin, spacing, normals=True)
    clock("extraction", t0)
    V, F, N = Vd.cpu().numpy(), Fd.cpu().numpy(), Nd.cpu().numpy()
    n_components, tri_label = triangle_components(len(V), F)
    if keep == "largest" and n_components > 0:
        (V, N), F = keep_triangles([V, N], F, tri_label == np.argmax(np.bincount(tri_label)))
    C = None
    if colors and len(V):
        view = -N
        view[np.linalg.norm(view, axis=1) == 0] = QUERY_DIR
        out = torch.empty(len(V), 4, dtype=torch.float32, device=dev)
        ops.ngp_query(testbed._ctx_int(), torch.from_numpy(np.ascontiguousarray(V)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(view, F32)).to(dev), out)
        C = out[:, 1:4].cpu().numpy()
    frame = "ngp"
    if nerf2sfm is not None:
        from .ngp import ngp_to_sfm_affine

        A = ngp_to_sfm_affine(nerf2sfm, testbed._snap.scale, testbed._snap.offset)
        G = A[:, :3]
        V = V.astype(np.float64) @ G.T + A[:, 3]
        N = N.astype(np.float64) @ np.linalg.inv(G)  # the inverse transpose, applied to row vectors
        length = np.linalg.norm(N, axis=1, keepdims=True)
        N = np.where(length > 0, N / np.where(length > 0, length, 1.0), 0.0)
        if np.linalg.det(G) < 0:  # a reflection turns every triangle round
            F = np.ascontiguousarray(F[:, [0, 2, 1]])
        frame = "sfm"
    t0 = time.perf_counter()
    diameter, pair = float("nan"), (-1, -1)
    if len(V):
        d, i, j = max_pairwise_distance(torch.from_numpy(np.ascontiguousarray(V, F32)).to(dev))
        diameter, pair = d, (i, j)
    clock("diameter", t0)
    lo = V.min(axis=0) if len(V) else np.zeros(3)
    size = V.max(axis=0) - lo if len(V) else np.zeros(3)
    return {"V": V, "F": F, "N": N, "C": C, "frame": frame, "n_components": int(n_components), "diameter": diameter,
            "diameter_pair": pair, "bbox": (lo.astype(np.float64), size.astype(np.float64)),
            "invariants": mesh_invariants(V, F), "times": times, "thresh": float(thresh)}


# ---------------------------------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------------------------------
def _colors_u8(C):
    return None if C is None else np.clip(np.rint(np.asarray(C, np.float64) * 255.0), 0, 255).astype(np.uint8)


def write_obj(path, V, F, N=None, C=None) -> None:
    """Wavefront OBJ: ``v x y z [r g b]`` (colours 0..1), ``vn``, 1-based ``f a//a b//b c//c``."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64) + 1
    with open(str(path), "w") as f:
        f.write("# tetrahedral iso-surface of a NeRF density lattice (pixtrack_amd.mesh)\n")
        if C is None:
            f.writelines("v %.9g %.9g %.9g\n" % tuple(v) for v in V)
        else:
            f.writelines("v %.9g %.9g %.9g %.4f %.4f %.4f\n" % (*v, *c) for v, c in zip(V, np.asarray(C, np.float64)))
        if N is not None:
            f.writelines("vn %.6f %.6f %.6f\n" % tuple(n) for n in np.asarray(N, np.float64))
            f.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in F)
        else:
            f.writelines("f %d %d %d\n" % tuple(t) for t in F)


def write_ply(path, V, F, N=None, C=None) -> None:
    """ASCII PLY with optional normals and uchar vertex colours."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    c8 = _colors_u8(C)
    with open(str(path), "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(V)}\nproperty float x\nproperty float y\nproperty float z\n")
        if N is not None:
            f.write("property float nx\nproperty float ny\nproperty float nz\n")
        if c8 is not None:
            f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write(f"element face {len(F)}\nproperty list uchar int vertex_indices\nend_header\n")
        for i, v in enumerate(V):
            row = "%.9g %.9g %.9g" % tuple(v)
            if N is not None:
                row += " %.6f %.6f %.6f" % tuple(N[i])
            if c8 is not None:
                row += " %d %d %d" % tuple(c8[i])
            f.write(row + "\n")
        f.writelines("3 %d %d %d\n" % tuple(t) for t in F)


def write_mesh(path, V, F, N=None, C=None) -> None:
    """OBJ, or PLY when ``path`` ends in ``.ply``."""
    (write_ply if str(path).lower().endswith(".ply") else write_obj)(path, V, F, N, C)


def read_obj(path):
    """``(V [n, 3], F [m, 3] int64 0-based, C [n, 3] or None)`` of an OBJ this module wrote."""
    V, C, F = [], [], []
    with open(str(path)) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                V.append([float(x) for x in w[1:4]])
                if len(w) >= 7:
                    C.append([float(x) for x in w[4:7]])
            elif w[0] == "f":
                F.append([int(x.split("/")[0]) - 1 for x in w[1:4]])
    return (np.asarray(V, np.float64).reshape(-1, 3), np.asarray(F, np.int64).reshape(-1, 3),
            np.asarray(C, np.float64).reshape(-1, 3) if C else None)


def write_points_xyz(path, V) -> None:
    """``x y z`` rows, the form ``evaluation.read_vertices`` reads (YCB's points.xyz)."""
    np.savetxt(str(path), np.asarray(V, np.float64).reshape(-1, 3), fmt="%.10g")


def models_info(V, diameter: float) -> Dict:
    """BOP's models_info.json entry of one object: diameter and bounding box.  No symmetries are invented."""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    lo, size = V.min(axis=0), V.max(axis=0) - V.min(axis=0)
    return {"diameter": float(diameter), "min_x": float(lo[0]), "min_y": float(lo[1]), "min_z": float(lo[2]),
            "size_x": float(size[0]), "size_y": float(size[1]), "size_z": float(size[2])}


def write_models_info(path, V, diameter: float) -> Dict:
    """``models_info.json`` in the one-object form ``symmetry.read_models_info`` reads."""
    info = models_info(V, diameter)
    with open(str(path), "w") as f:
        json.dump(info, f, indent=1)
    return info


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m pixtrack_amd.mesh",
                                 description="mesh.obj, points.xyz and models_info.json of an object from its NeRF")
    ap.add_argument("--object_path", required=True, help="the object's directory (SfM model, nerf2sfm.pkl, NeRF snapshot)")
    ap.add_argument("--obj_aabb", type=str, default="", help="render box [[min], [max]] instead of the one derived from the SfM points")
    ap.add_argument("--resolution", type=int, default=128, help="lattice points per axis")
    ap.add_argument("--thresh", type=float, default=2.5,
                    help="iso value of the density LOGIT (instant-ngp's default number; an untuned starting value here)")
    ap.add_argument("--keep", choices=("largest", "all"), default="largest", help="connected components to keep")
    ap.add_argument("--frame", choices=("sfm", "ngp"), default="sfm", help="coordinates of what is written")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--check_render", type=int, default=0, metavar="N",
                    help="draw the mesh beside the NeRF's Depth render from N views around the box and add the mean "
                         "silhouette IoU and depth error to the JSON line (mesh_evaluation.mesh_nerf_agreement)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    import ast

    args = build_parser().parse_args(argv)
    if not (str(args.device).startswith("cuda") and torch.cuda.is_available()):
        raise _lib.PxtError("mesh extraction runs on a ROCm device; no CPU path exists")
    from .model3d import Model3D
    from .utils.ingp_utils import get_nerf_aabb_from_sfm, initialize_ingp, load_nerf2sfm

    obj = Path(args.object_path)
    model3d = Model3D(str(obj / "pixtrack/aug_nerf_sfm/aug_sfm"))
    nerf2sfm = load_nerf2sfm(str(obj / "pixtrack/pixsfm/dataset/nerf2sfm.pkl"))
    aabb = ast.literal_eval(args.obj_aabb) if args.obj_aabb else get_nerf_aabb_from_sfm(model3d, nerf2sfm)
    testbed = initialize_ingp(str(obj / "pixtrack/instant-ngp/snapshots/weights.msgpack"), aabb, device=args.device)
    mesh = extract_mesh(testbed, args.resolution, args.thresh, keep=args.keep,
                        nerf2sfm=nerf2sfm if args.frame == "sfm" else None)
    if len(mesh["F"]) == 0:
        raise _lib.PxtError(f"the density logit never crosses {args.thresh} inside the box: no surface (try another --thresh)")
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    write_obj(out / "mesh.obj", mesh["V"], mesh["F"], mesh["N"], mesh["C"])
    write_points_xyz(out / "points.xyz", mesh["V"])
    write_models_info(out / "models_info.json", mesh["V"], mesh["diameter"])
    inv = mesh["invariants"]
    summary = {"n_vertices": int(len(mesh["V"])), "n_triangles": int(len(mesh["F"])), "n_components": mesh["n_components"],
               "kept": args.keep, "frame": mesh["frame"], "resolution": int(args.resolution), "thresh": float(args.thresh),
               "invariants": inv, "volume": inv["volume"], "area": inv["area"], "diameter": mesh["diameter"],
               "seconds_lattice": mesh["times"]["lattice"], "seconds_extraction": mesh["times"]["extraction"],
               "seconds_diameter": mesh["times"]["diameter"], "out_dir": str(out)}
    if args.check_render > 0:
        from .mesh_evaluation import mesh_nerf_agreement
        from .ngp import ngp_to_sfm_affine

        V_ngp = mesh["V"]
        if mesh["frame"] == "sfm":  # back into the renderer's frame
            A = ngp_to_sfm_affine(nerf2sfm, testbed._snap.scale, testbed._snap.offset)
            V_ngp = (np.asarray(V_ngp, np.float64) - A[:, 3]) @ np.linalg.inv(A[:, :3]).T
        check = mesh_nerf_agreement(testbed, V_ngp, mesh["F"], n_views=args.check_render)
        summary["check_render"] = {"n_views": check["n_views"], "iou_mean": check["iou_mean"],
                                   "mean_abs_dz_mean": check["mean_abs_dz_mean"]}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
