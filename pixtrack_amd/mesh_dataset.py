"""A reference model from a coloured or textured mesh: mapping images and a COLMAP model with tracks, no SuperPoint /
SuperGlue / COLMAP involved.

The reference starts a YCB / BOP object from its mesh (``scripts/create_sfm_from_obj.py``): ambient-lit colour renders
from look-at views on an icosphere become the ``mapping/`` images, and their cameras and poses the SfM model the tracker
loads.  Here the renders come from ``MeshRenderer.render`` (pxt_mesh_render for vertex colours, pxt_mesh_render_textured
for a texture map as YCB's ``textured.obj`` and BOP's ``texture_u`` PLYs carry one), the views from
``mesh_render.look_at_views``, and the 3-D points are mesh vertices with exact tracks: a vertex is observed in a view
when its float64 projection (``Camera`` convention), rounded to the nearest pixel, lies inside the image, the render's
id plane holds a triangle there, and that triangle has the vertex as a corner.  Integer ids, no tolerance.

    python -m pixtrack_amd.mesh_dataset --mesh FILE [--texture FILE] [--mesh_scale S] --out_dir D
           [--width 3072 --height 3072 --focal 2700 --cx 1536 --cy 1536]
           [--subdivisions 2] [--max_points 8192] [--min_track 3] [--views_per_call 8] [--device cuda:0]

writes ``D/dataset/mapping/0001.png ...`` and ``D/ref/{cameras,images,points3D}.bin`` and prints one JSON line.  The
defaults are the reference's numbers (``create_sfm_from_obj.py:154-159``); ``cx, cy`` are in COLMAP's convention (the
render goes through ``Camera.from_colmap``: pixel centres at integers, ``cx - 0.5``).

This is the SfM half of an object directory.  ``nerf2sfm.pkl``, a NeRF snapshot and the ``aug_sfm`` augmentation are not
produced; the tracker's mesh template (``--template mesh --mesh FILE --reference_sfm D/ref``, ``mesh_template.py``) needs
none of them.  A mesh with vertex colours is drawn with them (``mesh_render.read_mesh_colors``); one without is drawn with
its texture map (``mesh_render.read_mesh_textured``; ``--texture`` names another image for the same UVs); one with
neither is refused.
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import _lib
from . import mesh_render as R
from .geometry import Camera
from .utils.colmap import ColmapCamera, ColmapImage, ColmapPoint3D, rotmat2qvec, write_model_binary

Renderer = Callable[[np.ndarray, int, int], Dict[str, np.ndarray]]


def image_name(k: int) -> str:
    """The file name of image ``k`` (1-based), as the reference writes it."""
    return ("%d.png" % k).zfill(8)


def reference_renderer(V, F, C=None, uvs=None, triangle_uvs=None, texture=None) -> Renderer:
    """The numpy restatement as a renderer (for tests; seconds per small view): vertex colours ``C``, or ``uvs``,
    ``triangle_uvs`` and ``texture``."""
    def render(views, width, height):
        if C is not None:
            out = R.shade_reference(V, F, C, views, width, height)
        else:
            out = R.shade_textured_reference(V, F, uvs, F if triangle_uvs is None else triangle_uvs, texture, views,
                                             width, height)
        return {"rgb_u8": out[1], "ids": out[4]}
    return render


def gpu_renderer(V, F, C, device, uvs=None, triangle_uvs=None, texture=None) -> Renderer:
    mr = R.MeshRenderer(V, F, device, colors=C, uvs=uvs, triangle_uvs=triangle_uvs, texture=texture)

    def render(views, width, height):
        out = mr.render(views, width, height, want=("rgb_u8", "ids"), download_records=False)
        return {"rgb_u8": out["rgb_u8"].cpu().numpy(), "ids": out["ids"].cpu().numpy()}
    return render


def observed_vertices(points, ids, pose, fx, fy, cx, cy):
    """One view's part of the observation rule: ``points`` [n, 3] float64 projected through ``pose`` (4x4) in the
    Camera convention and looked up in the id plane ``ids`` [H, W] -> (lands on a triangle [n], that triangle [n], the
    projections xy [n, 2]).  Whether the triangle has the point as a corner is the caller's part."""
    p = points @ pose[:3, :3].T + pose[:3, 3]
    H, W = ids.shape
    with np.errstate(all="ignore"):
        xy = np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], 1)
    ok = (p[:, 2] > 0) & np.isfinite(xy).all(1)
    ij = np.rint(np.where(ok[:, None], xy, -1.0)).astype(np.int64)
    ok &= (ij[:, 0] >= 0) & (ij[:, 0] < W) & (ij[:, 1] >= 0) & (ij[:, 1] < H)
    tri = np.where(ok, ids[np.clip(ij[:, 1], 0, H - 1), np.clip(ij[:, 0], 0, W - 1)], -1)
    return ok & (tri >= 0), tri, xy


def vertex_texels(n: int, F, uvs, triangle_uvs, texture) -> np.ndarray:
    """The colour of each of ``n`` vertices as a 3-D point: the texture's nearest texel (the render's addressing: row 0
    is v = 1, corners aligned, the border clamped) at the vertex's first UV, the one of its first corner in ``F``'s
    order.  A vertex no triangle uses is black.  -> int64 [n, 3]."""
    Ht, Wt = texture.shape[:2]
    corner = np.full(n, -1, np.int64)
    flat_v, flat_uv = F.reshape(-1), triangle_uvs.reshape(-1)
    first = np.unique(flat_v, return_index=True)
    corner[first[0]] = flat_uv[first[1]]
    uv = uvs[np.clip(corner, 0, len(uvs) - 1)]
    i = np.rint(np.clip(uv[:, 0] * (Wt - 1), 0, Wt - 1)).astype(np.int64)
    j = np.rint(np.clip((1.0 - uv[:, 1]) * (Ht - 1), 0, Ht - 1)).astype(np.int64)
    return np.where((corner >= 0)[:, None], texture[j, i, :3].astype(np.int64), 0)


def build_reference_from_mesh(V, F, C, out_dir, width: int = 3072, height: int = 3072, focal: float = 2700.0,
                              cx: float = 1536.0, cy: float = 1536.0, subdivisions: int = 2, max_points: int = 8192,
                              min_track: int = 3, views_per_call: int = 8, device="cuda:0",
                              renderer: Optional[Renderer] = None, uvs=None, triangle_uvs=None, texture=None) -> Dict:
    """Writes ``out_dir/dataset/mapping/*.png`` and ``out_dir/ref/*.bin`` for the mesh ``V, F`` with vertex colours ``C``
    (0..1) - or, with ``C`` None, with the texture map ``texture`` (uint8 [Ht, Wt, 3 or 4]) read through ``uvs`` [n, 2]
    and ``triangle_uvs`` [m, 3] (default ``F``); a 3-D point then takes the nearest texel at its vertex's first UV - and
    returns the summary.  ``renderer(views [P, 20], width, height) -> {"rgb_u8": uint8 [P, H, W, 3], "ids": int32 [P, H,
    W]}`` (host arrays) replaces the GPU ``MeshRenderer``; ``reference_renderer`` is the numpy one."""
    from PIL import Image

    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    W, H = int(width), int(height)
    if C is not None:
        if uvs is not None or texture is not None:
            raise ValueError("vertex colours or a texture map, not both")
        C = np.asarray(C, np.float64).reshape(-1, 3)
        if len(C) != len(V):
            raise ValueError(f"{len(C)} colours for {len(V)} vertices")
        rgb = np.clip(np.rint(C * 255.0), 0, 255).astype(np.int64)
    else:
        if uvs is None or texture is None:
            raise ValueError("a mesh without vertex colours needs uvs and texture")
        uvs = np.asarray(uvs, np.float64).reshape(-1, 2)
        triangle_uvs = F if triangle_uvs is None else np.asarray(triangle_uvs, np.int64).reshape(-1, 3)
        if triangle_uvs.shape != F.shape or triangle_uvs.min() < 0 or triangle_uvs.max() >= len(uvs):
            raise ValueError(f"triangle_uvs {triangle_uvs.shape} does not index the {len(uvs)} uvs for {F.shape} triangles")
        rgb = vertex_texels(len(V), F, uvs, triangle_uvs, R.texture_rgb(texture))
    if min(max_points, min_track, views_per_call) < 1:
        raise ValueError("max_points, min_track and views_per_call are at least 1")
    out = Path(out_dir)
    mapping = out / "dataset" / "mapping"
    mapping.mkdir(parents=True, exist_ok=True)
    colmap_cam = ColmapCamera(1, "SIMPLE_RADIAL", W, H, np.asarray([focal, cx, cy, 0.0], np.float64))
    cam = Camera.from_colmap(colmap_cam)._data.double().numpy()
    fx, fy, cxp, cyp = (float(x) for x in cam[2:6])
    views, poses = R.look_at_views(V, fx, fy, cxp, cyp, W, H, subdivisions)
    if renderer is None:
        renderer = gpu_renderer(V, F, C, device, uvs, triangle_uvs, texture)

    n = len(V)
    sel = np.arange(n) if n <= max_points else np.unique((np.arange(max_points) * (n / max_points)).astype(np.int64))
    points = V[sel]
    seen, t_render, t_write = [], 0.0, 0.0  # per view: (indices into sel, xy)
    for k0 in range(0, len(views), views_per_call):
        t0 = time.perf_counter()
        got = renderer(views[k0:k0 + views_per_call], W, H)
        t_render += time.perf_counter() - t0
        for q in range(len(got["rgb_u8"])):
            k = k0 + q
            t0 = time.perf_counter()
            Image.fromarray(np.ascontiguousarray(got["rgb_u8"][q])).save(str(mapping / image_name(k + 1)))
            t_write += time.perf_counter() - t0
            hit, tri, xy = observed_vertices(points, got["ids"][q], poses[k], fx, fy, cxp, cyp)
            corner = (F[np.clip(tri, 0, len(F) - 1)] == sel[:, None]).any(1)
            obs = np.nonzero(hit & corner)[0]
            seen.append((obs, xy[obs]))

    track = np.zeros(len(sel), np.int64)
    for obs, _ in seen:
        track[obs] += 1
    keep = track >= min_track
    images, tracks = {}, {int(i): ([], []) for i in np.nonzero(keep)[0]}
    for k, (obs, xy) in enumerate(seen):
        m = keep[obs]
        obs, xy = obs[m], xy[m] + 0.5  # COLMAP's convention
        for idx2d, i in enumerate(obs):
            tracks[int(i)][0].append(k + 1)
            tracks[int(i)][1].append(idx2d)
        images[k + 1] = ColmapImage(k + 1, rotmat2qvec(poses[k][:3, :3]), poses[k][:3, 3].copy(), 1,
                                    "mapping/" + image_name(k + 1), xy.reshape(-1, 2), (sel[obs] + 1).astype(np.int64))
    points3D = {int(sel[i]) + 1: ColmapPoint3D(int(sel[i]) + 1, points[i].copy(), rgb[sel[i]], 0.0,
                                              np.asarray(tr[0], np.int64), np.asarray(tr[1], np.int64))
                for i, tr in tracks.items()}
    t0 = time.perf_counter()
    write_model_binary(out / "ref", {1: colmap_cam}, images, points3D)
    t_write += time.perf_counter() - t0
    per_image = [len(im.point3D_ids) for im in images.values()]
    kept = track[keep]
    return {"views": int(len(views)), "width": W, "height": H, "vertices": int(n), "triangles": int(len(F)),
            "points": int(keep.sum()), "track_min": int(kept.min()) if len(kept) else 0,
            "track_mean": float(kept.mean()) if len(kept) else 0.0, "points_per_image_min": int(min(per_image)),
            "points_per_image_mean": float(np.mean(per_image)), "render_seconds": t_render, "write_seconds": t_write,
            "out_dir": str(out)}


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="PLY with vertex red green blue, OBJ with v x y z r g b, or a textured "
                    "OBJ (vt, mtllib, usemtl -> map_Kd) / PLY (texture_u texture_v, comment TextureFile)")
    ap.add_argument("--texture", default=None, help="the texture map of a textured mesh, in place of the one it names")
    ap.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the vertices (BOP's models are in mm)")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--width", type=int, default=3072)
    ap.add_argument("--height", type=int, default=3072)
    ap.add_argument("--focal", type=float, default=2700.0)
    ap.add_argument("--cx", type=float, default=1536.0, help="COLMAP convention")
    ap.add_argument("--cy", type=float, default=1536.0)
    ap.add_argument("--subdivisions", type=int, default=2, help="of the icosphere of view directions: 12 / 42 / 162 views")
    ap.add_argument("--max_points", type=int, default=8192, help="vertices taken as 3-D points (an evenly strided subset)")
    ap.add_argument("--min_track", type=int, default=3, help="views a point must be observed in to be kept")
    ap.add_argument("--views_per_call", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    args = build_parser().parse_args(argv)
    V, F, C = R.read_mesh_colors(args.mesh)
    textured = {}
    if C is None:
        mesh = R.read_mesh_textured(args.mesh, require_image=args.texture is None)
        if mesh is None:
            raise _lib.PxtError(f"{args.mesh} has no vertex colours and no texture coordinates")
        V, F, uvs, triangle_uvs, image = mesh
        textured = dict(uvs=uvs, triangle_uvs=triangle_uvs, texture=R.read_texture(args.texture or image))
    elif args.texture:
        raise _lib.PxtError(f"{args.mesh} has vertex colours; --texture goes with a mesh that has texture coordinates")
    summary = build_reference_from_mesh(V * args.mesh_scale, F, C, args.out_dir, args.width, args.height, args.focal,
                                        args.cx, args.cy, args.subdivisions, args.max_points, args.min_track,
                                        args.views_per_call, args.device, **textured)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
