"""The iso-surface rule on the CPU: mesh.iso_surface_reference (the numpy restatement the GPU path is held to bit for
bit in test_iso_surface_gpu.py) on lattices with known answers, the mesh invariants, the native case table against the
Python one, the writers against the evaluation's readers, and the argument refusals.  No GPU."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, mesh as M


def sphere(n, r, c=None, shape=None):
    shape = (n, n, n) if shape is None else shape
    c = [(n - 1) / 2.0] * 3 if c is None else c
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def closed_and_oriented(inv):
    return inv["directed_edges_repeated"] == 0 and inv["directed_edges_unpaired"] == 0


def exact_hit_lattice():
    i = np.indices((12, 12, 12)).astype(np.float64)
    return (16.0 - ((i - 5.0) ** 2).sum(axis=0)).astype(np.float32)  # zero exactly at lattice points


def non_finite_lattice():
    v = np.random.default_rng(3).normal(size=(7, 8, 9)).astype(np.float32)
    v[1, 2, 3], v[2, 2, 3], v[3, 3, 3] = np.nan, np.inf, -np.inf
    v[4, 4, 4], v[4, 4, 5], v[5, 1, 1], v[5, 1, 2] = np.inf, -np.inf, np.nan, np.nan
    return v


@pytest.mark.parametrize("n,r,nv,nf", [(12, 4.0, 914, 1824), (24, 8.3, 3878, 7752)])
def test_sphere_counts_and_topology(n, r, nv, nf):
    V, F = M.iso_surface_reference(sphere(n, r), 0.0)
    inv = M.mesh_invariants(V, F)
    assert (len(V), len(F)) == (nv, nf) and V.dtype == np.float32 and F.dtype == np.int32
    assert closed_and_oriented(inv) and inv["euler"] == 2 and inv["volume"] > 0 and inv["unreferenced_vertices"] == 0
    assert inv["zero_area_triangles"] == 0


def test_sphere_lies_inside_the_analytic_sphere():
    """r - |p - c| is concave along any line: the chord's zero lies inside the sphere, so the mesh is inscribed."""
    r = 8.3
    V, F = M.iso_surface_reference(sphere(24, r), 0.0)
    inv = M.mesh_invariants(V, F)
    vol, area = 4.0 / 3.0 * np.pi * r ** 3, 4.0 * np.pi * r ** 2
    dv, da = (vol - inv["volume"]) / vol, (area - inv["area"]) / area
    print(f"volume {inv['volume']:.2f} of {vol:.2f} (deficit {dv:.4%}), area {inv['area']:.2f} of {area:.2f} ({da:.4%})")
    assert inv["volume"] == pytest.approx(2377.80, abs=0.01) and inv["area"] == pytest.approx(862.48, abs=0.01)
    assert 0 < dv < 0.015 and 0 < da < 0.008
    assert (np.linalg.norm(V.astype(np.float64) - 11.5, axis=1) <= r + 1e-5).all()


def test_torus_and_two_spheres():
    z, y, x = np.meshgrid(*[np.arange(24, dtype=np.float64) - 11.5] * 3, indexing="ij")
    torus = (2.5 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 7.0) ** 2 + z ** 2)).astype(np.float32)
    V, F = M.iso_surface_reference(torus, 0.0)
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["euler"] == 0 and inv["volume"] > 0 and inv["unreferenced_vertices"] == 0
    two = np.maximum(sphere(0, 4.0, (6, 6, 6), (14, 14, 28)), sphere(0, 4.5, (20, 7, 7), (14, 14, 28)))
    V, F = M.iso_surface_reference(two, 0.0)
    inv = M.mesh_invariants(V, F)
    n_comp, labels = M.triangle_components(len(V), F)
    assert closed_and_oriented(inv) and inv["euler"] == 4 and n_comp == 2 and inv["volume"] > 0
    (V1,), F1 = M.keep_triangles([V], F, labels == np.argmax(np.bincount(labels)))
    inv1 = M.mesh_invariants(V1, F1)
    assert closed_and_oriented(inv1) and inv1["euler"] == 2 and inv1["unreferenced_vertices"] == 0
    assert inv1["volume"] == pytest.approx(4.0 / 3.0 * np.pi * 4.5 ** 3, rel=0.05)  # the larger sphere


def test_noise_closes_only_with_a_border():
    a = np.random.default_rng(0).normal(size=(11, 10, 9)).astype(np.float32)  # nz, ny, nx: a 9 x 10 x 11 lattice
    V, F = M.iso_surface_reference(a, 0.0)
    assert M.mesh_invariants(V, F)["directed_edges_unpaired"] > 0  # the check can fail
    b = a.copy()
    b[0] = b[-1] = b[:, 0] = b[:, -1] = -1
    b[:, :, 0] = b[:, :, -1] = -1
    V, F, N = M.iso_surface_reference(b, 0.0, normals=True)
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["volume"] > 0 and inv["unreferenced_vertices"] == 0
    assert np.abs(np.linalg.norm(N, axis=1) - 1).max() < 1e-6


def test_normals_point_out_of_a_sphere():
    c = (7.3, 7.6, 7.1)
    V, F, N = M.iso_surface_reference(sphere(16, 6.0, c), 0.0, normals=True)
    radial = V.astype(np.float64) - np.asarray(c)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert np.einsum("ij,ij->i", radial, N).min() > 0.999  # the gradient of r - |p - c| is the inward unit radius
    # and the triangles are wound the same way: every face normal points outwards
    p = V.astype(np.float64)
    fn = np.cross(p[F[:, 1]] - p[F[:, 0]], p[F[:, 2]] - p[F[:, 0]])
    assert (np.einsum("ij,ij->i", fn, p[F].mean(axis=1) - np.asarray(c)) > 0).all()


def test_exact_hits_stay_closed_and_report_their_zero_area_triangles():
    V, F = M.iso_surface_reference(exact_hit_lattice(), 0.0)
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["euler"] == 2
    assert inv["zero_area_triangles"] == 108  # reported, not removed


def test_non_finite_values_follow_the_rule():
    v = non_finite_lattice()
    V, F, N = M.iso_surface_reference(v, 0.25, origin=(1.0, -2.0, 0.5), spacing=(0.5, 0.25, 2.0), normals=True)
    assert np.isfinite(V).all() and np.isfinite(N).all() and len(F) > 0
    # the NaN and -inf points are outside, +inf inside: every edge between a finite point below iso and them has no vertex
    inside = np.nan_to_num(v, nan=-1.0) >= 0.25
    n_edges = sum(int((inside[:7 - dz, :8 - dy, :9 - dx] != inside[dz:, dy:, dx:]).sum()) for dx, dy, dz in M.EDGE_DIRS)
    assert len(V) == n_edges
    # an edge with a NaN or two infinite ends puts its vertex at the middle: (4, 4, 4) = +inf next to (5, 4, 4) = -inf
    mid = np.array([1.0 + 4.5 * 0.5, -2.0 + 4 * 0.25, 0.5 + 4 * 2.0], np.float32)
    assert (V == mid).all(axis=1).any()


def test_single_cell_patterns_and_flat_lattices():
    for code in range(1, 255):
        v = np.array([1.0 if (code >> k) & 1 else -1.0 for k in range(8)], np.float32).reshape(2, 2, 2)
        V, F = M.iso_surface_reference(v, 0.0)
        inv = M.mesh_invariants(V, F)
        assert len(F) >= 1 and inv["directed_edges_repeated"] == 0 and inv["unreferenced_vertices"] == 0, code
    V, F = M.iso_surface_reference(np.random.default_rng(1).normal(size=(5, 5, 1)).astype(np.float32), 0.0)
    assert len(F) == 0 and F.shape == (0, 3) and len(V) > 0  # no cells: edges carry vertices, nothing joins them
    for fill in (-1.0, 1.0):
        V, F = M.iso_surface_reference(np.full((3, 4, 5), fill, np.float32), 0.0)
        assert len(V) == 0 and len(F) == 0


def test_native_case_table_equals_the_python_table():
    mine, native = M.case_table(), M.native_case_table()
    assert mine.shape == native.shape == (6, 16, 7)
    for t in range(6):
        for code in range(16):
            assert mine[t, code].tolist() == native[t, code].tolist(), (t, code)
    pc = np.array([bin(c).count("1") for c in range(16)])
    assert (native[:, :, 0] == np.where(pc == 2, 2, np.where((pc == 1) | (pc == 3), 1, 0))[None]).all()


def test_abi_and_argument_refusals():
    L = _lib.lib()
    assert _lib.ABI_VERSION == 13 and L.pxt_version() == 13
    assert int(L.pxt_iso_surface_workspace_bytes(128, 128, 128)) >= 4 * 128 ** 3
    assert int(L.pxt_iso_surface_workspace_bytes(1, 5, 5)) > 0  # no cells, still valid
    assert int(L.pxt_iso_surface_workspace_bytes(0, 5, 5)) == -1
    assert int(L.pxt_iso_surface_workspace_bytes(512, 512, 512)) > 0  # 2^27 exactly
    assert int(L.pxt_iso_surface_workspace_bytes(513, 512, 512)) == -1
    assert int(L.pxt_max_pairwise_distance_workspace_bytes(0)) == -1
    assert int(L.pxt_max_pairwise_distance_workspace_bytes((1 << 22) + 1)) == -1
    assert int(L.pxt_max_pairwise_distance_workspace_bytes(1)) > 0
    assert L.pxt_iso_case_table(None) == -1
    # refused before any launch: null pointers, bad extents (nothing dereferenced, no device needed)
    g = _lib.IsoGrid(0, 4, 4, 0.0, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
    assert L.pxt_iso_surface_count(16, C.byref(g), 16, 16, None) == -1
    g.nx = 4
    assert L.pxt_iso_surface_count(None, C.byref(g), 16, 16, None) == -1
    assert L.pxt_iso_surface_count(16, C.byref(g), 20, 16, None) == -1  # workspace not 16-byte aligned
    assert L.pxt_iso_surface_emit(16, C.byref(g), 16, None, 3, None, 16, 1, None) == -1
    assert L.pxt_iso_surface_emit(16, C.byref(g), 16, 16, -1, None, 16, 1, None) == -1
    assert L.pxt_max_pairwise_distance(None, 4, 16, 16, None) == -1
    assert L.pxt_max_pairwise_distance(16, 0, 16, 16, None) == -1
    # the Python layer refuses host tensors: there is no CPU path
    with pytest.raises(_lib.PxtError):
        M.iso_surface(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(_lib.PxtError):
        M.max_pairwise_distance(torch.zeros(4, 3))
    from pixtrack_amd import ops

    for name in ("iso_surface_count", "iso_surface_emit", "max_pairwise_distance", "ngp_query"):
        assert name in ops.op_names()
    with pytest.raises(NotImplementedError):
        torch.ops.pixtrack.max_pairwise_distance(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32),
                                                 torch.zeros(64, dtype=torch.uint8))


def test_writers_round_trip_through_the_evaluation_readers(tmp_path):
    from pixtrack_amd.evaluation import read_vertices
    from pixtrack_amd.symmetry import read_models_info

    V, F, N = M.iso_surface_reference(sphere(12, 4.0), 0.0, origin=(0.1, 0.2, 0.3), spacing=(0.01, 0.02, 0.03), normals=True)
    Cc = np.random.default_rng(2).uniform(size=V.shape)
    M.write_points_xyz(tmp_path / "points.xyz", V)
    got = read_vertices(tmp_path / "points.xyz")
    assert got.shape == V.shape and np.allclose(got, V.astype(np.float64), rtol=1e-9, atol=0)
    info = M.write_models_info(tmp_path / "models_info.json", V, 0.123456789)
    back = read_models_info(tmp_path / "models_info.json")
    assert back["diameter"] == 0.123456789 and back["symmetries"].shape == (1, 4, 4)
    assert set(info) == {"diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"}
    raw = json.loads((tmp_path / "models_info.json").read_text())
    assert np.allclose([raw["min_x"] + raw["size_x"], raw["min_y"] + raw["size_y"], raw["min_z"] + raw["size_z"]],
                       V.max(axis=0).astype(np.float64))
    M.write_mesh(tmp_path / "m.obj", V, F, N, Cc)
    V2, F2, C2 = M.read_obj(tmp_path / "m.obj")
    assert np.array_equal(V2.astype(np.float32), V) and np.array_equal(F2, F) and np.abs(C2 - Cc).max() <= 5e-5
    M.write_mesh(tmp_path / "m.ply", V, F, N, Cc)
    head = (tmp_path / "m.ply").read_text().splitlines()
    assert head[0] == "ply" and f"element vertex {len(V)}" in head and f"element face {len(F)}" in head
    assert len(head) == head.index("end_header") + 1 + len(V) + len(F)


def oracle_lattice(n=24, pad=0.05):
    """The synthetic NeRF's density logit on an n^3 lattice over the default box, from the CPU oracle."""
    from oracle import ngp_oracle as NO
    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, make_synthetic_nerf

    snap = make_synthetic_nerf()
    model = NO.NgpModel(grid=snap.grid, mlp=snap.mlp_dict(), occupancy=snap.occupancy, cascades=snap.cascades,
                        aabb_scale=snap.aabb_scale, cone_angle=snap.cone_angle, depth_scale=1.0 / snap.scale,
                        linear_colors=snap.linear_colors)
    shape, origin, spacing = M.lattice_frame(n, *PREMIER_PROTEIN_AABB, pad)
    pts = M.lattice_points_host(shape, origin, spacing)
    unit = ((pts - np.float32(0.5 - snap.aabb_scale / 2)) * np.float32(1.0 / snap.aabb_scale)).astype(np.float32)
    dirs = np.tile(np.asarray(M.QUERY_DIR, np.float32), (len(pts), 1))
    with np.errstate(divide="ignore"):
        density, _ = NO.network(model, unit, dirs)
        logit = np.log(density).astype(np.float32)
    return snap, logit.reshape(shape), origin, spacing


def test_end_to_end_on_the_cpu_oracle():
    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, shape_value

    _, logit, origin, spacing = oracle_lattice()
    V, F = M.iso_surface_reference(logit, 2.5, origin, spacing)
    inv = M.mesh_invariants(V, F)
    n_comp, _ = M.triangle_components(len(V), F)
    assert closed_and_oriented(inv) and inv["euler"] == 2 and n_comp == 1 and inv["volume"] > 0
    assert (len(V), len(F)) == (5328, 10652)
    s = shape_value(V.astype(np.float64), PREMIER_PROTEIN_AABB)
    print("shape_value at the vertices:", float(s.min()), float(s.max()))
    # the band's width is the synthetic snapshot's own 56^3 indicator grid, not the extractor
    assert 0.0769 - 5e-4 <= s.min() and s.max() <= 0.1784 + 5e-4
