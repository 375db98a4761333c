"""GPU iso-surface extraction (csrc/pxt_iso.hip) against its numpy restatement, bit for bit; BOP's diameter against
scipy; the NeRF -> lattice -> mesh pipeline on the synthetic snapshot against the CPU oracle; the command line into the
BOP evaluation."""
import json

import numpy as np
import pytest
import torch

from pixtrack_amd import mesh as M
from test_iso_surface_host import closed_and_oriented, exact_hit_lattice, non_finite_lattice, oracle_lattice, sphere

pytestmark = pytest.mark.gpu


def compare(device, values, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """iso_surface == iso_surface_reference: counts, vertex bits, triangle indices; normals within 1e-5."""
    values = np.ascontiguousarray(values, np.float32)
    Vr, Fr, Nr = M.iso_surface_reference(values, iso, origin, spacing, normals=True)
    V, F, N = M.iso_surface(torch.from_numpy(values).to(device), iso, origin, spacing, normals=True)
    V2, F2 = M.iso_surface(torch.from_numpy(values).to(device), iso, origin, spacing)  # without normals: the same mesh
    assert V.dtype == torch.float32 and F.dtype == torch.int32 and V.is_cuda and F.is_cuda
    assert (tuple(V.shape), tuple(F.shape)) == (Vr.shape, Fr.shape), (tuple(V.shape), tuple(F.shape), Vr.shape, Fr.shape)
    assert torch.equal(V, V2) and torch.equal(F, F2)
    V, F, N = V.cpu().numpy(), F.cpu().numpy(), N.cpu().numpy()
    assert np.array_equal(V.view(np.int32), Vr.view(np.int32))
    assert np.array_equal(F, Fr)
    if len(N):
        assert np.abs(N - Nr).max() <= 1e-5  # a handful of 6e-8 roundings on unit-vector components
    return V, F, N


def test_every_single_cell_pattern(device):
    for code in range(1, 255):
        v = np.array([1.0 if (code >> k) & 1 else -1.5 for k in range(8)], np.float32).reshape(2, 2, 2)
        V, F, _ = compare(device, v)
        assert len(F) >= 1, code


@pytest.mark.parametrize("shape,seed", [((11, 10, 9), 0), ((65, 3, 2), 1), ((65, 66, 70), 2)])
def test_noise_lattices(device, shape, seed):
    """nz, ny, nx: extents that are no multiple of any tile; a thin lattice that crosses scan blocks along z; about 3e5
    points and a million vertices: more than one chunk of the second-level scan."""
    v = np.random.default_rng(seed).normal(size=shape).astype(np.float32)
    V, F, _ = compare(device, v)
    assert len(V) > 0 and len(F) > 0
    if shape == (65, 66, 70):
        assert v.size > 256 * 1024 and len(V) > 900_000


def test_lattices_without_cells_or_without_a_surface(device):
    V, F, _ = compare(device, np.random.default_rng(4).normal(size=(5, 5, 1)))  # nx = 1: no cells, no triangles
    assert len(F) == 0 and len(V) > 0
    compare(device, np.random.default_rng(5).normal(size=(1, 1, 7)))
    compare(device, np.zeros((1, 1, 1)) + 1.0)
    for fill in (-1.0, 1.0):
        V, F, _ = compare(device, np.full((9, 10, 11), fill))
        assert len(V) == 0 and len(F) == 0


def test_exact_hits_non_finite_values_and_an_anisotropic_frame(device):
    V, F, _ = compare(device, exact_hit_lattice())
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["euler"] == 2 and inv["zero_area_triangles"] == 108
    V, F, N = compare(device, non_finite_lattice(), 0.25, origin=(1.0, -2.0, 0.5), spacing=(0.5, 0.25, 2.0))
    assert np.isfinite(V).all() and np.isfinite(N).all()
    V, F, _ = compare(device, sphere(24, 8.3), 0.0, origin=(0.37, -11.0, 1e3), spacing=(0.013, 0.7, 3.1))
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["euler"] == 2 and (len(V), len(F)) == (3878, 7752)
    assert inv["volume"] == pytest.approx(2377.80 * 0.013 * 0.7 * 3.1, rel=1e-3)  # 1e3 + x in fp32 costs the rest


def test_the_same_call_twice_gives_the_same_bits(device):
    v = torch.from_numpy(np.random.default_rng(6).normal(size=(33, 31, 40)).astype(np.float32)).to(device)
    a = M.iso_surface(v, 0.1, normals=True)
    b = M.iso_surface(v, 0.1, normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------ the diameter
@pytest.mark.parametrize("n", [1, 2, 257, 5000])
def test_max_pairwise_distance_against_scipy(device, n):
    from scipy.spatial.distance import pdist

    p = (np.random.default_rng(n).normal(size=(n, 3)) * [0.05, 0.2, 0.1] + [0.3, -0.1, 1.0]).astype(np.float32)
    d, i, j = M.max_pairwise_distance(torch.from_numpy(p).to(device))
    if n == 1:
        assert (d, i, j) == (0.0, 0, 0)
        return
    want = float(pdist(p.astype(np.float64)).max())
    pair = float(np.linalg.norm(p[i].astype(np.float64) - p[j].astype(np.float64)))
    assert 0 <= i < j < n
    assert abs(pair - want) <= 1e-6 * want  # three fp32 products, two sums and a square root
    assert abs(d - pair) <= 1e-6 * want


def test_max_pairwise_distance_ties_go_to_the_lowest_pair(device):
    p = (np.random.default_rng(9).uniform(-0.1, 0.1, size=(3000, 3))).astype(np.float32)
    a, b = np.array([-1, 0.5, 0.25], np.float32), np.array([1, -0.5, 0.125], np.float32)
    for k in (2900, 1500, 40):  # the extreme points several times over, across tiles and workgroups
        p[k] = a
    for k in (2950, 1100, 1030, 7):
        p[k] = b
    d, i, j = M.max_pairwise_distance(torch.from_numpy(p).to(device))
    assert (i, j) == (7, 40)
    assert d == np.float32(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)))
    p[[7, 40]] = p[[40, 7]]
    assert M.max_pairwise_distance(torch.from_numpy(p).to(device))[1:] == (7, 40)
    p[7] = 0
    assert M.max_pairwise_distance(torch.from_numpy(p).to(device))[1:] == (40, 1500)


# ------------------------------------------------------------------------------------------- the synthetic NeRF at 24^3
@pytest.fixture(scope="module")
def oracle():
    snap, logit, origin, spacing = oracle_lattice()
    V, F = M.iso_surface_reference(logit, 2.5, origin, spacing)
    return dict(snap=snap, logit=logit, origin=origin, spacing=spacing, V=V, F=F)


@pytest.fixture(scope="module")
def testbed(device, oracle):
    from pixtrack_amd.ngp import Testbed
    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB

    tb = Testbed(device=device)
    tb.load_snapshot(oracle["snap"])
    tb.snap_to_pixel_centers = True
    tb.render_aabb.min, tb.render_aabb.max = PREMIER_PROTEIN_AABB
    return tb


def test_nerf_lattice_and_mesh_against_the_oracle(device, oracle, testbed):
    from scipy.spatial.distance import pdist

    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, shape_value

    values, origin, spacing = M.density_lattice(testbed, 24)
    assert np.array_equal(origin, oracle["origin"]) and np.array_equal(spacing, oracle["spacing"])
    got = values.cpu().numpy()
    # the bar test_ngp_gpu.py holds pxt_ngp_query to; both logits are -inf or far below where the density underflows
    live = np.isfinite(oracle["logit"]) & (oracle["logit"] > -80)
    assert live.mean() > 0.9 and np.abs(got[live] - oracle["logit"][live]).max() < 5e-3
    assert (got[~live] < -60).all()
    # the mesh of the GPU lattice == the restatement on that same lattice
    V, F = M.iso_surface(values, 2.5, origin, spacing)
    Vr, Fr = M.iso_surface_reference(got, 2.5, origin, spacing)
    V, F = V.cpu().numpy(), F.cpu().numpy()
    assert np.array_equal(V.view(np.int32), Vr.view(np.int32)) and np.array_equal(F, Fr)
    inv = M.mesh_invariants(V, F)
    assert closed_and_oriented(inv) and inv["euler"] == 2 and M.triangle_components(len(V), F)[0] == 1
    # where the surface lies: inside the band of the CPU oracle's mesh, widened by 0.002 (a 5e-3 logit error over a slope
    # of 30 logits per unit is 2e-4; this is ten times that)
    band = shape_value(oracle["V"].astype(np.float64), PREMIER_PROTEIN_AABB)
    s = shape_value(V.astype(np.float64), PREMIER_PROTEIN_AABB)
    print("shape_value: oracle mesh", float(band.min()), float(band.max()), "GPU mesh", float(s.min()), float(s.max()))
    assert band.min() - 0.002 <= s.min() and s.max() <= band.max() + 0.002
    # the diameter: within one lattice spacing of the oracle mesh's
    d, i, j = M.max_pairwise_distance(torch.from_numpy(V).to(device))
    want = float(pdist(oracle["V"].astype(np.float64)).max())
    print("diameter", d, "oracle mesh", want)
    assert abs(d - want) <= float(spacing.max())
    assert abs(d - float(pdist(V.astype(np.float64)).max())) <= 1e-6 * want


def test_extract_mesh_frames_and_testbed_methods(device, oracle, testbed, tmp_path):
    from pixtrack_amd.ngp import ngp_to_sfm_affine

    ngp = M.extract_mesh(testbed, 24)
    assert ngp["frame"] == "ngp" and ngp["n_components"] == 1 and closed_and_oriented(ngp["invariants"])
    assert ngp["invariants"]["euler"] == 2 and ngp["invariants"]["volume"] > 0
    assert ngp["V"].shape == ngp["N"].shape == ngp["C"].shape and ngp["F"].dtype == np.int32
    assert np.abs(np.linalg.norm(ngp["N"], axis=1) - 1).max() < 1e-5
    assert (ngp["C"] >= 0).all() and (ngp["C"] <= 1).all() and ngp["C"].std() > 0.01
    lo, size = ngp["bbox"]
    assert np.allclose(lo, ngp["V"].min(axis=0)) and np.allclose(lo + size, ngp["V"].max(axis=0))
    # the normals point out of the object: along the gradient of the procedural shape
    centre = 0.5 * (np.asarray(testbed.render_aabb.min) + np.asarray(testbed.render_aabb.max))
    assert (np.einsum("ij,ij->i", ngp["N"], ngp["V"] - centre) > 0).mean() > 0.99

    nerf2sfm = {"up": np.array([0.0, 0.0, 1.0]), "centroid": np.array([0.1, -0.2, 0.3]), "avglen": 2.5, "totp": np.zeros(3),
                "R": np.eye(4)}
    sfm = M.extract_mesh(testbed, 24, nerf2sfm=nerf2sfm)
    A = ngp_to_sfm_affine(nerf2sfm, testbed._snap.scale, testbed._snap.offset)
    assert sfm["frame"] == "sfm" and np.array_equal(sfm["V"], ngp["V"].astype(np.float64) @ A[:, :3].T + A[:, 3])
    scale = abs(np.linalg.det(A[:, :3])) ** (1.0 / 3.0)
    assert sfm["invariants"]["volume"] == pytest.approx(ngp["invariants"]["volume"] * scale ** 3, rel=1e-6)
    assert sfm["diameter"] == pytest.approx(ngp["diameter"] * scale, rel=1e-5)
    assert closed_and_oriented(sfm["invariants"]) and np.abs(np.linalg.norm(sfm["N"], axis=1) - 1).max() < 1e-9

    m = testbed.compute_marching_cubes_mesh([24, 24, 24])
    assert set(m) == {"V", "N", "C", "F"} and np.array_equal(m["V"], ngp["V"]) and np.array_equal(m["F"], ngp["F"])
    w = testbed.compute_and_save_marching_cubes_mesh(str(tmp_path / "test.obj"), [24, 24, 24])
    V, F, C = M.read_obj(tmp_path / "test.obj")
    assert np.array_equal(V.astype(np.float32), m["V"]) and np.array_equal(F, m["F"]) and np.array_equal(w["F"], m["F"])
    assert np.abs(C - m["C"]).max() <= 5e-5
    testbed.compute_and_save_marching_cubes_mesh(str(tmp_path / "test.ply"), [24, 24, 24])
    assert f"element face {len(F)}" in (tmp_path / "test.ply").read_text().splitlines()
    anis = testbed.compute_marching_cubes_mesh([20, 24, 28], thresh=0.0)  # nx, ny, nz
    assert len(anis["F"]) > 0 and closed_and_oriented(M.mesh_invariants(anis["V"], anis["F"]))


def test_command_line_feeds_the_bop_evaluation(device, tmp_path, capsys):
    from pixtrack_amd.evaluation import evaluate_poses_bop, read_vertices
    from pixtrack_amd.geometry import Camera, Pose
    from pixtrack_amd.symmetry import read_models_info
    from pixtrack_amd.synthetic import make_tracking_assets, perturb_pose, write_object_dir

    assets = make_tracking_assets(width=160, height=120, n_frames=2)
    obj, out = tmp_path / "object", tmp_path / "model"
    write_object_dir(assets, obj)
    aabb = json.dumps([[float(x) for x in corner] for corner in assets["aabb"]])
    summary = M.main(["--object_path", str(obj), "--obj_aabb", aabb, "--resolution", "32", "--out_dir", str(out),
                      "--device", str(device)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(summary)) and line["frame"] == "sfm"
    assert line["n_components"] == 1 and line["invariants"]["euler"] == 2 and line["volume"] > 0
    assert line["invariants"]["directed_edges_unpaired"] == 0 and line["invariants"]["directed_edges_repeated"] == 0
    assert min(line["seconds_lattice"], line["seconds_extraction"], line["seconds_diameter"]) > 0
    vertices = read_vertices(out / "points.xyz")
    info = read_models_info(out / "models_info.json")
    V, F, C = M.read_obj(out / "mesh.obj")
    assert len(vertices) == line["n_vertices"] == len(V) and len(F) == line["n_triangles"] and C is not None
    assert info["diameter"] == line["diameter"]
    # the object is the synthetic super-ellipsoid in SfM units: the mesh lies about the SfM points
    pts = np.stack([p.xyz for p in assets["model3d"].points3D.values()])
    assert np.abs(vertices.min(axis=0) - pts.min(axis=0)).max() < 0.05 * info["diameter"]
    assert np.abs(vertices.max(axis=0) - pts.max(axis=0)).max() < 0.05 * info["diameter"]

    cam = Camera.from_colmap(assets["query_camera"])
    rng = np.random.default_rng(0)
    poses = {}
    for k, (Rg, tg) in enumerate(assets["gt_poses"]):
        Re, te = perturb_pose(Rg, tg, rng, 1.0, 0.01, assets["center"])
        poses[f"{k:06d}.png"] = {"success": True, "camera": cam,
                                 "gt_pose": Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg)),
                                 "T_refined": Pose.from_Rt(torch.from_numpy(Re), torch.from_numpy(te))}
    res = evaluate_poses_bop(poses, vertices, device, info["diameter"])
    assert res["n_evaluated"] == 2 and res["diameter"] == info["diameter"]
    assert 0 < res["mssd_mean"] < 0.2 * info["diameter"] and 0 < res["mspd_mean"] < np.inf
    assert 0 <= res["ar_mssd"] <= 1 and 0 <= res["ar_mspd"] <= 1
