"""The HIP NeRF renderer and point query against the numpy oracle on every snapshot geometry the loader can hand them -
aabb_scale 1 (one cascade, constant step), 2, 16 (five cascades, a hashed level 1), integer level scales - and on view
settings off their usual values, at tests/test_ngp_gpu.py's tolerances.  tests/test_ngp_geometries_host.py holds the cases
and shows, from the oracle alone, that each reaches what it is there for."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ngp_oracle as NO
from pixtrack_amd.ngp import NerfSnapshot, RenderMode, Testbed
from pixtrack_amd.synthetic import NERF_VARIANT_CASES, nerf_variant_camera
from test_ngp_geometries_host import (ALL_CASES, QUERY_MODELS, SETTINGS_CASES, TRANSPARENT, case_snapshot, model_snapshot,
                                      oracle_case, oracle_case_depth, oracle_model, query_points)

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def case_testbed(case, device):
    W, _ = case["size"]
    tb = Testbed(device=device)
    tb.load_snapshot(case_snapshot(case))
    tb.background_color = list(case.get("background", TRANSPARENT))
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = case.get("min_transmittance", 1e-7)
    tb.fov_axis = 0
    tb.render_aabb.min, tb.render_aabb.max = [list(map(float, b)) for b in case["box"]]
    tb._cam_ngp = nerf_variant_camera(case)
    tb.fov = math.degrees(2 * math.atan(W / (2 * 1.2 * W)))
    return tb


def check_case(name, device):
    """render_both_device (one march, the production path) against the oracle's Shade and Depth renders at
    tests/test_ngp_gpu.py's bars; the single-mode renders equal its outputs bit for bit."""
    case = ALL_CASES[name]
    (W, H), spp = case["size"], case["spp"]
    o = oracle_case(name)
    refs = {"shade": o["shade"], "depth": oracle_case_depth(name)}
    st = o["stats"]
    tb = case_testbed(case, device)
    tb.stats_accum = torch.zeros(4, dtype=torch.int64, device=device)
    rgba, depth = tb.render_both_device(W, H, spp)
    stats = tb.stats_accum.cpu().tolist()
    tb.stats_accum = None
    tb.render_mode = RenderMode.Shade
    assert torch.equal(tb.render_device(W, H, spp, True), rgba)
    tb.render_mode = RenderMode.Depth
    assert torch.equal(tb.render_device(W, H, spp, True), depth)
    outs = {"shade": rgba.cpu().numpy(), "depth": depth.cpu().numpy()}
    figures = {}
    for k, out in outs.items():
        ref = refs[k]
        assert out.shape == (H, W, 4) and np.isfinite(out).all()
        diff = np.abs(out - ref) / max(1.0, float(np.abs(ref[..., :3]).max()))
        figures[k] = (float(diff.max()), float(diff.mean()))
    print("CASE", name, "rays_hit", stats[1], st["rays_hit"], "samples", stats[0], st["samples"],
          " ".join("%s max %.3e mean %.3e" % ((k,) + v) for k, v in figures.items()))
    assert stats[1] == st["rays_hit"]
    assert abs(stats[0] - st["samples"]) <= max(4, st["samples"] // 2000)
    for k, (dmax, dmean) in figures.items():
        assert dmax < 1e-2, (k, dmax)
        assert dmean < 5e-4, (k, dmean)
    assert float(outs["depth"][..., 0].max()) > 0


@pytest.mark.parametrize("name", list(NERF_VARIANT_CASES))
def test_render_matches_oracle_on_geometry(device, name):
    check_case(name, device)


@pytest.mark.parametrize("name", list(SETTINGS_CASES))
def test_render_matches_oracle_with_setting(device, name):
    check_case(name, device)


@pytest.mark.parametrize("name", QUERY_MODELS)
def test_network_query_matches_oracle_over_the_scene_cube(device, name):
    """pxt_ngp_query at points of the WHOLE scene cube, its upper faces included (where a dense level's corner index passes
    the level's size and wraps, tiny-cuda-nn's `% size`); dense random MLP weights as in tests/test_ngp_gpu.py."""
    from pixtrack_amd import _lib

    snap = model_snapshot(name)
    rg = np.random.default_rng(5)
    shapes = dict(d1=(64, 32), d2=(16, 64), c1=(64, 32), c2=(64, 64), c3=(16, 64))
    rnd = {k: (rg.normal(size=v) * (2.0 / v[1]) ** 0.5).astype(np.float16) for k, v in shapes.items()}
    s2 = NerfSnapshot(grid=snap.grid, mlp=np.concatenate([rnd[k].ravel() for k in ("d1", "d2", "c1", "c2", "c3")]),
                      occupancy=snap.occupancy, log2_hashmap=snap.log2_hashmap, base_res=snap.base_res,
                      per_level_scale=snap.per_level_scale, cascades=snap.cascades, aabb_scale=snap.aabb_scale,
                      cone_angle=snap.cone_angle)
    x, d, unit = query_points(snap.aabb_scale)
    n = x.shape[0]
    tb = Testbed(device=device)
    tb.load_snapshot(s2)
    out = torch.zeros(n, 4, device=device)
    xd, dd = torch.from_numpy(x).to(device), torch.from_numpy(d).to(device)
    _lib.check(_lib.lib().pxt_ngp_query(tb._ctx, xd.data_ptr(), dd.data_ptr(), n, out.data_ptr(),
                                        _lib.stream_ptr(device)), "pxt_ngp_query")
    torch.cuda.synchronize()
    den, rgb = NO.network(oracle_model(s2), unit, d)
    got = out.cpu().numpy()
    e_den, e_rgb = np.abs(got[:, 0] - np.log(den)), np.abs(got[:, 1:] - rgb).max(axis=1)
    print("QUERY", name, "log density max %.3e colour max %.3e; on the upper faces %.3e %.3e" % (
        e_den.max(), e_rgb.max(), e_den[:96].max(), e_rgb[:96].max()))
    assert np.isfinite(got).all()
    assert e_den.max() < 5e-3
    assert e_rgb.max() < 5e-3


# ---- the run-time knobs of the render chain on the new geometries: every setting is a process of its own
KNOBS = {"default": {}, "first_hit_0": {"PXT_NGP_FIRST_HIT": "0"}, "first_hit_2": {"PXT_NGP_FIRST_HIT": "2"},
         "coop_0": {"PXT_NGP_COOP": "0"}}


def test_knobs_keep_every_bit_on_the_geometries():
    """scripts/render_checksum.py variants under the first-hit settings and without the cooperative patch fetch: the same
    digests (float RGBA, float depth, 8-bit image, mask plane, stats) for every geometry, as
    tests/test_ngp_first_hit_gpu.py requires of the default model."""
    base = {k: v for k, v in os.environ.items() if k not in ("PXT_NGP_FIRST_HIT", "PXT_NGP_COOP")}
    procs = {k: subprocess.Popen([sys.executable, str(ROOT / "scripts" / "render_checksum.py"), "variants"],
                                 env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, env in KNOBS.items()}
    got = {}
    for k, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, (k, err[-2000:])
        rows = [line.split() for line in out.splitlines() if line.startswith("DIGEST")]
        got[k] = {r[1]: (r[2], int(r[4]), int(r[6])) for r in rows}
        assert sorted(got[k]) == sorted(NERF_VARIANT_CASES), out
    for case, ref in got["default"].items():
        print(case, ref)
        assert ref[1] > 0 and ref[2] > 0
        for k in KNOBS:
            assert got[k][case] == ref, (k, case)
