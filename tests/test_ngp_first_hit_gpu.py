"""The first-hit pass of the render chain (ngp_first_hit_kernel: every ray walked to its first occupied lattice point, groups
of rays without one finished before the render kernel) must not change a bit of any output: the walk is memoryless, a
ray started at its first occupied lattice point visits the samples it visits when started at the box entry.
PXT_NGP_FIRST_HIT is read once per process, so every setting is a subprocess of scripts/render_checksum.py (as
tests/test_variants_gpu.py does for the other knobs); the digests - float RGBA, float depth, 8-bit image, mask plane, stats[0]
and stats[1] of every case - are compared.  One case is checked against the CPU oracle."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

CASES = ["synthetic_mode%d_spp%d" % (m, s) for s in (8, 3) for m in (0, 1, 2)] + [
    "camera_inside_box", "box_leaves_frame", "no_occupied_cell", "all_cells_occupied",
    "batch2_render0", "batch2_render1"] + ["batch5_render%d" % k for k in range(5)]
# 1: the default (whole groups of 8 rays dropped); 0: the chain without the launch; 2: single rays dropped
SETTINGS = ("0", "1", "2")


@pytest.fixture(scope="module")
def digests():
    """{setting: {case: (digest, samples, rays_hit)}} - the three processes run side by side."""
    procs = {v: subprocess.Popen([sys.executable, str(ROOT / "scripts" / "render_checksum.py")],
                                 env=dict(os.environ, PXT_NGP_FIRST_HIT=v), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                 text=True) for v in SETTINGS}
    got = {}
    for v, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, (v, err[-2000:])
        rows = [line.split() for line in out.splitlines() if line.startswith("DIGEST")]
        got[v] = {r[1]: (r[2], int(r[4]), int(r[6])) for r in rows}
        assert sorted(got[v]) == sorted(CASES), out
    return got


@pytest.mark.parametrize("case", CASES)
def test_first_hit_pass_keeps_every_bit(digests, case):
    off = digests["0"][case]
    print(case, off)
    assert digests["1"][case] == off
    assert digests["2"][case] == off
    assert off[2] > 0  # rays did hit the box
    if case == "no_occupied_cell":
        assert off[1] == 0
    else:
        assert off[1] > 0


def test_first_hit_chain_matches_the_oracle(device):
    """48 x 36, spp 2, the default chain: stats[0] / stats[1] are the oracle's sample and ray counts, the image lies within
    the tolerance of tests/test_ngp_gpu.py's comparison."""
    from oracle import ngp_oracle as NO
    from pixtrack_amd.ngp import RenderMode, Testbed
    from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, look_at_pose, make_synthetic_nerf

    assert os.environ.get("PXT_NGP_FIRST_HIT", "1") != "0"
    snap = make_synthetic_nerf(11)
    W, H, spp = 48, 36, 2
    lo, hi = np.array(PREMIER_PROTEIN_AABB)
    c = 0.5 * (lo + hi)
    d = np.array([0.9, 0.5, 0.3])
    eye = c + d / np.linalg.norm(d) * 1.2
    R, _ = look_at_pose(eye, c, up=np.array([0.0, 1.0, 0.0]))
    cam = np.concatenate([R.T, eye[:, None]], 1)
    m = NO.NgpModel(grid=snap.grid, mlp=snap.mlp_dict(), occupancy=snap.occupancy, cascades=snap.cascades,
                    aabb_scale=snap.aabb_scale, cone_angle=snap.cone_angle, depth_scale=1.0 / snap.scale,
                    linear_colors=snap.linear_colors)
    v = NO.View(cam=cam, focal=1.2 * W, width=W, height=H, spp=spp, aabb_min=tuple(PREMIER_PROTEIN_AABB[0]),
                aabb_max=tuple(PREMIER_PROTEIN_AABB[1]), mode=0)
    ref, st = NO.render(m, v, return_stats=True)

    tb = Testbed(device=device)
    tb.load_snapshot(snap)
    tb.background_color = [255, 255, 255, 0.0]
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = 1e-7
    tb.render_aabb.min, tb.render_aabb.max = PREMIER_PROTEIN_AABB
    tb._cam_ngp = cam
    tb.fov = math.degrees(2 * math.atan(W / (2 * 1.2 * W)))
    tb.render_mode = RenderMode.Shade
    out = tb.render_device(W, H, spp, True, collect_stats=True).cpu().numpy()
    stats = tb.read_stats()
    print(stats, st)
    assert stats["rays_hit"] == st["rays_hit"]
    assert stats["samples"] == st["samples"]
    scale = max(1.0, float(np.abs(ref[..., :3]).max()))
    diff = np.abs(out - ref) / scale
    print("max", diff.max(), "mean", diff.mean())
    assert diff.max() < 1e-2, diff.max()
    assert diff.mean() < 5e-4, diff.mean()
    assert (ref[..., 3] > 0.99).mean() > 0.05  # the object is really there
