"""SHA-256 digests of a set of small NeRF renders - every output the render chain writes (float RGBA, float depth, the 8-bit
image, the mask plane) and the statistics words stats[0] (samples composited) and stats[1] (rays that hit the render box).
Run under different values of a run-time knob of the chain (PXT_NGP_FIRST_HIT; knobs are read once per process) the digests
must not change: tests/test_ngp_first_hit_gpu.py.      python scripts/render_checksum.py

Cases: the synthetic snapshot at 64 x 48 in modes 0 / 1 / 2 at spp 8 and spp 3 (spp 3: a ray-generator thread's rays are not
one pixel's passes), the camera inside the render box, the box partly outside the frame, an occupancy grid without a set
cell (every ray leaves the box without a sample: the image is the background), an occupancy grid with every cell set, a
batched chain of 2 renders of different size and mode, a batched chain of 5 renders of 16 x 12 (the parameter records
travel through device memory)."""
import dataclasses, hashlib, math, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np, torch
from pixtrack_amd.ngp import Testbed
from pixtrack_amd.synthetic import PREMIER_PROTEIN_AABB, look_at_pose, make_synthetic_nerf

dev = torch.device("cuda:0")
LO, HI = np.array(PREMIER_PROTEIN_AABB)
CENTRE = 0.5 * (LO + HI)


def testbed(snap, direction, dist, W, background=(255, 255, 255, 0.0)):
    tb = Testbed(device=dev)
    tb.load_snapshot(snap)
    tb.background_color = list(background)
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = 1e-7
    tb.render_aabb.min, tb.render_aabb.max = PREMIER_PROTEIN_AABB
    d = np.asarray(direction, np.float64)
    eye = CENTRE + d / np.linalg.norm(d) * dist
    R, _ = look_at_pose(eye, CENTRE, up=np.array([0, 1.0, 0]))
    tb._cam_ngp = np.concatenate([R.T, eye[:, None]], 1)
    tb.fov = math.degrees(2 * math.atan(W / (2 * 1.2 * W)))
    tb.stats_accum = torch.zeros(4, dtype=torch.int64, device=dev)
    return tb


def digest(name, tensors, stats):
    h = hashlib.sha256()
    for key in sorted(tensors):
        h.update(key.encode())
        h.update(tensors[key].detach().cpu().numpy().tobytes())
    s = stats.cpu().numpy()[:2]
    h.update(s.tobytes())
    print("DIGEST", name, h.hexdigest()[:16], "samples", int(s[0]), "rays_hit", int(s[1]))


def single(name, tb, W, H, spp, mode):
    tb.stats_accum.zero_()
    out = tb.render_frame_device(W, H, spp, mode=mode, want_float=True)
    torch.cuda.synchronize()
    digest(name, out, tb.stats_accum)
    return out


def variants():
    """`render_checksum.py variants`: one 32 x 24, spp 8, mode-2 render of every case of synthetic.NERF_VARIANT_CASES (the
    snapshot geometries besides the default one: aabb_scale 1 / 2 / 16, integer level scales)."""
    from pixtrack_amd.synthetic import NERF_VARIANT_CASES, make_nerf_variant, nerf_variant_camera

    snaps = {}
    for name, case in NERF_VARIANT_CASES.items():
        if case["model"] not in snaps:
            snaps[case["model"]] = make_nerf_variant(case["model"])
        t = testbed(snaps[case["model"]], [0.0, 0.0, 1.0], 1.0, 32)
        t.render_aabb.min, t.render_aabb.max = [list(map(float, b)) for b in case["box"]]
        t._cam_ngp = nerf_variant_camera(case)
        single(name, t, 32, 24, 8, 2)


if sys.argv[1:] == ["variants"]:
    variants()
    sys.exit(0)

snap = make_synthetic_nerf(11)
tb = testbed(snap, [0.9, 0.5, 0.3], 1.2, 64)
for spp in (8, 3):
    for mode in (0, 1, 2):
        single("synthetic_mode%d_spp%d" % (mode, spp), tb, 64, 48, spp, mode)
# the camera inside the render box: tmin < 0, the rays start at the camera
single("camera_inside_box", testbed(snap, [0.9, 0.5, 0.3], 0.12, 64), 64, 48, 8, 2)
# a close-up: the box's silhouette leaves the frame on every side
single("box_leaves_frame", testbed(snap, [-0.4, 0.2, 1.0], 0.55, 50), 50, 37, 8, 2)
# no occupied cell: every ray is finished before the render kernel, the image is the background
empty = dataclasses.replace(snap, occupancy=np.zeros_like(snap.occupancy))
out = single("no_occupied_cell", testbed(empty, [0.9, 0.5, 0.3], 1.2, 64, background=(0.5, 0.25, 1.0, 1.0)), 64, 48, 8, 2)
assert torch.equal(out["rgba"], torch.tensor([0.5, 0.25, 1.0, 1.0], device=dev).expand(48, 64, 4)), "not the background"
# every cell occupied: no ray is dropped and no start moves
full = dataclasses.replace(snap, occupancy=np.full_like(snap.occupancy, 255))
single("all_cells_occupied", testbed(full, [0.9, 0.5, 0.3], 1.2, 64), 64, 48, 8, 2)


def batch(name, tbs, sizes, spp, modes):
    for t in tbs:
        t.stats_accum.zero_()
    outs = Testbed.render_frame_batch_device(tbs, sizes, spp, mode=modes, depth_float=True)
    torch.cuda.synchronize()
    for k, (t, o) in enumerate(zip(tbs, outs)):
        digest("%s_render%d" % (name, k), o, t.stats_accum)


batch("batch2", [tb, testbed(snap, [0.2, 0.9, 0.4], 1.0, 50)], [(64, 48), (50, 37)], 8, [2, 1])
views = ([0.9, 0.5, 0.3], [0.1, 0.3, 1.0], [-0.8, 0.2, 0.1], [0.2, -1.0, 0.4], [0.0, 0.1, -1.0])
batch("batch5", [testbed(snap, d, 0.9 + 0.15 * k, 16) for k, d in enumerate(views)], [(16, 12)] * 5, 8, [2, 0, 1, 2, 1])
