"""pxt_mesh_render_scene_batch and pxt_mask_exclude against mesh_render.scene_reference and
occlusion.mask_exclude_reference - bit for bit on every plane and record, no tolerance and no excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_render as R
from test_mesh_frame_gpu import same
from test_mesh_scene_host import H, T_A, T_B, T_C, W, counts, grey, mutual_pair, scene_view

pytestmark = pytest.mark.gpu

NAMES = ("A", "B", "C", "A2")


class CountingOps:
    """Stands in for a renderer's op namespace: counts the batch calls of either kind that it passes on."""

    def __init__(self, ops):
        self.ops, self.plain, self.scene = ops, 0, 0

    def mesh_render_frame_batch(self, *args):
        self.plain += 1
        return self.ops.mesh_render_frame_batch(*args)

    def mesh_render_scene_batch(self, *args):
        self.scene += 1
        return self.ops.mesh_render_scene_batch(*args)


def host(outs):
    return [[{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()} for o in item] for item in outs]


def gpu_batch(device, items, **kw):
    out = R.render_frame_batch(items, **kw)
    torch.cuda.synchronize(device)
    return host(out)


def same_items(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            same(a, b)


def counted(device, renderer, items, **kw):
    counting = CountingOps(renderer._ops)
    renderer._ops = counting
    try:
        got = gpu_batch(device, items, **kw)
    finally:
        renderer._ops = counting.ops
    return got, counting


@pytest.fixture(scope="module")
def fixture(device):
    """The fixture scene of test_mesh_scene_host: per object its scene view (depth_nz, 70 x 37) and an S = 2 reference
    view of another size that is in no scene; the two meshes' renderers; the numpy reference for r_grow = 0, once."""
    Va, Fa = R.icosphere(2)
    Vb, Fb = R.icosphere(1)
    Va, Vb = Va * 0.1, Vb * 0.12
    mesh = {"A": (Va, Fa, grey(Va, 0.7)), "B": (Vb, Fb, grey(Vb, 0.4))}
    mesh["C"] = mesh["A2"] = mesh["A"]
    rs = {"A": R.MeshRenderer(Va, Fa, device, **mesh["A"][2]), "B": R.MeshRenderer(Vb, Fb, device, **mesh["B"][2])}
    rs["C"] = rs["A2"] = rs["A"]
    t = {"A": T_A, "B": T_B, "C": T_C, "A2": T_A}
    reqs = {n: [(scene_view(t[n]), W, H, 1, ("depth_nz",)),
                (scene_view((0.0, 0.01, 0.5), fx=70.0, fy=71.0, cx=20.3, cy=14.1), 41, 29, 2, ("rgb_u8",))] for n in NAMES}
    ref = lambda names, scenes, r: R.scene_reference([mesh[n] + (reqs[n],) for n in names], scenes, r)
    want = dict(zip(NAMES, ref(NAMES, [[0, None]] * 4, 0)))
    assert [counts(want[n][0]) for n in NAMES] == [(560, 0, 0), (418, 311, 311), (490, 0, 0), (560, 0, 0)]
    return dict(mesh=mesh, renderers=rs, requests=reqs, want=want, ref=ref)


@pytest.mark.parametrize("order", [[0, 1, 2, 3], [2, 0, 3, 1]])
def test_the_fixture_scene_beside_the_reference_views_in_one_call(device, fixture, order):
    rs, reqs = fixture["renderers"], fixture["requests"]
    names = [NAMES[k] for k in order]
    got, calls = counted(device, rs["A"], [(rs[n], reqs[n]) for n in names], scenes=[[0, None]] * 4, r_grow=0)
    assert (calls.scene, calls.plain) == (1, 0)
    same_items(got, [fixture["want"][n] for n in names])
    assert all("occluder" in g[0] and "occluder" not in g[1] for g in got)


@pytest.mark.parametrize("r_grow", [1, 3, 8])
def test_growth(device, fixture, r_grow):
    rs, reqs = fixture["renderers"], fixture["requests"]
    want = fixture["ref"](NAMES, [[4, None]] * 4, r_grow)
    assert counts(want[1][0])[1] == 311 and counts(want[1][0])[2] > 311 + 20 * r_grow
    same_items(gpu_batch(device, [(rs[n], reqs[n]) for n in NAMES], scenes=[[4, None]] * 4, r_grow=r_grow), want)


def test_two_scenes_and_a_view_in_none_in_one_call(device, fixture):
    # scene 0: A and B at 70 x 37; scene 1: the mutual pair at 70 x 37 through the same camera; C is in no scene
    rs, reqs, mesh = fixture["renderers"], fixture["requests"], fixture["mesh"]
    pair = mutual_pair()
    items = [mesh["A"] + (reqs["A"],), pair[0], mesh["C"] + (reqs["C"][:1],), mesh["B"] + (reqs["B"],), pair[1]]
    scenes = [[0, None], [1], [None], [0, None], [1]]
    want = R.scene_reference(items, scenes, 2)
    assert counts(want[3][0])[1] == 311 and counts(want[1][0])[1] > 20 and counts(want[4][0])[1] > 20
    assert "occluder" not in want[2][0]
    pr = R.MeshRenderer(pair[0][0], pair[0][1], device, **pair[0][2])
    got, calls = counted(device, rs["A"], [(rs["A"], reqs["A"]), (pr, pair[0][3]), (rs["C"], reqs["C"][:1]),
                                           (rs["B"], reqs["B"]), (pr, pair[1][3])], scenes=scenes, r_grow=2)
    assert (calls.scene, calls.plain) == (1, 0)
    same_items(got, want)


def test_the_mutual_pair(device):
    pair = mutual_pair(("depth_nz", "depth"))
    want = R.scene_reference(pair, [[0], [0]], 1)
    assert counts(want[0][0])[1] > 20 and counts(want[1][0])[1] > 20
    pr = R.MeshRenderer(pair[0][0], pair[0][1], device, **pair[0][2])
    same_items(gpu_batch(device, [(pr, pair[0][3]), (pr, pair[1][3])], scenes=[[0], [0]], r_grow=1), want)
    same_items(gpu_batch(device, [(pr, pair[1][3]), (pr, pair[0][3])], scenes=[[7], [7]], r_grow=1), want[::-1])


@pytest.mark.parametrize("r_grow", [0, 3, 8])
def test_a_hidden_region_across_every_tile_seam_and_at_the_border(device, fixture, r_grow):
    """The scene kernel's tile is 64 x 16 pixels (one workgroup), with an r_grow halo.  150 x 50 is 3 x 4 tiles with seams
    at x = 64, 128 and y = 16, 32, 48; the width is not a multiple of 4 (the plane's rows are stored bytewise)."""
    Ws, Hs = 150, 50
    cam = dict(fx=200.0, fy=200.0, cx=74.6, cy=24.7)
    mesh, rs = fixture["mesh"], fixture["renderers"]
    qa = [(scene_view((0.0, 0.0, 0.25), **cam), Ws, Hs, 1, ("depth_nz",))]
    qb = [(scene_view((0.06, 0.0, 0.40), **cam), Ws, Hs, 1, ("depth_nz",))]
    want = R.scene_reference([mesh["A"] + (qa,), mesh["B"] + (qb,)], [[0], [0]], 0)
    hidden = want[1][0]["occluder"].astype(bool)
    for x in (63, 64, 127, 128, Ws - 1):
        assert hidden[:, x].any(), x
    for y in (0, 15, 16, 31, 32, 47, 48, Hs - 1):
        assert hidden[y].any(), y
    assert not hidden.all() and not want[0][0]["occluder"].any()
    if r_grow:
        want = R.scene_reference([mesh["A"] + (qa,), mesh["B"] + (qb,)], [[0], [0]], r_grow)
        assert want[1][0]["occluder"].sum() > hidden.sum()
    same_items(gpu_batch(device, [(rs["A"], qa), (rs["B"], qb)], scenes=[[0], [0]], r_grow=r_grow), want)


@pytest.mark.parametrize("Ws,Hs", [(1, 1), (5, 1)])
def test_the_smallest_views(device, fixture, Ws, Hs):
    cam = dict(fx=60.0, fy=58.0, cx=(Ws - 1) / 2, cy=0.0)
    mesh, rs = fixture["mesh"], fixture["renderers"]
    qa = [(scene_view((0.0, 0.0, 0.45), **cam), Ws, Hs, 1, ("depth_nz",))]
    qb = [(scene_view((0.0, 0.0, 0.60), **cam), Ws, Hs, 1, ("depth_nz",))]
    want = R.scene_reference([mesh["A"] + (qa,), mesh["B"] + (qb,)], [[0], [0]], 2)
    assert counts(want[1][0]) == (Ws * Hs,) * 3 and counts(want[0][0]) == (Ws * Hs, 0, 0)
    same_items(gpu_batch(device, [(rs["A"], qa), (rs["B"], qb)], scenes=[[0], [0]], r_grow=2), want)


def test_without_scenes_the_old_op_is_called_and_the_planes_are_the_parents(device, fixture):
    rs, reqs, mesh = fixture["renderers"], fixture["requests"], fixture["mesh"]
    got, calls = counted(device, rs["A"], [(rs[n], reqs[n]) for n in NAMES])
    assert (calls.scene, calls.plain) == (0, 1)
    plain = R.frame_batch_reference([mesh[n] + (reqs[n],) for n in NAMES])
    same_items(got, plain)
    # ... which are the scene call's planes too, and its record words 0..9
    for g, w in zip(got, [fixture["want"][n] for n in NAMES]):
        assert np.array_equal(g[0]["depth_nz"], w[0]["depth_nz"]) and np.array_equal(g[1]["rgb_u8"], w[1]["rgb_u8"])
        assert np.array_equal(g[0]["records"][:10], w[0]["records"][:10]) and not g[0]["records"][10:].any()


def test_what_the_scene_call_refuses_is_refused_before_anything_is_written(device, fixture):
    rs, reqs = fixture["renderers"], fixture["requests"]
    a, b = reqs["A"][:1], reqs["B"][:1]
    other_camera = [(scene_view(T_B, fx=60.5), W, H, 1, ("depth_nz",))]
    other_size = [(scene_view(T_B), W, H + 1, 1, ("depth_nz",))]
    supersampled = [(scene_view(T_B), W, H, 2, ("rgb_u8",))]
    for qb, kw in ((other_camera, {}), (other_size, {}), (supersampled, {}), (b, dict(r_grow=9)), (b, dict(r_grow=-1))):
        with pytest.raises(_lib.PxtError):
            R.render_frame_batch([(rs["A"], a), (rs["B"], qb)], scenes=[[0], [0]], **{**dict(r_grow=0), **kw})
    with pytest.raises(_lib.PxtError):
        R.render_frame_batch([(rs["A"], a), (rs["B"], b)], scenes=[[0]])  # one id per item and request
    # a scene that the 16-mesh limit would split across two calls is refused, not drawn in part
    with pytest.raises(_lib.PxtError, match="split"):
        R.render_frame_batch([(rs["A"], a)] * 17, scenes=[[0]] + [[None]] * 15 + [[0]])
    torch.cuda.synchronize(device)


@pytest.mark.parametrize("Wm,Hm", [(70, 37), (64, 16)])
@pytest.mark.parametrize("shift", [0, 4, 1])
def test_mask_exclude(device, Wm, Hm, shift):
    """16-byte aligned planes (70 * 37 leaves a 14-byte tail), planes that are 4-byte aligned only, unaligned planes."""
    from pixtrack_amd.occlusion import mask_exclude, mask_exclude_reference

    rng = np.random.default_rng(Wm + shift)
    m = (rng.integers(0, 3, (Hm, Wm)) * 100).astype(np.uint8)
    g = (rng.integers(0, 2, (Hm, Wm)) * rng.integers(1, 255, (Hm, Wm))).astype(np.uint8)
    want = mask_exclude_reference(m, g)
    assert 0 < want["record"][1] < want["record"][0] < Wm * Hm
    n = Wm * Hm

    def plane(a=None):  # a [H, W] view `shift` bytes into a guarded flat buffer
        flat = torch.full((n + 64,), 9, dtype=torch.uint8, device=device)
        v = flat[16 + shift:16 + shift + n].view(Hm, Wm)
        if a is not None:
            v.copy_(torch.from_numpy(a))
        return flat, v

    (_, mi), (_, oc), (out_flat, out) = plane(m), plane(g), plane()
    assert mi.data_ptr() % 16 == shift % 16
    mask, record = mask_exclude(mi, oc, mask=out)
    torch.cuda.synchronize(device)
    assert np.array_equal(mask.cpu().numpy(), want["mask"]) and tuple(record.cpu().tolist()) == want["record"]
    assert np.array_equal(mi.cpu().numpy(), m) and np.array_equal(oc.cpu().numpy(), g)
    guard = out_flat.cpu().numpy()
    assert (guard[:16 + shift] == 9).all() and (guard[16 + shift + n:] == 9).all()
    # in place
    in_flat, mi = plane(m)
    mask, record = mask_exclude(mi, oc, mask=mi, record=torch.zeros(16, dtype=torch.int32, device=device))
    torch.cuda.synchronize(device)
    assert mask.data_ptr() == mi.data_ptr() and np.array_equal(mi.cpu().numpy(), want["mask"])
    assert tuple(record.cpu().tolist()[:2]) == want["record"] and not any(record.cpu().tolist()[2:])
    guard = in_flat.cpu().numpy()
    assert (guard[:16 + shift] == 9).all() and (guard[16 + shift + n:] == 9).all()
    with pytest.raises(_lib.PxtError):
        mask_exclude(mi, oc, mask=oc)
