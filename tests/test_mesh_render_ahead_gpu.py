"""pxt_mesh_render_frame_batch_posed: views whose pose is read on the device from an LM output record, against the plain
batch call given ``mesh_render.posed_view_reference``'s floats - bit for bit on every plane, every record word and every
``views_out`` row.  No tolerance and no excluded pixel."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd import mesh_render as R
from test_mesh_batch_gpu import gpu_batch, same_items
from test_mesh_frame_gpu import shading_of, sphere_view
from test_mesh_raster_host import rotation

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB
ALL = ("rgba", "rgb_u8", "depth", "depth_nz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lm_record(view20, failed=0.0, status=0.0, n=16):
    """An LM output record holding the pose of ``view20``: [0..11] the pose, [12] failed, [13] status, [15] done."""
    rec = np.zeros(n, np.float32)
    rec[:12] = view20[:12]
    rec[12], rec[13], rec[14], rec[15] = failed, status, 7.0, 1.0
    return rec


def pose_free(view20):
    """What the host knows of a posed view: the intrinsics and near; the pose and depth_q are garbage the call ignores."""
    v = np.array(view20, np.float32)
    v[:12] = np.float32(123.25)
    v[17] = np.float32(-5.0)
    return v


def pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def sentinel_out(n_views, device=None):
    t = torch.empty((n_views, R.VIEW_OUT), dtype=torch.float32)
    t = t.pin_memory() if device is None else t.to(device)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


@pytest.fixture(scope="module", params=["colors", "texture"])
def probe(request, device):
    """The probe scene: icosphere(2) x 0.1 and a second, smaller mesh of the other detail, with the shading of the case."""
    V, F = R.icosphere(2)
    V2, F2 = R.icosphere(1)
    sh, sh2 = shading_of(request.param, V, F), shading_of(request.param, V2, F2, 9)
    return dict(r=R.MeshRenderer(V * 0.1, F, device, **sh), r2=R.MeshRenderer(V2 * 0.08, F2, device, **sh2),
                radius=float(np.linalg.norm(V * 0.1, axis=1).max()), radius2=float(np.linalg.norm(V2 * 0.08, axis=1).max()))


def check(device, items, poses, out_device=None, views_out=True):
    """The posed call against the plain call on the reference's floats -> (the planes, views_out on the host)."""
    n = sum(len(q) for _, q in items)
    out = sentinel_out(n, out_device) if views_out else None
    got = gpu_batch(device, [(r, [(pose_free(v) if p is not None else v, *rest) for (v, *rest), p in zip(q, ps)])
                             for (r, q), ps in zip(items, poses)], poses=poses, views_out=out)
    want_views, flags = [], []
    for (r, q), ps in zip(items, poses):
        for (v, *_), p in zip(q, ps):
            ref = (v, None) if p is None else R.posed_view_reference(p[0], pose_free(v), p[1])
            want_views.append(ref[0])
            flags.append(ref[1])
    it = iter(want_views)
    want = gpu_batch(device, [(r, [(next(it), *rest) for (v, *rest) in q]) for r, q in items])
    same_items(got, want)
    if out is None:
        return got, None
    rows = out.cpu().numpy()
    for p, (v, flag) in enumerate(zip(want_views, flags)):
        if flag is None:
            assert (rows[p].view(np.uint8) == SENTINEL).all(), p
        else:
            assert np.array_equal(bits(rows[p, :20]), bits(v)) and rows[p, 20] == flag and (bits(rows[p, 21:]) == 0).all(), p
    return got, rows


def test_one_posed_view(device, probe):
    v = sphere_view(23, 41, Rm=rotation(3))
    got, rows = check(device, [(probe["r"], [(v, 23, 41, 1, ALL)])], [[(pinned(lm_record(v)), probe["radius"])]])
    assert got[0][0]["records"][R.W_COVERED] > 100 and got[0][0]["records"][R.W_STATUS] == 0 and rows[0, 20] == 1.0
    # the pose is a bit copy, and the plane is the one the host's own record draws
    q = 1.0 / (float(np.linalg.norm(v[9:12].astype(np.float64))) + probe["radius"])
    host = v.copy()
    host[17] = np.float32(q)
    assert np.array_equal(bits(rows[0, :20]), bits(host))


def test_two_views_share_one_record(device, probe):
    v = sphere_view(23, 41, Rm=rotation(1))
    other = v.copy()
    other[12:16] = sphere_view(37, 29, 1)[12:16]
    rec = pinned(lm_record(v, n=40))  # a record with a log behind its 16 words
    got, _ = check(device, [(probe["r"], [(v, 23, 41, 1, ("depth_nz", "depth")), (other, 37, 29, 2, ("rgb_u8",))])],
                   [[(rec, probe["radius"])] * 2])
    assert got[0][0]["depth_nz"].sum() > 100 and got[0][1]["rgb_u8"].max() > 0


@pytest.mark.parametrize("where", ["pinned", "device"])
def test_three_views_on_two_meshes_the_middle_one_unposed(device, probe, where):
    place = pinned if where == "pinned" else (lambda a: torch.from_numpy(a).to(device))
    va, vb, vc = sphere_view(23, 41, Rm=rotation(2)), sphere_view(31, 22, 1), sphere_view(19, 13, 2, Rm=rotation(5))
    items = [(probe["r"], [(va, 23, 41, 1, ("depth_nz",)), (vb, 31, 22, 2, ("rgb_u8", "rgba"))]),
             (probe["r2"], [(vc, 19, 13, 1, ALL)])]
    poses = [[(place(lm_record(va)), probe["radius"]), None], [(place(lm_record(vc)), probe["radius2"])]]
    got, rows = check(device, items, poses, out_device=None if where == "pinned" else device)
    assert rows[0, 20] == 1.0 and rows[2, 20] == 1.0 and all(o["records"][R.W_COVERED] > 20 for item in got for o in item)


@pytest.mark.parametrize("failed,status", [(1.0, 0.0), (0.0, -4.0), (1.0, -6.0)])
def test_a_failed_refinement_is_flagged_and_still_drawn(device, probe, failed, status):
    v = sphere_view(23, 41, Rm=rotation(4))
    got, rows = check(device, [(probe["r"], [(v, 23, 41, 1, ("depth_nz", "rgb_u8"))])],
                      [[(pinned(lm_record(v, failed, status)), probe["radius"])]])
    assert rows[0, 20] == -1.0 and got[0][0]["records"][R.W_COVERED] > 100


def test_a_nan_translation_draws_nothing_beside_an_intact_view(device, probe):
    v, w = sphere_view(23, 41), sphere_view(19, 13, 1)
    bad = v.copy()
    bad[10] = np.nan
    got, rows = check(device, [(probe["r"], [(bad, 23, 41, 1, ALL), (w, 19, 13, 1, ("depth_nz",))])],
                      [[(pinned(lm_record(bad)), probe["radius"]), (pinned(lm_record(w)), probe["radius"])]])
    rec = got[0][0]["records"]
    assert rec[R.W_STATUS] == 0xFFFFFFFF and rec[R.W_COVERED] == 0
    assert all((got[0][0][k] == 0).all() for k in ALL)
    assert np.isnan(rows[0, 10]) and np.isnan(rows[0, 17]) and rows[0, 20] == 1.0
    assert got[0][1]["records"][R.W_STATUS] == 0 and got[0][1]["depth_nz"].sum() > 20


def test_without_views_out(device, probe):
    v = sphere_view(23, 41, Rm=rotation(6))
    check(device, [(probe["r"], [(v, 23, 41, 2, ("rgb_u8",))])], [[(pinned(lm_record(v)), probe["radius"])]], views_out=False)


def test_depth_q_of_a_full_table_of_random_poses(device, probe):
    # 32 views per call: every lane of the table, and the float64 chain (square, add, add, sqrt, add, divide) on 96 poses
    rng = np.random.default_rng(11)
    for call in range(3):
        reqs, poses = [], []
        for p in range(R.BATCH_MAX_VIEWS):
            t = rng.normal((0.0, 0.0, 3.0), (0.5, 0.5, 1.0)).astype(np.float32)
            v = sphere_view(5, 4, Rm=rotation(100 * call + p), t=tuple(float(x) for x in t))
            reqs.append((pose_free(v), 5, 4, 1, ("depth_nz",)))
            poses.append((pinned(lm_record(v)), float(rng.uniform(0.05, 2.0))))
        out = sentinel_out(len(reqs))
        R.render_frame_batch([(probe["r"], reqs)], poses=[poses], views_out=out, download_records=False)
        torch.cuda.synchronize(device)
        rows = out.numpy()
        for p, (req, (rec, radius)) in enumerate(zip(reqs, poses)):
            want, flag = R.posed_view_reference(rec, req[0], radius)
            assert np.array_equal(bits(rows[p, :20]), bits(want)) and rows[p, 20] == flag, (call, p)


def test_bad_arguments_are_refused_and_nothing_is_written(device, probe):
    L, C = _lib.lib(), _lib.C
    r, W, H = probe["r"], 15, 11
    n, off1 = W * H * 3, (W * H * 3 + 3) // 4 * 4  # the second view's plane starts on a multiple of 4: one byte between them
    geometry, offsets = [W, H, 1, W, H, 1], [-1, 0, -1, -1, -1, off1, -1, -1]
    need = int(L.pxt_mesh_render_frame_batch_workspace_bytes(1, (C.c_int32 * 1)(r.n_triangles), 2, (C.c_int32 * 2)(0, 0),
                                                               (C.c_int32 * 6)(*geometry)))
    assert need > 0
    v = sphere_view(W, H)
    views = np.ascontiguousarray(np.stack([pose_free(v), v]))
    rec = torch.from_numpy(lm_record(v, n=20)).to(device)
    outs = dict(u8=torch.empty(off1 + n + 8, dtype=torch.uint8, device=device),
                rec=torch.empty(3 * 16, dtype=torch.int32, device=device),
                ws=torch.empty(need + 32, dtype=torch.uint8, device=device),
                out=torch.empty(3 * R.VIEW_OUT, dtype=torch.float32, device=device))
    for t in outs.values():
        t.view(torch.uint8).fill_(SENTINEL)
    d = _lib.MeshDesc()
    d.vertices, d.triangles, d.colors = r.vertices.data_ptr(), r.triangles.data_ptr(), _lib.dptr(r.colors)
    d.uvs, d.triangle_uvs, d.texture = _lib.dptr(r.uvs), _lib.dptr(r.triangle_uvs), _lib.dptr(r.texture)
    d.n_vertices, d.n_triangles = r.n_vertices, r.n_triangles
    if r.texture is not None:
        d.n_uvs, d.tex_width, d.tex_height = int(r.uvs.shape[0]), int(r.texture.shape[1]), int(r.texture.shape[0])
    stream = _lib.stream_ptr(device)

    def call(pose=((rec.data_ptr(), 0.1), (None, 0.0)), table=True, out=outs["out"].data_ptr(), p=2, geo=geometry,
             views_ptr=views.ctypes.data, ws=outs["ws"].data_ptr()):
        t = (_lib.MeshViewPose * 2)()
        for k, (ptr, radius) in enumerate(pose):
            t[k].pose_record, t[k].radius = ptr, radius
        return L.pxt_mesh_render_frame_batch_posed(
            (_lib.MeshDesc * 1)(d), 1, (C.c_int32 * 2)(0, 0), views_ptr, p, (C.c_int32 * len(geo))(*geo),
            (C.c_int64 * 8)(*offsets), None, outs["u8"].data_ptr(), None, None,
            (C.c_int64 * 4)(0, outs["u8"].numel(), 0, 0), outs["rec"].data_ptr(), ws, t if table else None, out, stream)

    ptr = rec.data_ptr()
    bad = [dict(table=False),                                                                  # view_pose NULL
           dict(pose=((ptr, -0.5), (None, 0.0))), dict(pose=((ptr, float("nan")), (None, 0.0))),  # the radius
           dict(pose=((ptr, float("inf")), (None, 0.0))), dict(pose=((ptr, 0.1), (ptr, -1e-300))),
           dict(pose=((ptr + 2, 0.1), (None, 0.0))), dict(pose=((ptr, 0.1), (ptr + 1, 0.1))),    # alignment
           dict(out=outs["out"].data_ptr() + 2),
           dict(p=0), dict(p=33), dict(geo=[W, H, 3, W, H, 1]), dict(views_ptr=None), dict(ws=None),  # the batch call's own
           dict(ws=outs["ws"].data_ptr() + 8)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize(device)
    for name, t in outs.items():
        assert (t.view(torch.uint8) == SENTINEL).all(), name
    # an un-posed view's radius is ignored, whatever it holds; the same buffers serve the good call
    assert call(pose=((ptr, 0.1), (None, float("nan")))) == 0
    torch.cuda.synchronize(device)
    rows = outs["out"].cpu().numpy().reshape(3, R.VIEW_OUT)
    want, flag = R.posed_view_reference(rec, views[0], 0.1)
    assert np.array_equal(bits(rows[0, :20]), bits(want)) and rows[0, 20] == flag == 1.0
    assert (rows[1:].view(np.uint8) == SENTINEL).all()
    assert (outs["rec"][32:].view(torch.uint8) == SENTINEL).all() and (outs["ws"][need:] == SENTINEL).all()
    plain = gpu_batch(device, [(r, [(want, W, H, 1, ("rgb_u8",)), (v, W, H, 1, ("rgb_u8",))])])
    u8 = outs["u8"].cpu().numpy()
    assert np.array_equal(u8[:n].reshape(H, W, 3), plain[0][0]["rgb_u8"]) and plain[0][0]["rgb_u8"].max() > 0
    assert np.array_equal(u8[off1:off1 + n].reshape(H, W, 3), plain[0][1]["rgb_u8"])
    assert off1 > n and (u8[n:off1] == SENTINEL).all() and (u8[off1 + n:] == SENTINEL).all()


def test_the_op_checks_before_any_launch(device, probe):
    from pixtrack_amd.ops import ops

    r, W, H = probe["r"], 16, 12
    v = sphere_view(W, H)
    rec = pinned(lm_record(v))
    u8 = torch.full((W * H * 3,), SENTINEL, dtype=torch.uint8, device=device)
    records = torch.full((1, 16), -1, dtype=torch.int32, device=device)
    need = int(_lib.lib().pxt_mesh_render_frame_batch_workspace_bytes(
        1, (_lib.C.c_int32 * 1)(r.n_triangles), 1, (_lib.C.c_int32 * 1)(0), (_lib.C.c_int32 * 3)(W, H, 1)))
    out = sentinel_out(1)
    good = dict(v=[r.vertices], f=[r.triangles], c=[r.colors], uv=[r.uvs], fuv=[r.triangle_uvs], tex=[r.texture], vm=[0],
                views=torch.from_numpy(pose_free(v)[None]), geo=[W, H, 1], off=[-1, 0, -1, -1], poses=[rec], radii=[0.1],
                rgba=None, u8=u8, depth=None, nz=None, rec=records, ws=torch.empty(need, dtype=torch.uint8, device=device),
                out=out)
    bad = [dict(poses=[]), dict(poses=[rec, rec]), dict(radii=[]), dict(radii=[-1.0]), dict(radii=[float("nan")]),
           dict(radii=[float("inf")]), dict(poses=[rec[:12]]), dict(poses=[rec.double()]), dict(poses=[rec.clone()]),  # unpinned
           dict(poses=[torch.zeros(32).pin_memory()[::2]]), dict(out=torch.zeros(1, R.VIEW_OUT)), dict(out=out[:, :20]),
           dict(out=torch.zeros(2, R.VIEW_OUT).pin_memory()), dict(out=out.double()), dict(geo=[W, H, 3]), dict(vm=[1]),
           dict(u8=u8[:-1]), dict(views=torch.from_numpy(pose_free(v)[None]).to(device))]
    for kw in bad:
        with pytest.raises(_lib.PxtError):
            ops.mesh_render_frame_batch_posed(*{**good, **kw}.values())
    torch.cuda.synchronize(device)
    assert (u8 == SENTINEL).all() and (records == -1).all() and (out.view(torch.uint8) == SENTINEL).all()
    ops.mesh_render_frame_batch_posed(*good.values())
    torch.cuda.synchronize(device)
    want, _ = R.posed_view_reference(rec, pose_free(v), 0.1)
    assert np.array_equal(bits(out.numpy()[0, :20]), bits(want)) and out[0, 20] == 1.0
    plain = gpu_batch(device, [(r, [(want, W, H, 1, ("rgb_u8",))])])
    assert np.array_equal(u8.cpu().numpy().reshape(H, W, 3), plain[0][0]["rgb_u8"])
    with pytest.raises(_lib.PxtError):  # poses and scenes do not combine; views_out goes with poses
        R.render_frame_batch([(r, [(v, W, H, 1, ("depth_nz",))])], poses=[[(rec, 0.1)]], scenes=[[0]])
    with pytest.raises(_lib.PxtError):
        R.render_frame_batch([(r, [(v, W, H, 1, ("depth_nz",))])], views_out=out)


def test_the_posed_call_queued_behind_the_lm_launch(device, probe):
    """As test_lm_epilogue_camera_equals_the_conversion_kernel: the refinement's launch and, with no host synchronisation
    between the two, the posed call that reads its output record; the planes are the plain call's at ``res.T``."""
    from pixtrack_amd.optimizer import LevelPack, PixTrackOptimizer, cstride_for
    from pixtrack_amd.synthetic import make_lm_scene

    sc = make_lm_scene(seed=1007, width=160, height=120, n_points=600, sigma_px=2.0)
    packs = []
    for level in reversed(range(3)):
        fq = sc.feats_query[level]
        Cc = fq.shape[0] - 1
        fmap = torch.zeros(fq.shape[1], fq.shape[2], cstride_for(Cc))
        fmap[..., :Cc] = torch.nn.functional.normalize(fq[:-1], dim=0).permute(1, 2, 0)
        fmap[..., Cc] = fq[-1]
        fr = sc.feats_ref[level]
        fref = torch.zeros(fr.shape[0], cstride_for(Cc))
        fref[:, :Cc] = torch.nn.functional.normalize(fr[:, :-1], dim=1)
        fref[:, Cc] = fr[:, -1]
        packs.append(LevelPack(fmap.to(device).contiguous(), fref.to(device).contiguous(), Cc,
                               sc.camera.scale(sc.scales[level]), torch.full((6,), 1e-4)))
    p3d = torch.from_numpy(sc.p3d).float().to(device)
    ws = torch.zeros(int(_lib.lib().pxt_lm_workspace_bytes()), dtype=torch.uint8, device=device)
    opt = PixTrackOptimizer(dict(num_iters=150, pad=1))
    r, radius = probe["r"], probe["radius"]
    W, H = 160, 120
    host = R.view_record(sc.camera, sc.T_init, 1e-6, 0.0)
    host[:12] = 0.0
    requests = [(host, W, H, 1, ("depth_nz", "depth")), (host, W, H, 2, ("rgb_u8",))]
    out = sentinel_out(2)
    batch_ws = R.FrameBatchWorkspace()
    R.render_frame_batch([(r, requests)], workspace=batch_ws, download_records=False)  # the plan and the staging ring exist
    torch.cuda.synchronize(device)
    pend = PixTrackOptimizer.refine_levels(p3d, packs, sc.T_init, opt.native_conf(), ws)
    ahead = R.render_frame_batch([(r, requests)], workspace=batch_ws, poses=[[(pend.buf, radius)] * 2], views_out=out)
    res = pend.result()
    assert not res.failed
    torch.cuda.synchronize(device)
    rows = out.numpy()
    assert rows[0, 20] == 1.0 and rows[1, 20] == 1.0
    q = 1.0 / (float(np.linalg.norm(R._pose_Rt(res.T)[1])) + radius)
    want_view = R.view_record(sc.camera, res.T, 1e-6, q)
    assert np.array_equal(bits(rows[0, :20]), bits(want_view)) and np.array_equal(bits(rows[1, :20]), bits(want_view))
    plain = gpu_batch(device, [(r, [(want_view, W, H, 1, ("depth_nz", "depth")), (want_view, W, H, 2, ("rgb_u8",))])])
    got = [[{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()} for o in item] for item in ahead]
    same_items(got, plain)
