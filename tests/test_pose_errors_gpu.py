"""pxt_pose_errors (csrc/pxt_eval.hip) / torch.ops.pixtrack.pose_errors and the evaluation API on top of it: ADD and
ADD-S of F frames in one call, against a float64 oracle.

Oracle: float64 numpy - ADD is the direct mean / max of |T_est v - T_gt v|; ADD-S is evaluation.adds_distance.  adds_distance
costs 0.2 s per frame at V = 1500, so it is called on every frame where V <= 257 and on frames 0, 1, 2 and the last one of
the larger clouds (all of the F = 1 and F = 3 cases); every frame of every cloud has the per-point nearest distances of a
float64 k-d tree (exact nearest neighbours; this also gives the max that adds_distance does not return), and the tree's
mean must equal adds_distance to 1e-12 wherever both exist - four orders of magnitude below the bar.

Bar (the project's convention): first the error of a float32 restatement of the kernel's
relative form (centred float32 vertices, float32 T_rel, elementwise float32 arithmetic, no FMA) against the oracle is
measured on the very inputs of the tests; the kernel may be 4 x that maximum off.  It is expressed relative to the
model's diameter (0.2), not to the value, so that a small pose error gets no free pass.
Measured (seeded inputs below, 6 clouds x 70 frames x 4 words): restatement max 3.18e-07 of the diameter (6.36e-08
absolute) -> bar 1.27e-06 of the diameter (2.54e-07 absolute).  The kernel's own figure is printed per case before the assertion (pytest -s)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, evaluation as E, ops

pytestmark = pytest.mark.gpu

DIAMETER = 0.2
VS = (1, 63, 257, 1024, 1025, 1500)  # one lane, a partial wave, a partial query block, an exact tile, tile + 1, ragged blocks
FS = (1, 3, 70)
FMAX = max(FS)
IDENTITY_FRAME = 1
SENTINEL = -777.0


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _cloud(V, seed):
    """Seeded Gaussian cloud scaled to diameter 0.2, away from the origin (so that centring matters)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(V, 3))
    if V > 1:
        from scipy.spatial.distance import pdist

        p *= DIAMETER / pdist(p).max()
    return p + np.array([0.31, -0.12, 0.45])


def _poses(F, seed):
    """Random ground truth; estimates = ground truth perturbed (in the object frame) by rotations of 0..0.3 rad and
    translations of 0..0.05; frame IDENTITY_FRAME is not perturbed."""
    rng = np.random.default_rng(seed)
    T_gt, T_est = [], []
    for k in range(F):
        g = _T(_rot(rng.normal(size=3), rng.uniform(0, np.pi)), np.r_[rng.uniform(-0.5, 0.5, 2), rng.uniform(1.0, 3.0)])
        d = rng.normal(size=3)
        D = _T(_rot(rng.normal(size=3), rng.uniform(0, 0.3)), d / np.linalg.norm(d) * rng.uniform(0, 0.05))
        T_gt.append(g)
        T_est.append(g.copy() if k == IDENTITY_FRAME else g @ D)
    return np.stack(T_est), np.stack(T_gt)


def _oracle(T_est, T_gt, v, with_adds_distance):
    """float64: (ADD, max, ADD-S, max) and adds_distance's figure (or NaN)."""
    from scipy.spatial import cKDTree

    a = v @ T_est[:3, :3].T + T_est[:3, 3]
    b = v @ T_gt[:3, :3].T + T_gt[:3, 3]
    d = np.linalg.norm(a - b, axis=1)
    nn = cKDTree(a).query(b)[0]  # for every ground-truth point the nearest estimated point
    return [d.mean(), d.max(), nn.mean(), nn.max()], (E.adds_distance(T_est, T_gt, v) if with_adds_distance else np.nan)


def _restate32(rel, u):
    """The kernel's relative form in elementwise float32 (torch on the host: IEEE float32, no FMA)."""
    rel, u = torch.from_numpy(rel), torch.from_numpy(u)
    out = []
    for p in rel:
        R, t = p[:9].reshape(3, 3), p[9:]
        tu = u[:, 0:1] * R[:, 0] + u[:, 1:2] * R[:, 1] + u[:, 2:3] * R[:, 2] + t
        d = ((tu - u) ** 2).sum(-1).sqrt()
        nn = ((tu[None, :, :] - u[:, None, :]) ** 2).sum(-1).min(dim=1).values.sqrt()
        out.append([float(d.mean()), float(d.max()), float(nn.mean()), float(nn.max())])
    return np.array(out, np.float64)


@pytest.fixture(scope="module")
def refs():
    """Per V: the cloud, FMAX poses, the kernel's inputs, the float64 oracle and the float32 restatement; and the bar."""
    out, worst = {}, 0.0
    for V in VS:
        v = _cloud(V, 100 + V)
        T_est, T_gt = _poses(FMAX, 200 + V)
        c = v.mean(axis=0)
        u = (v - c).astype(np.float32)
        rel = E.relative_poses(T_est, T_gt, c)
        want, via_adds = [], []
        for k in range(FMAX):
            w, a = _oracle(T_est[k], T_gt[k], v, V <= 257 or k in (0, 1, 2, FMAX - 1))
            want.append(w)
            via_adds.append(a)
        want, via_adds = np.array(want), np.array(via_adds)
        have = np.isfinite(via_adds)
        assert have.sum() >= 4 and np.abs(via_adds[have] - want[have, 2]).max() < 1e-12
        want[have, 2] = via_adds[have]  # adds_distance IS the ADD-S oracle where it was run
        restated = _restate32(rel, u)
        worst = max(worst, float(np.abs(restated - want).max()))
        out[V] = dict(v=v, T_est=T_est, T_gt=T_gt, u=u, rel=rel, want=want)
    out["restatement"] = worst / DIAMETER
    out["bar"] = 4.0 * worst  # absolute; 4 x restatement / DIAMETER of the diameter
    print(f"float32 restatement: max {worst / DIAMETER:.3e} of the diameter ({worst:.3e}); bar {4 * worst / DIAMETER:.3e} "
          f"({4 * worst:.3e})")
    assert 0 < out["bar"] < 1e-5 * DIAMETER  # float32 on object-sized numbers: far below any pose error of interest
    return out


def _run(device, u, rel, want_adds=True, records=None):
    """One call of the op on host arrays; -> the records tensor (device)."""
    verts = torch.from_numpy(np.ascontiguousarray(u, np.float32)).to(device)
    poses = torch.from_numpy(np.ascontiguousarray(rel, np.float32)).to(device)
    F, V = len(rel), len(u)
    if records is None:
        records = torch.full((F, 8), SENTINEL, device=device)
    ws = torch.empty(int(_lib.lib().pxt_pose_errors_workspace_bytes(F, V)), dtype=torch.uint8, device=device)
    ops.ops.pose_errors(verts, poses, want_adds, records, ws)
    return records


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("V", VS)
def test_records_match_the_float64_oracle(device, refs, V, F):
    r = refs[V]
    rec = _run(device, r["u"], r["rel"][:F]).cpu().numpy().astype(np.float64)
    err = np.abs(rec[:, :4] - r["want"][:F])
    print(f"V {V} F {F}: max error {err.max():.3e} = {err.max() / DIAMETER:.3e} of the diameter; bar {refs['bar']:.3e}")
    assert (rec[:, 7] == 1.0).all() and (rec[:, 4] == V).all() and (rec[:, 5:7] == 0.0).all()
    assert err.max() <= refs["bar"], (err.max(axis=0), refs["bar"])
    if F > IDENTITY_FRAME:
        assert (rec[IDENTITY_FRAME, :4] == 0.0).all()
    assert (rec[:, 2] <= rec[:, 0]).all() and (rec[:, 0] <= rec[:, 1]).all() and (rec[:, 2] <= rec[:, 3]).all()


# ------------------------------------------------------------------------------------------------ 2. identity
def test_identity_is_exactly_zero(device, refs):
    r = refs[1500]
    rel = E.relative_poses(r["T_gt"][:5], r["T_gt"][:5].copy(), r["v"].mean(axis=0))
    want = np.r_[np.eye(3).reshape(-1), np.zeros(3)].astype(np.float32)
    assert (rel.view(np.uint32) == want.view(np.uint32)).all()
    rec = _run(device, r["u"], rel).cpu()
    assert torch.equal(_bits(rec[:, :4]), torch.zeros(5, 4, dtype=torch.int32))  # +0.0, not -0.0
    assert (rec[:, 7] == 1.0).all()


# ------------------------------------------------------------------------------------------------ 3. symmetry
def test_a_symmetric_object_turned_onto_itself(device, refs):
    edge = 0.1
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    mids = np.array([(a + b) / 2 for i, a in enumerate(corners) for b in corners[i + 1:] if np.abs(a - b).sum() == 1])
    assert len(mids) == 12
    v = np.r_[corners, mids] * edge + np.array([0.4, 0.2, -0.3])
    c = v.mean(axis=0)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # exactly 90 degrees
    S = _T(Rz, c - Rz @ c)  # about the z axis through the centroid
    T_gt = refs[63]["T_gt"][:3]
    T_est = np.stack([g @ S for g in T_gt])
    rec = _run(device, (v - c).astype(np.float32), E.relative_poses(T_est, T_gt, c)).cpu().numpy().astype(np.float64)
    for k in range(3):
        want, via_adds = _oracle(T_est[k], T_gt[k], v, True)
        assert via_adds <= refs["bar"] and want[3] <= refs["bar"] and want[0] > edge / 2
        assert np.abs(rec[k, :4] - want).max() <= refs["bar"]
    assert (rec[:, 2] <= refs["bar"]).all() and (rec[:, 3] <= refs["bar"]).all()
    assert (rec[:, 0] > edge / 2).all()


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_bit_identical_whatever_the_batch_the_order_and_the_stream(device, refs):
    r = refs[1500]
    u, rel = r["u"], r["rel"][:24]
    base = _bits(_run(device, u, rel))
    perm = np.random.default_rng(9).permutation(24)
    assert torch.equal(_bits(_run(device, u, rel[perm])), base[perm])
    for k in range(24):
        assert torch.equal(_bits(_run(device, u, rel[k:k + 1])), base[k:k + 1]), k
    verts, poses = torch.from_numpy(u).to(device), torch.from_numpy(rel).to(device)
    ws = torch.empty(int(_lib.lib().pxt_pose_errors_workspace_bytes(24, 1500)), dtype=torch.uint8, device=device)
    outs = [torch.full((24, 8), SENTINEL, device=device) for _ in range(20)]
    for o in outs:
        ops.ops.pose_errors(verts, poses, True, o, ws)
    torch.cuda.synchronize(device)
    assert all(torch.equal(_bits(o), base) for o in outs)
    # ADD only: the same bits in words 0, 1 (and 4..7), 0.0 in words 2, 3
    lean = _bits(_run(device, u, rel, want_adds=False))
    assert torch.equal(lean[:, :2], base[:, :2]) and torch.equal(lean[:, 4:], base[:, 4:])
    assert torch.equal(lean[:, 2:4], torch.zeros(24, 2, dtype=torch.int32))
    # on a side stream, beside another stream's UNet pass
    from pixtrack_amd.unet import UNet, make_synthetic_unet_weights

    net = UNet(make_synthetic_unet_weights(7), device)
    img = torch.rand(240, 320, 3, device=device) * 255
    main, side = torch.cuda.current_stream(device), torch.cuda.Stream(device=device)
    out = torch.full((24, 8), SENTINEL, device=device)
    side.wait_stream(main)
    net.forward_packed(img, None, True)
    with torch.cuda.stream(side):
        ops.ops.pose_errors(verts, poses, True, out, ws)
    net.forward_packed(img, None, True)
    torch.cuda.synchronize(device)
    assert torch.equal(_bits(out), base)


# ------------------------------------------------------------------------------------------------ 5. bad input
def test_a_non_finite_pose_marks_its_frame_only(device, refs):
    r = refs[1025]
    rel = r["rel"][:5].copy()
    base = _bits(_run(device, r["u"], rel))
    for word, value in ((4, np.nan), (10, np.inf), (0, -np.inf)):
        bad = rel.copy()
        bad[2, word] = value
        for want_adds in (True, False):
            rec = _run(device, r["u"], bad, want_adds=want_adds).cpu()
            assert rec[2, 7] == -1.0 and (rec[2, :7] == SENTINEL).all()
            keep = [0, 1, 3, 4]
            if want_adds:
                assert torch.equal(_bits(rec)[keep], base[keep])
            else:
                assert torch.equal(_bits(rec)[keep][:, :2], base[keep][:, :2]) and (rec[keep, 7] == 1.0).all()


def test_invalid_arguments_raise(device, refs):
    r = refs[63]
    L = _lib.lib()
    verts, poses = torch.from_numpy(r["u"]).to(device), torch.from_numpy(r["rel"][:3]).to(device)
    rec = torch.zeros(3, 8, device=device)
    ws = torch.empty(4096, dtype=torch.uint8, device=device)
    ops.ops.pose_errors(verts, poses, True, rec, ws)
    # through the op
    with pytest.raises(_lib.PxtError):  # V = 0
        ops.ops.pose_errors(verts[:0], poses, True, rec, ws)
    with pytest.raises(_lib.PxtError):  # F = 0
        ops.ops.pose_errors(verts, poses[:0], True, rec[:0], ws)
    with pytest.raises(_lib.PxtError):  # a workspace smaller than _workspace_bytes
        ops.ops.pose_errors(verts, poses, True, rec, ws[:int(L.pxt_pose_errors_workspace_bytes(3, 63)) - 1])
    with pytest.raises(_lib.PxtError):  # records of another shape
        ops.ops.pose_errors(verts, poses, True, torch.zeros(2, 8, device=device), ws)
    with pytest.raises(_lib.PxtError):  # host memory beside device tensors
        ops.ops.pose_errors(verts, poses, True, rec, ws.cpu())
    with pytest.raises(_lib.PxtError):  # F = 65536
        ops.ops.pose_errors(verts, torch.zeros(65536, 12, device=device), True, torch.zeros(65536, 8, device=device),
                            torch.empty(65536 * 16, dtype=torch.uint8, device=device))
    with pytest.raises(_lib.PxtError):  # V = 2^20 + 1
        ops.ops.pose_errors(torch.zeros((1 << 20) + 1, 3, device=device), poses, True, rec,
                            torch.empty(3 * 1025 * 16, dtype=torch.uint8, device=device))
    # the entry point's own checks (nothing is launched)
    s = _lib.stream_ptr(device)
    a = (verts.data_ptr(), 63, poses.data_ptr(), 3, 1, rec.data_ptr(), ws.data_ptr(), s)

    def call(**kw):
        args = list(a)
        for i, val in kw.items():
            args[int(i[1:])] = val
        return L.pxt_pose_errors(*args)

    assert call() == 0
    for kw in (dict(_1=0), dict(_3=0), dict(_3=65536), dict(_1=(1 << 20) + 1), dict(_0=None), dict(_2=None), dict(_5=None),
               dict(_6=None), dict(_0=verts.data_ptr() + 2)):
        assert call(**kw) == -1, kw  # PXT_E_ARG
        with pytest.raises(_lib.PxtError):
            _lib.check(call(**kw), "pxt_pose_errors")
    torch.cuda.synchronize(device)


# ------------------------------------------------------------------------------------------------ 6. host wrapper
def test_pose_errors_is_the_raw_op(device, refs):
    r = refs[1500]
    rec = _run(device, r["u"], r["rel"]).cpu().numpy()
    res = E.pose_errors(r["T_est"], r["T_gt"], np.c_[r["v"], np.ones(1500)], device)
    for k, name in enumerate(("add", "add_max", "adds", "adds_max")):
        np.testing.assert_array_equal(res[name].astype(np.float32).view(np.uint32), rec[:, k].view(np.uint32))
    assert res["ok"].all() and res["ok"].dtype == bool
    lean = E.pose_errors(list(r["T_est"]), list(r["T_gt"]), r["v"], device, adds=False)
    np.testing.assert_array_equal(lean["add"], res["add"])
    assert np.isnan(lean["adds"]).all()


def test_evaluate_poses_reproduces_get_metrics(device, refs):
    from pixtrack_amd.geometry import Pose

    r = refs[257]
    v4 = np.c_[r["v"], np.ones(257)]
    poses = {}
    for k in range(12):
        poses[f"{k:06d}.png"] = dict(T_refined=Pose.from_4x4mat(torch.from_numpy(r["T_est"][k]).float()),
                                     gt_pose=Pose.from_4x4mat(torch.from_numpy(r["T_gt"][k]).float()),
                                     success=k not in (4, 9), tracked=k not in (4, 9, 10))
    want = E.get_metrics(poses, v4, 5.0, 5.0)
    got = E.evaluate_poses(poses, v4, device, offset=True, max_distance=DIAMETER, threshold=0.1 * DIAMETER)
    print("add_mean x 100", got["add_mean"] * 100, "average_error_vertices", want["average_error_vertices"])
    assert abs(got["add_mean"] * 100 - want["average_error_vertices"]) <= refs["bar"] * 100
    assert got["n_frames"] == 12 and got["n_success"] == 10 and got["n_tracked"] == 9 and got["n_evaluated"] == 10
    names = list(poses)
    add = np.array([got["frames"][n]["add"] for n in names])
    assert np.isinf(add[[4, 9]]).all() and np.isfinite(np.delete(add, [4, 9])).all()
    assert not got["frames"][names[4]]["ok"] and got["frames"][names[0]]["ok"]
    # the two failed frames count as 0 in the AUC and as misses in the accuracy, and are left out of the means
    part = np.maximum(0.0, 1.0 - np.delete(add, [4, 9]) / DIAMETER)
    assert got["auc_add"] == pytest.approx(part.sum() / 12, abs=1e-12) and got["auc_add"] <= 10 / 12
    assert got["add_mean"] == pytest.approx(np.delete(add, [4, 9]).mean(), abs=1e-15)
    assert got["acc_add"] == pytest.approx((add < 0.1 * DIAMETER).sum() / 12)
    assert got["auc_add_s"] == got["auc_add"] and got["auc_adds"] >= got["auc_add"]
    sym = E.evaluate_poses(poses, v4, device, symmetric=True, offset=True, max_distance=DIAMETER)
    assert sym["auc_add_s"] == sym["auc_adds"] == got["auc_adds"] and "acc_add" not in sym
    # without the alignment: the plain ADD of the stored (float32) poses
    plain = E.evaluate_poses(poses, r["v"], device, max_distance=DIAMETER)
    direct = []
    for k in range(12):
        if k not in (4, 9):
            A, B = (E.get_pose_mat_from_tensor(poses[names[k]][key]) for key in ("T_refined", "gt_pose"))
            direct.append(np.linalg.norm(r["v"] @ (A[:3, :3] - B[:3, :3]).T + (A[:3, 3] - B[:3, 3]), axis=1).mean())
    assert abs(plain["add_mean"] - np.mean(direct)) <= refs["bar"]


# ------------------------------------------------------------------------------------------------ 7. tracker
def test_a_tracked_sequence_is_scored(device, refs):
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames

    assets = make_tracking_assets(width=160, height=120, n_frames=6)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
    frames = render_query_frames(assets, tr.testbed)
    names = [f"{i:06d}.png" for i in range(6)]
    for name, frame in zip(names, frames):
        tr.run_single_frame((name, frame))
    torch.cuda.synchronize(device)
    history = tr.pose_history
    for name, (Rg, tg) in zip(names, assets["gt_poses"]):
        history[name]["gt_pose"] = Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg))
    pts = assets["model3d"].points3D
    v = np.stack([pts[i].xyz for i in sorted(pts)]).astype(np.float64)
    from scipy.spatial import ConvexHull
    from scipy.spatial.distance import pdist

    diameter = float(pdist(v[ConvexHull(v).vertices]).max())
    res = E.evaluate_poses(history, v, device, max_distance=diameter)
    assert res["n_frames"] == 6 and all(res["frames"][n]["ok"] for n in names), res
    assert res["n_success"] == 6 and 0 < res["auc_add"] <= 1 and res["auc_add"] <= res["auc_adds"] <= 1
    mats = [(E.get_pose_mat_from_tensor(history[n]["T_refined"]), E.get_pose_mat_from_tensor(history[n]["gt_pose"]))
            for n in names]
    with ThreadPoolExecutor(max_workers=6) as pool:  # (adds_distance takes seconds per frame on 5600 points)
        want = list(pool.map(lambda m: E.adds_distance(m[0], m[1], v), mats))
    got = np.array([res["frames"][n]["adds"] for n in names])
    bar = refs["bar"] / DIAMETER * diameter  # the bar is relative to the model's diameter
    print("ADD-S", got, "adds_distance", want, "diameter", diameter, "bar", bar, "auc", res["auc_add"], res["auc_adds"])
    assert np.abs(got - np.array(want)).max() <= bar
