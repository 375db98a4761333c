"""pxt_symmetric_pose_errors (csrc/pxt_eval_sym.hip) / torch.ops.pixtrack.symmetric_pose_errors and the evaluation API on
top of it: BOP's MSSD and MSPD of F frames over a set of S symmetry transforms, against a float64 oracle.

Oracle: float64 numpy straight from the BOP definitions - the model points are taken to the camera frame with T_est and
with T_gt S_s, their distance and the distance of their pinhole projections are maximised over the points, for every
(f, s).  It does not use the kernel's relative form (T_gt^-1 T_est, centred vertices), so it shares no algebra with it.

Inputs (test_pose_errors_gpu.py's generator): Gaussian clouds of seed 100 + V scaled to diameter 0.2 about the offset
point (0.31, -0.12, 0.45); T_gt a random rotation with t = (U(-.3, .3), U(-.3, .3), U(1.5, 3)); T_est = T_gt S[(7 f) mod S] D
with D <= 0.05 rad and <= 0.01 translation; frame 1 has T_est = T_gt exactly; intrinsics 600, 600, 319.5, 239.5; the sets
rotate about z (the flip: about x) through the offset point.

Bar (the project's convention): first the error of a float32 restatement of the kernel's form
(centred float32 vertices, float32 set and frames, elementwise float32 torch on the host: no FMA, IEEE division) against
the oracle is measured on these very inputs over every (f, s); the kernel may be 4 x that maximum off.  MSSD is expressed
against the diameter, MSPD in pixels.  Measured with the seeded inputs below: restatement MSSD 3.3e-08 (1.7e-07 of the
diameter), MSPD 2.0e-04 px -> bars 1.3e-07 (6.7e-07 of the diameter) and 8.2e-04 px.  The test recomputes and prints
them, and the kernel's own figures per case, before it asserts (pytest -s).  The kernel on the MI355X: MSSD 6.7e-09 at
most, MSPD 2.0e-04 px at most (the one-point case; 1.1e-05 ... 4.7e-05 px in the others).

Chosen symmetry: the index the kernel reports must, in the oracle, be within 2 bars of the minimum.  Neighbouring steps of
an axis set differ by very little, so the index itself is compared only for the discrete sets (whose margin in the
oracle is asserted to be far above the bar): there it is the oracle's argmin and the generator's (7 f) mod S."""
import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, evaluation as E, ops, symmetry as SY

pytestmark = pytest.mark.gpu

DIAMETER = 0.2
OFFSET = np.array([0.31, -0.12, 0.45])
KMAT = (600.0, 600.0, 319.5, 239.5)
IDENTITY_FRAME = 1
SENTINEL = -777.0
# name -> (set, V, F); the sets are built in _sets()
CASES = {
    "identity": ("identity", 1, 3),       # one lane, no min
    "c2": ("c2", 63, 3),                  # a partial wave
    "c4": ("c4", 257, 70),                # one past a block of 256; many frames
    "axis": ("axis", 1025, 24),           # S = 315: no multiple of 64; two tiles + 1
    "axis_flip": ("axis_flip", 300, 8),   # S = 630 > V; ten set chunks
    "c4_blocks": ("c4", 4099, 3),         # two vertex blocks, ragged tail
}
DISCRETE = ("identity", "c2", "c4", "c4_blocks")


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _about(axis, angle):
    R = _rot(axis, angle)
    return _T(R, OFFSET - R @ OFFSET)


def _sets():
    z = dict(axis=[0.0, 0.0, 1.0], offset=list(OFFSET))
    return {
        "identity": SY.symmetry_transforms(),
        "c2": SY.symmetry_transforms(discrete=[_about([0, 0, 1], np.pi)]),
        "c4": SY.symmetry_transforms(discrete=[_about([0, 0, 1], k * np.pi / 2) for k in (1, 2, 3)]),
        "axis": SY.symmetry_transforms(continuous=[z]),
        "axis_flip": SY.symmetry_transforms(discrete=[_about([1, 0, 0], np.pi)], continuous=[z]),
    }


def _cloud(V, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(V, 3))
    if V > 1:
        from scipy.spatial.distance import pdist

        p *= DIAMETER / pdist(p).max()
    return p + OFFSET


def _poses(F, seed, sym):
    rng = np.random.default_rng(seed)
    T_gt, T_est = [], []
    for f in range(F):
        g = _T(_rot(rng.normal(size=3), rng.uniform(0, np.pi)), np.r_[rng.uniform(-0.3, 0.3, 2), rng.uniform(1.5, 3.0)])
        d = rng.normal(size=3)
        D = _T(_rot(rng.normal(size=3), rng.uniform(0, 0.05)), d / np.linalg.norm(d) * rng.uniform(0, 0.01))
        T_gt.append(g)
        T_est.append(g.copy() if f == IDENTITY_FRAME else g @ sym[(7 * f) % len(sym)] @ D)
    return np.stack(T_est), np.stack(T_gt)


def _project64(p):
    with np.errstate(all="ignore"):
        px = np.stack([KMAT[0] * p[..., 0] / p[..., 2] + KMAT[2], KMAT[1] * p[..., 1] / p[..., 2] + KMAT[3]], axis=-1)
    return px, (p[..., 2] > 0) & np.isfinite(p[..., 2])


def _oracle(T_est, T_gt, v, sym):
    """float64 e3, e2 [F, S]: max_i |T_est v_i - T_gt S_s v_i| and the same after projection (+inf: a point not in front)."""
    e3, e2 = np.empty((len(T_est), len(sym))), np.empty((len(T_est), len(sym)))
    for f, (A, B) in enumerate(zip(T_est, T_gt)):
        a = v @ A[:3, :3].T + A[:3, 3]
        M = B[None] @ sym  # [S, 4, 4]
        g = np.einsum("sij,vj->svi", M[:, :3, :3], v) + M[:, None, :3, 3]
        e3[f] = np.linalg.norm(a[None] - g, axis=-1).max(axis=1)
        pa, oka = _project64(a)
        pg, okg = _project64(g)
        d2 = np.linalg.norm(pa[None] - pg, axis=-1)
        e2[f] = np.where(oka[None] & okg, d2, np.inf).max(axis=1)
    return e3, e2


def _restate32(u, syms12, frames40):
    """The kernel's form in elementwise float32 (torch on the host: IEEE float32, no FMA, division) -> e3, e2 [F, S]."""
    u, syms12, frames40 = torch.from_numpy(u), torch.from_numpy(syms12), torch.from_numpy(frames40)

    def apply(T, p):  # T [..., 12], p [..., V, 3] -> [..., V, 3]
        R, t = T[..., :9].reshape(*T.shape[:-1], 1, 3, 3), T[..., 9:].reshape(*T.shape[:-1], 1, 3)
        return p[..., 0:1] * R[..., 0] + p[..., 1:2] * R[..., 1] + p[..., 2:3] * R[..., 2] + t

    def project(p, K):
        return torch.stack([K[0] * (p[..., 0] / p[..., 2]) + K[2], K[1] * (p[..., 1] / p[..., 2]) + K[3]], dim=-1), \
            (p[..., 2] > 0) & torch.isfinite(p[..., 2])

    w = apply(syms12, u[None])  # [S, V, 3]
    e3, e2 = [], []
    for fr in frames40:
        rel, est, gt, K = fr[:12], fr[12:24], fr[24:36], fr[36:]
        a = apply(rel, u)
        pe, oke = project(apply(est, u), K)
        d3 = ((a[None] - w) ** 2).sum(-1).max(dim=1).values.sqrt()
        pg, okg = project(apply(gt, w), K)
        d2 = ((pe[None] - pg) ** 2).sum(-1)
        d2 = torch.where(oke[None] & okg, d2, torch.full_like(d2, float("inf"))).max(dim=1).values.sqrt()
        e3.append(d3.numpy().astype(np.float64))
        e2.append(d2.numpy().astype(np.float64))
    return np.stack(e3), np.stack(e2)


def build_refs():
    """Per case: cloud, set, poses, the kernel's inputs, the oracle's e3 / e2 [F, S], the restatement; and the two bars."""
    sets = _sets()
    out, worst3, worst2 = {}, 0.0, 0.0
    for name, (set_name, V, F) in CASES.items():
        sym = sets[set_name]
        v = _cloud(V, 100 + V)
        T_est, T_gt = _poses(F, 200 + V, sym)
        c = v.mean(axis=0)
        u = (v - c).astype(np.float32)
        syms12 = SY.centred_12(sym, c).astype(np.float32)
        frames40 = E.symmetric_frames(T_est, T_gt, c, np.tile(KMAT, (F, 1)))
        e3, e2 = _oracle(T_est, T_gt, v, sym)
        assert np.isfinite(e3).all() and np.isfinite(e2).all()
        r3, r2 = _restate32(u, syms12, frames40)
        worst3, worst2 = max(worst3, float(np.abs(r3 - e3).max())), max(worst2, float(np.abs(r2 - e2).max()))
        out[name] = dict(v=v, sym=sym, T_est=T_est, T_gt=T_gt, u=u, syms12=syms12, frames40=frames40, e3=e3, e2=e2)
    out["bar3"], out["bar2"] = 4.0 * worst3, 4.0 * worst2
    print(f"float32 restatement: MSSD max {worst3:.3e} ({worst3 / DIAMETER:.3e} of the diameter), MSPD max {worst2:.3e} px; "
          f"bars {4 * worst3:.3e} ({4 * worst3 / DIAMETER:.3e}) and {4 * worst2:.3e} px")
    # float32 on object-sized numbers and on pixel coordinates of a few hundred: far below any error of interest
    assert 0 < out["bar3"] < 1e-5 * DIAMETER and 0 < out["bar2"] < 1e-2
    return out


@pytest.fixture(scope="module")
def refs():
    return build_refs()


def _run(device, u, syms12, frames40, records=None):
    """One call of the op on host arrays; -> the records tensor (device)."""
    verts = torch.from_numpy(np.ascontiguousarray(u, np.float32)).to(device)
    syms = torch.from_numpy(np.ascontiguousarray(syms12, np.float32)).to(device)
    frames = torch.from_numpy(np.ascontiguousarray(frames40, np.float32)).to(device)
    F, S, V = len(frames40), len(syms12), len(u)
    if records is None:
        records = torch.full((F, 8), SENTINEL, device=device)
    ws = torch.empty(int(_lib.lib().pxt_symmetric_pose_errors_workspace_bytes(F, S, V)), dtype=torch.uint8, device=device)
    ops.ops.symmetric_pose_errors(verts, syms, frames, records, ws)
    return records


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", list(CASES))
def test_records_match_the_float64_oracle(device, refs, case):
    r = refs[case]
    F, S, V = len(r["frames40"]), len(r["sym"]), len(r["u"])
    rec = _run(device, r["u"], r["syms12"], r["frames40"]).cpu().numpy().astype(np.float64)
    e3, e2, bar3, bar2 = r["e3"], r["e2"], refs["bar3"], refs["bar2"]
    err3, err2 = np.abs(rec[:, 0] - e3.min(axis=1)), np.abs(rec[:, 2] - e2.min(axis=1))
    print(f"{case} (S {S}, V {V}, F {F}): MSSD max error {err3.max():.3e} = {err3.max() / DIAMETER:.3e} of the diameter "
          f"(bar {bar3:.3e}); MSPD max error {err2.max():.3e} px (bar {bar2:.3e})")
    assert (rec[:, 7] == 1.0).all() and (rec[:, 4] == V).all() and (rec[:, 5] == S).all() and (rec[:, 6] == 0.0).all()
    assert err3.max() <= bar3, (err3, bar3)
    assert err2.max() <= bar2, (err2, bar2)
    # the chosen symmetries: whole numbers inside the set, and as good as the best in the oracle (no frame is skipped)
    i3, i2 = rec[:, 1].astype(np.int64), rec[:, 3].astype(np.int64)
    assert (i3 == rec[:, 1]).all() and (i2 == rec[:, 3]).all() and (0 <= i3).all() and (i3 < S).all() \
        and (0 <= i2).all() and (i2 < S).all()
    rows = np.arange(F)
    assert (e3[rows, i3] <= e3.min(axis=1) + 2 * bar3).all()
    assert (e2[rows, i2] <= e2.min(axis=1) + 2 * bar2).all()
    if case in DISCRETE:
        want = (7 * rows) % S
        want[IDENTITY_FRAME] = 0
        if S > 1:  # the runner-up is far away in the oracle, so the index is no matter of rounding
            margin3 = np.sort(e3, axis=1)[:, 1] - e3.min(axis=1)
            margin2 = np.sort(e2, axis=1)[:, 1] - e2.min(axis=1)
            print(f"   margins: MSSD {margin3.min():.3e}, MSPD {margin2.min():.3e} px")
            assert margin3.min() > 1000 * bar3 and margin2.min() > 1000 * bar2
        np.testing.assert_array_equal(e3.argmin(axis=1), want)
        np.testing.assert_array_equal(e2.argmin(axis=1), want)
        np.testing.assert_array_equal(i3, want)
        np.testing.assert_array_equal(i2, want)
    # T_est = T_gt: MSSD is +0.0 exactly, MSPD within the bar, both at the identity
    assert _bits(torch.tensor(rec[IDENTITY_FRAME, 0], dtype=torch.float32)).item() == 0
    assert rec[IDENTITY_FRAME, 2] <= bar2 and rec[IDENTITY_FRAME, 1] == 0.0 and rec[IDENTITY_FRAME, 3] == 0.0


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_a_record_depends_on_its_own_frame_only(device, refs):
    r = refs["c4"]
    base = _bits(_run(device, r["u"], r["syms12"], r["frames40"]))
    for k in (0, 1, 33, 69):
        alone = _bits(_run(device, r["u"], r["syms12"], r["frames40"][k:k + 1]))
        assert torch.equal(alone, base[k:k + 1]), k
        moved = _bits(_run(device, r["u"], r["syms12"], r["frames40"][[5, 6, k]]))
        assert torch.equal(moved[2], base[k]), k
    r = refs["axis"]  # several set chunks and tiles
    base = _bits(_run(device, r["u"], r["syms12"], r["frames40"]))
    perm = np.random.default_rng(9).permutation(len(base))
    assert torch.equal(_bits(_run(device, r["u"], r["syms12"], r["frames40"][perm])), base[perm])
    assert torch.equal(_bits(_run(device, r["u"], r["syms12"], r["frames40"][7:8])), base[7:8])


def test_a_side_stream_gives_the_same_bits(device, refs):
    r = refs["axis_flip"]
    base = _bits(_run(device, r["u"], r["syms12"], r["frames40"]))
    main, side = torch.cuda.current_stream(device), torch.cuda.Stream(device=device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = _run(device, r["u"], r["syms12"], r["frames40"])
    side.synchronize()
    assert torch.equal(_bits(out), base)


# ------------------------------------------------------------------------------------------------ 3. bad frames
def test_a_non_finite_frame_marks_its_record_only(device, refs):
    r = refs["axis"]
    frames = r["frames40"][:5].copy()
    base = _bits(_run(device, r["u"], r["syms12"], frames))
    for word, value in ((4, np.nan), (21, np.inf), (35, -np.inf), (37, np.nan)):
        bad = frames.copy()
        bad[2, word] = value
        rec = _run(device, r["u"], r["syms12"], bad).cpu()
        assert rec[2, 7] == -1.0 and (rec[2, :7] == SENTINEL).all(), word
        keep = [0, 1, 3, 4]
        assert torch.equal(_bits(rec)[keep], base[keep]), word


def test_an_estimate_behind_the_camera_has_no_projection_distance(device, refs):
    r = refs["c2"]
    v, sym = r["v"], r["sym"]
    T_gt = r["T_gt"][:3]
    T_est = T_gt.copy()
    T_est[0, 2, 3] = -2.0  # the whole object behind the camera
    T_est[2] = r["T_est"][2]
    T_gt = T_gt.copy()
    T_gt[1, 2, 3] = -2.0  # frame 1: the ground truth behind the camera, the estimate in front of it
    c = v.mean(axis=0)
    frames = E.symmetric_frames(T_est, T_gt, c, np.tile(KMAT, (3, 1)))
    rec = _run(device, r["u"], r["syms12"], frames).cpu().numpy().astype(np.float64)
    e3, e2 = _oracle(T_est, T_gt, v, sym)
    assert np.isinf(e2[:2]).all() and np.isfinite(e2[2]).all() and np.isfinite(e3).all()
    assert rec[1, 2] == np.inf and rec[1, 3] == 0.0 and np.isfinite(rec[1, 0])
    assert rec[0, 2] == np.inf and rec[0, 3] == 0.0 and rec[0, 7] == 1.0  # every symmetry ties at +inf: the lowest index
    # a distance of many diameters: float32 relative to the value (the bars belong to object-sized distances)
    assert np.isfinite(rec[0, 0]) and abs(rec[0, 0] - e3[0].min()) <= 1e-6 * e3[0].min()
    assert np.isfinite(rec[2, 2]) and abs(rec[2, 2] - e2[2].min()) <= refs["bar2"]


def test_invalid_arguments_change_nothing(device, refs):
    r = refs["c2"]
    L = _lib.lib()
    verts, syms, frames = (torch.from_numpy(r[k]).to(device) for k in ("u", "syms12", "frames40"))
    rec = torch.full((3, 8), SENTINEL, device=device)
    need = int(L.pxt_symmetric_pose_errors_workspace_bytes(3, 2, 63))
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device=device)
    assert 0 < need <= 4096
    # through the op
    bad = (lambda: ops.ops.symmetric_pose_errors(verts[:0], syms, frames, rec, ws),                     # V = 0
           lambda: ops.ops.symmetric_pose_errors(verts, syms[:0], frames, rec, ws),                      # S = 0
           lambda: ops.ops.symmetric_pose_errors(verts, syms, frames[:0], rec[:0], ws),                  # F = 0
           lambda: ops.ops.symmetric_pose_errors(verts, syms, frames, rec, ws[:need - 1]),               # a small workspace
           lambda: ops.ops.symmetric_pose_errors(verts, syms, frames, rec[:2], ws),                      # records' shape
           lambda: ops.ops.symmetric_pose_errors(verts, syms, frames[:, :39], rec, ws),                  # frames' shape
           lambda: ops.ops.symmetric_pose_errors(verts, syms[:, :11], frames, rec, ws),                  # not contiguous
           lambda: ops.ops.symmetric_pose_errors(verts, syms, frames, rec, ws.cpu()),                    # host memory
           lambda: ops.ops.symmetric_pose_errors(verts, syms.double(), frames, rec, ws),                 # dtype
           lambda: ops.ops.symmetric_pose_errors(verts, torch.zeros(1025, 12, device=device), frames, rec,
                                                 torch.empty(1 << 20, dtype=torch.uint8, device=device)),  # S = 1025
           lambda: ops.ops.symmetric_pose_errors(verts, syms, torch.zeros(65536, 40, device=device),
                                                 torch.zeros(65536, 8, device=device),
                                                 torch.empty(65536 * 16, dtype=torch.uint8, device=device)),  # F = 65536
           lambda: ops.ops.symmetric_pose_errors(torch.zeros((1 << 20) + 1, 3, device=device), syms, frames, rec,
                                                 torch.empty(1 << 20, dtype=torch.uint8, device=device)))  # V = 2^20 + 1
    for k, call in enumerate(bad):
        with pytest.raises(_lib.PxtError):
            call()
    # the entry point's own checks (nothing is launched)
    s = _lib.stream_ptr(device)
    a = (verts.data_ptr(), 63, syms.data_ptr(), 2, frames.data_ptr(), 3, rec.data_ptr(), ws.data_ptr(), s)

    def call(**kw):
        args = list(a)
        for i, val in kw.items():
            args[int(i[1:])] = val
        return L.pxt_symmetric_pose_errors(*args)

    for kw in (dict(_1=0), dict(_1=(1 << 20) + 1), dict(_3=0), dict(_3=1025), dict(_5=0), dict(_5=65536), dict(_0=None),
               dict(_2=None), dict(_4=None), dict(_6=None), dict(_7=None), dict(_0=verts.data_ptr() + 2),
               dict(_2=syms.data_ptr() + 1), dict(_4=frames.data_ptr() + 2), dict(_6=rec.data_ptr() + 2),
               dict(_7=ws.data_ptr() + 1)):
        assert call(**kw) == -1, kw  # PXT_E_ARG
        with pytest.raises(_lib.PxtError):
            _lib.check(call(**kw), "pxt_symmetric_pose_errors")
    torch.cuda.synchronize(device)
    assert (rec == SENTINEL).all() and (ws == 0xA5).all()
    assert call() == 0
    torch.cuda.synchronize(device)
    assert (rec[:, 7] == 1.0).all()


# ------------------------------------------------------------------------------------------------ 4. host wrapper, scoreboard
def test_symmetric_pose_errors_is_the_raw_op(device, refs):
    from pixtrack_amd.geometry import Camera

    r = refs["axis_flip"]
    rec = _run(device, r["u"], r["syms12"], r["frames40"]).cpu().numpy()
    F = len(rec)
    cam = Camera(torch.tensor([640.0, 480.0, *KMAT]))
    for cameras in (cam, [cam] * F, np.array(KMAT), np.tile(KMAT, (F, 1))):
        res = E.symmetric_pose_errors(r["T_est"], r["T_gt"], np.c_[r["v"], np.ones(len(r["v"]))], cameras, r["sym"], device)
        np.testing.assert_array_equal(res["mssd"].astype(np.float32).view(np.uint32), rec[:, 0].view(np.uint32))
        np.testing.assert_array_equal(res["mspd"].astype(np.float32).view(np.uint32), rec[:, 2].view(np.uint32))
        np.testing.assert_array_equal(res["mssd_sym"], rec[:, 1].astype(np.int64))
        np.testing.assert_array_equal(res["mspd_sym"], rec[:, 3].astype(np.int64))
        assert res["ok"].all() and res["ok"].dtype == bool
    # no set: the identity only, which is element 0 of every set
    plain = E.symmetric_pose_errors(list(r["T_est"]), list(r["T_gt"]), r["v"], cam, None, device)
    assert np.abs(plain["mssd"] - r["e3"][:, 0]).max() <= refs["bar3"] and (plain["mssd_sym"] == 0).all()
    assert np.abs(plain["mspd"] - r["e2"][:, 0]).max() <= refs["bar2"]  # (the bars were taken over every (f, s))
    bad = r["T_est"].copy()
    bad[3, 0, 0] = np.nan
    res = E.symmetric_pose_errors(bad, r["T_gt"], r["v"], cam, r["sym"], device)
    assert not res["ok"][3] and np.isnan(res["mssd"][3]) and res["mssd_sym"][3] == -1 and res["ok"].sum() == F - 1


def test_the_bop_scoreboard_needs_the_symmetry_set(device, refs):
    from pixtrack_amd.geometry import Camera, Pose

    r = refs["c4"]
    F = len(r["T_est"])
    cam = Camera(torch.tensor([640.0, 480.0, *KMAT]))
    poses = {f"{k:06d}.png": dict(T_refined=Pose.from_4x4mat(torch.from_numpy(r["T_est"][k]).float()),
                                  gt_pose=Pose.from_4x4mat(torch.from_numpy(r["T_gt"][k]).float()),
                                  success=k != 4, camera=None if k == 9 else cam) for k in range(F)}
    names = list(poses)
    turned = np.array([(7 * k) % 4 != 0 and k != IDENTITY_FRAME for k in range(F)])
    lost = np.zeros(F, bool)
    lost[[4, 9]] = True
    # float64: without the set a turned frame is off by more than half the diameter; with it no frame is
    assert (r["e3"][turned, 0] > 0.5 * DIAMETER).all() and (r["e3"].min(axis=1) < 0.5 * DIAMETER).all()
    plain = E.evaluate_poses_bop(poses, r["v"], device, DIAMETER)
    full = E.evaluate_poses_bop(poses, r["v"], device, DIAMETER, symmetries=r["sym"], ar_vsd=0.25)
    mssd_plain = np.array([plain["frames"][n]["mssd"] for n in names])
    mssd_full = np.array([full["frames"][n]["mssd"] for n in names])
    np.testing.assert_array_equal(mssd_plain < 0.5 * DIAMETER, ~turned & ~lost)
    np.testing.assert_array_equal(mssd_full < 0.5 * DIAMETER, ~lost)
    assert np.isinf(mssd_full[lost]).all() and np.isinf([full["frames"][names[k]]["mspd"] for k in (4, 9)]).all()
    assert not full["frames"][names[4]]["ok"] and full["frames"][names[4]]["mssd_sym"] == -1
    assert [full["frames"][n]["mssd_sym"] for n in names[:4]] == [0, 0, 2, 1]
    assert plain["n_frames"] == full["n_frames"] == F and full["n_evaluated"] == F - 2 and full["n_symmetries"] == 4
    assert plain["n_symmetries"] == 1 and "ar_bop" not in plain
    assert full["ar_mssd"] == pytest.approx(E.recall_mssd(mssd_full, DIAMETER)) and full["ar_mssd"] > plain["ar_mssd"]
    assert full["ar_mspd"] > plain["ar_mspd"] and 0 < full["ar_mspd"] <= (F - 2) / F
    assert full["ar_bop"] == pytest.approx((0.25 + full["ar_mssd"] + full["ar_mspd"]) / 3, abs=1e-15)
    assert full["mssd_mean"] == pytest.approx(mssd_full[~lost].mean(), abs=1e-15)
    # (the stored poses are float32: the figures differ from the float64 inputs' by that rounding of a pose, not by a bar)
    assert np.abs(mssd_full[~lost] - r["e3"].min(axis=1)[~lost]).max() < 1e-5


# ------------------------------------------------------------------------------------------------ 5. command lines
def test_both_command_lines_add_the_bop_keys_on_request(device, tmp_path, capsys):
    import json

    from pixtrack_amd import render_evaluation as RE
    from pixtrack_amd.geometry import Pose
    from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9
    from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames, write_object_dir
    from pixtrack_amd.utils.io import dump_reference_pickle

    N = 4
    assets = make_tracking_assets(width=160, height=120, n_frames=N)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=device, assets=assets)
    names = [f"{i:06d}.png" for i in range(N)]
    for name, frame in zip(names, render_query_frames(assets, tr.testbed)):
        tr.run_single_frame((name, frame))
    torch.cuda.synchronize(device)
    for name, (Rg, tg) in zip(names, assets["gt_poses"]):
        tr.pose_history[name]["gt_pose"] = Pose.from_Rt(torch.from_numpy(Rg), torch.from_numpy(tg))
    pts = assets["model3d"].points3D
    v = np.stack([pts[i].xyz for i in sorted(pts)]).astype(np.float64)
    d = RE.bounding_box_diagonal(assets["model3d"])
    obj = tmp_path / "object"
    write_object_dir(assets, obj)
    dump_reference_pickle(tr.pose_history, str(tmp_path / "poses.pkl"))
    np.save(tmp_path / "v.npy", v)
    # a half turn about z through the centroid, in units of 1000 per model unit (as BOP's millimetres to metres)
    c = v.mean(axis=0) * 1000.0
    (tmp_path / "info.json").write_text(json.dumps({"3": {"diameter": d * 1000.0, "symmetries_discrete": [
        [-1, 0, 0, 2 * c[0], 0, -1, 0, 2 * c[1], 0, 0, 1, 0, 0, 0, 0, 1]]}}))
    base = ["--poses", str(tmp_path / "poses.pkl"), "--device", str(device)]
    bop = ["--bop", "--models_info", str(tmp_path / "info.json"), "--obj_id", "3", "--models_info_scale", "0.001"]

    plain = E.main(base + ["--vertices", str(tmp_path / "v.npy")])
    capsys.readouterr()
    full = E.main(base + ["--vertices", str(tmp_path / "v.npy"), "--diameter", str(d), "--json", str(tmp_path / "e.json")] + bop)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    added = {"n_symmetries", "diameter", "mssd_mean", "mspd_mean", "ar_mssd", "ar_mspd"}
    assert set(full) - set(plain) == added and not (set(plain) & added) and "ar_bop" not in line
    assert {k: full[k] for k in plain if k != "frames"} == {k: plain[k] for k in plain if k != "frames"}
    assert line["n_symmetries"] == 2 and line["n_evaluated"] == N and "frames" not in line
    want = E.symmetric_pose_errors([tr.pose_history[n]["T_refined"] for n in names],
                                   [tr.pose_history[n]["gt_pose"] for n in names], v,
                                   [tr.pose_history[n]["camera"] for n in names], None, device)
    got = [full["frames"][n] for n in names]
    # a tracked frame is nearest to the identity, so the set changes nothing here; the figures are the plain call's
    assert [g["mssd"] for g in got] == list(want["mssd"]) and [g["mssd_sym"] for g in got] == [0] * N
    assert 0 < line["mssd_mean"] < np.inf and 0 < line["mspd_mean"] < np.inf
    assert 0 <= line["ar_mssd"] <= 1 and 0 <= line["ar_mspd"] <= 1
    print("tracked run:", {k: line[k] for k in sorted(added)})
    assert {"add", "adds", "mssd", "mspd", "mssd_sym", "mspd_sym", "ok"} <= set(json.loads((tmp_path / "e.json").read_text())["frames"][names[0]])

    aabb = json.dumps([[float(x) for x in corner] for corner in assets["aabb"]])
    rbase = base + ["--object_path", str(obj), "--obj_aabb", aabb]
    rplain = RE.main(rbase)
    capsys.readouterr()
    rfull = RE.main(rbase + bop)  # the SfM points are the point set, the box diagonal the diameter
    rline = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(rfull) - set(rplain) == {"n_symmetries", "mssd_mean", "mspd_mean", "ar_mssd", "ar_mspd", "ar_bop"}
    assert {k: rfull[k] for k in rplain if k != "frames"} == {k: rplain[k] for k in rplain if k != "frames"}
    assert rline["ar_bop"] == pytest.approx((rline["ar_vsd"] + rline["ar_mssd"] + rline["ar_mspd"]) / 3, abs=1e-15)
    # (the object directory holds the points in float32: the same figures up to that rounding of the point set)
    assert rline["mssd_mean"] == pytest.approx(line["mssd_mean"], rel=1e-3)
    assert "vsd" in rfull["frames"][names[0]] and "mspd" in rfull["frames"][names[0]]
