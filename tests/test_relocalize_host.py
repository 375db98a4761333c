"""CPU checks of the relocaliser (pixtrack_amd/relocalizer.py, pxt_score_pose_hypotheses): the hypothesis generator,
the ranking formula, the C-ABI records against the header and the op's registration (no GPU needed)."""
import ctypes
import math
import subprocess
import tempfile
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib, ops
from pixtrack_amd.relocalizer import (make_hypotheses, rank_scores, robust_rho, shift_pixels, top_candidates)
from pixtrack_amd.synthetic import look_at_pose

ROOT = Path(__file__).resolve().parent.parent


def _views(n=5, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        centre = rng.normal(size=3) * 0.05
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        R, t = look_at_pose(centre + d * rng.uniform(0.4, 0.8), centre)
        out.append((R, t, centre))
    return out


def _camera10(w=640, h=480, f=768.0):
    return [w, h, f, f, w / 2 - 0.5, h / 2 - 0.5, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("rolls,shifts", [(24, 1), (7, 1), (5, 3), (1, 2)])
def test_hypothesis_count(rolls, shifts):
    views = _views()
    poses, owner = make_hypotheses(views, rolls, shifts, _camera10())
    assert poses.shape == (len(views) * rolls * shifts * shifts, 12)
    assert owner.shape == (poses.shape[0],)
    per = rolls * shifts * shifts
    assert (owner == np.repeat(np.arange(len(views)), per)).all()


def test_roll_zero_is_the_db_pose_exactly():
    views = _views()
    poses, _ = make_hypotheses(views, 24)
    for k, (R, t, _) in enumerate(views):
        p = poses[k * 24]
        assert np.array_equal(p[:9], R.reshape(-1)) and np.array_equal(p[9:], t)


def test_roll_keeps_camera_centre_and_optical_axis():
    views = _views()
    rolls = 12
    poses, owner = make_hypotheses(views, rolls)
    for p, o in zip(poses, owner):
        R, t = p[:9].reshape(3, 3), p[9:]
        Rv, tv, _ = views[o]
        np.testing.assert_allclose(-R.T @ t, -Rv.T @ tv, atol=1e-12)   # camera centre
        np.testing.assert_allclose(R[2], Rv[2], atol=1e-12)             # optical axis (third row: camera z in world)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    # the rolls are evenly spaced about the axis
    R1 = poses[1][:9].reshape(3, 3)
    Rv = views[0][0]
    ang = math.atan2((R1 @ Rv.T)[1, 0], (R1 @ Rv.T)[0, 0])
    assert abs(ang - 2 * math.pi / rolls) < 1e-12


def test_shift_puts_the_object_centre_on_the_requested_pixel():
    views = _views()
    cam = _camera10()
    shifts, rolls = 3, 4
    poses, owner = make_hypotheses(views, rolls, shifts, cam)
    targets = shift_pixels(cam, shifts)
    assert len(targets) == shifts * shifts
    fx, fy, cx, cy = cam[2:6]
    for i, (p, o) in enumerate(zip(poses, owner)):
        R, t = p[:9].reshape(3, 3), p[9:]
        c = R @ views[o][2] + t
        u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
        tu, tv = targets[i % (shifts * shifts)]
        assert abs(u - tu) < 1e-9 and abs(v - tv) < 1e-9
        # the depth of the centre is the rolled view's
        Rr = poses[(i // (shifts * shifts)) * (shifts * shifts)][:9].reshape(3, 3)
        assert np.array_equal(R, Rr)


def test_ranking_formula_on_hand_made_sums():
    rho2 = robust_rho(2, 0.0, 0.1, 2.0)
    assert rho2 == pytest.approx(0.01 * 2.0 * math.log1p(0.5 * 2.0 / 0.01))
    out = torch.tensor([[5.0, 50.0, 0, 0],     # all points valid
                        [4.0, 10.0, 0, 0],     # few valid: the 40 missing ones cost rho(2) each
                        [0.0, 9.0, 0, 0],      # below min_valid: last whatever its sum
                        [8.0, 50.0, 0, 0],
                        [0.0, 0.0, 0, 0]])     # nothing valid
    counts = torch.tensor([50, 50, 50, 50, 50], dtype=torch.int32)
    s = rank_scores(out, counts, rho2, 10)
    assert s[0].item() == pytest.approx(5.0 / 50)
    assert s[1].item() == pytest.approx((4.0 + 40 * rho2) / 50)  # 0.154: behind row 0, ahead of row 3
    assert math.isinf(s[2].item()) and math.isinf(s[4].item())
    assert s[3].item() == pytest.approx(8.0 / 50)
    assert top_candidates(s, 3).tolist() == [0, 1, 3]
    assert top_candidates(s, 16).tolist() == [0, 1, 3, 2, 4]  # ties (inf) in index order


def test_robust_rho_matches_the_oracle_losses():
    from oracle import lm_oracle as LO

    for kind, name, alpha in ((0, "squared", 2.0), (1, "huber", 0.0), (2, "barron", 0.0), (2, "barron", 1.0), (2, "barron", -2.0)):
        fn = LO.make_loss(name, alpha, 0.1) if name != "squared" else LO.make_loss(name)
        for x in (0.0, 0.004, 0.5, 2.0):
            want = float(fn(torch.tensor([x], dtype=torch.float64))[0][0])
            assert robust_rho(kind, alpha, 0.1 if kind else 1.0, x) == pytest.approx(want, rel=1e-9, abs=1e-15)


def test_reloc_struct_sizes_match_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "pixtrack_hip.h"
        int main(void) {
          printf("%zu %zu %zu %zu\\n", sizeof(pxt_reloc_map), sizeof(pxt_reloc_bank), offsetof(pxt_reloc_map, cam),
                 offsetof(pxt_reloc_bank, n_points));
          return 0;
        }
        """
    )
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = [int(x) for x in subprocess.check_output([str(Path(d) / "s")]).decode().split()]
    assert got == [ctypes.sizeof(_lib.RelocMap), ctypes.sizeof(_lib.RelocBank), _lib.RelocMap.cam.offset,
                   _lib.RelocBank.n_points.offset]


def test_binding_and_op_exist():
    assert "pxt_score_pose_hypotheses" in _lib.PROTOTYPES
    assert "score_pose_hypotheses" in ops.op_names()
    s = str(torch.ops.pixtrack.score_pose_hypotheses.default._schema)
    assert "Tensor(a!) out" in s and "Tensor poses" in s and "Tensor ranges" in s


def test_op_is_cuda_only_and_refuses_host_tensors():
    fmap = torch.zeros(4, 4, 132)
    with pytest.raises(NotImplementedError):
        torch.ops.pixtrack.score_pose_hypotheses(fmap, 128, [4.0, 4.0, 1, 1, 0, 0, 0, 0, 0, 0], 0, torch.zeros(3, 3),
                                                 torch.zeros(3, 132), None, torch.zeros(2, 12),
                                                 torch.zeros(2, 2, dtype=torch.int32), 1, 2, 0.0, 0.1, torch.zeros(2, 4))


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 13
    assert _lib.lib().pxt_version() == 13
