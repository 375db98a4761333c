"""Symmetry sets (pixtrack_amd/symmetry.py): sizes and order, the rule of a continuous axis, what is refused, the
models_info.json reader.  No GPU."""
from pathlib import Path

import numpy as np
import pytest

from pixtrack_amd import symmetry as SY

GOLDEN = Path(__file__).resolve().parent / "golden"
Z = [0.0, 0.0, 1.0]


def _T(R, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _cn(n):
    return [_T(SY.rotation(Z, 2 * np.pi * k / n)) for k in range(1, n)]


def test_set_sizes_and_order():
    flip = _T(SY.rotation([1, 0, 0], np.pi))
    sets = {"none": SY.symmetry_transforms(), "c2": SY.symmetry_transforms(_cn(2)), "c4": SY.symmetry_transforms(_cn(4)),
            "axis": SY.symmetry_transforms(continuous=[dict(axis=Z, offset=[0, 0, 0])]),
            "axis_flip": SY.symmetry_transforms([flip], [dict(axis=Z, offset=[0, 0, 0])])}
    assert [len(s) for s in sets.values()] == [1, 2, 4, 315, 630]
    for name, s in sets.items():
        assert s.dtype == np.float64 and s.shape[1:] == (4, 4)
        np.testing.assert_array_equal(s[0], np.eye(4), err_msg=name)  # the identity, exactly, is element 0
        np.testing.assert_array_equal(s[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(s), 1)))
        assert np.abs(np.transpose(s[:, :3, :3], (0, 2, 1)) @ s[:, :3, :3] - np.eye(3)).max() < 1e-12
    # the discrete list is [I] + discrete, in the order given
    np.testing.assert_array_equal(sets["c4"][1:], np.stack(_cn(4)))
    # element k of an axis set turns by 2 pi k / 315
    for k in (1, 2, 157, 314):
        np.testing.assert_allclose(sets["axis"][k, :3, :3], SY.rotation(Z, 2 * np.pi * k / 315), atol=1e-15)
    # continuous outer, discrete inner: element 2 k is the bare rotation, 2 k + 1 the rotation times the flip
    np.testing.assert_array_equal(sets["axis_flip"][0::2], sets["axis"])
    np.testing.assert_allclose(sets["axis_flip"][1::2], sets["axis"] @ flip, atol=1e-15)
    np.testing.assert_array_equal(sets["axis_flip"][1], flip)
    # 16 row-major floats are a matrix too; max_step sets the number of steps
    assert np.array_equal(SY.symmetry_transforms([list(_cn(2)[0].reshape(-1))]), sets["c2"])
    assert len(SY.symmetry_transforms(continuous=[dict(axis=Z)], max_step=0.1)) == 32  # ceil(pi / 0.1)


def test_a_rotation_about_an_offset_axis_keeps_the_offset_point():
    offset = np.array([0.31, -0.12, 0.45])
    s = SY.symmetry_transforms(continuous=[dict(axis=[0.2, -1.0, 0.5], offset=list(offset))])
    moved = s[:, :3, :3] @ offset + s[:, :3, 3]
    assert np.abs(moved - offset).max() < 1e-15
    axis = np.array([0.2, -1.0, 0.5]) / np.linalg.norm([0.2, -1.0, 0.5])
    on_axis = offset + 0.7 * axis  # every point of the axis stays
    assert np.abs(s[:, :3, :3] @ on_axis + s[:, :3, 3] - on_axis).max() < 1e-15
    assert np.linalg.norm(s[100, :3, :3] @ (offset + [0.1, 0, 0]) + s[100, :3, 3] - (offset + [0.1, 0, 0])) > 0.05


def test_what_is_refused():
    R = SY.rotation(Z, 0.3)
    for bad in (_T(1.001 * R), _T(R + 1e-5), _T(np.diag([1.0, 1.0, -1.0])), _T(R, (np.nan, 0, 0)), _T(np.full((3, 3), np.inf)),
                np.eye(3), list(range(15))):
        with pytest.raises(ValueError):
            SY.symmetry_transforms([bad])
    SY.symmetry_transforms([_T(R + 1e-8)])  # inside the tolerance of 1e-6
    for entry in (dict(axis=[0, 0, 0]), dict(axis=[0, np.nan, 1]), dict(axis=Z, offset=[0, np.inf, 0]), dict(axis=[0, 1])):
        with pytest.raises(ValueError):
            SY.symmetry_transforms(continuous=[entry])
    for step in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            SY.symmetry_transforms(continuous=[dict(axis=Z)], max_step=step)
    # more than 1024 transforms: 315 x 4, two axes x 315 x 2, a fine step
    for kw in (dict(discrete=_cn(4), continuous=[dict(axis=Z)]),
               dict(discrete=_cn(2), continuous=[dict(axis=Z), dict(axis=[1, 0, 0])]),
               dict(continuous=[dict(axis=Z)], max_step=0.003), dict(discrete=_cn(1026))):
        with pytest.raises(ValueError):
            SY.symmetry_transforms(**kw)
    assert len(SY.symmetry_transforms(discrete=_cn(1024))) == 1024
    assert len(SY.symmetry_transforms(continuous=[dict(axis=Z)], max_step=0.00307)) == 1024  # ceil(1023.3)


def test_centred_transforms_move_centred_points_alike():
    rng = np.random.default_rng(0)
    c = np.array([0.4, -1.2, 2.5])
    s = SY.symmetry_transforms([_T(SY.rotation([1, 2, 3], 1.0), (0.1, 0.2, -0.3))], [dict(axis=Z, offset=[0.3, 0.1, 0.0])],
                               max_step=0.5)
    s12 = SY.centred_12(s, c)
    assert s12.shape == (len(s), 12) and s12.dtype == np.float64
    np.testing.assert_array_equal(s12[0], np.r_[np.eye(3).reshape(-1), np.zeros(3)])
    v = rng.normal(size=(20, 3)) + c
    for T, row in zip(s, s12):
        want = v @ T[:3, :3].T + T[:3, 3] - c
        got = (v - c) @ row[:9].reshape(3, 3).T + row[9:]
        assert np.abs(got - want).max() < 1e-14


def test_models_info_reader():
    whole = GOLDEN / "bop_models_info.json"
    plain = SY.read_models_info(whole, 1)
    assert plain["diameter"] == 172.063 and plain["symmetries"].shape == (1, 4, 4)
    axis = SY.read_models_info(whole, obj_id=5)
    assert axis["diameter"] == 201.5 and axis["symmetries"].shape == (315, 4, 4)
    disc = SY.read_models_info(str(whole), 12)
    assert disc["symmetries"].shape == (2, 4, 4)
    np.testing.assert_array_equal(disc["symmetries"][1], np.array([[-1, 0, 0, 4.0], [0, -1, 0, -2.0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    with pytest.raises(ValueError):  # several objects and no obj_id
        SY.read_models_info(whole)
    with pytest.raises(KeyError):
        SY.read_models_info(whole, 7)
    one = SY.read_models_info(GOLDEN / "bop_models_info_one_object.json")
    assert one["diameter"] == 98.5 and one["symmetries"].shape == (630, 4, 4)  # units of the file: nothing is converted
    np.testing.assert_array_equal(one["symmetries"][1, :3, 3], [0.0, 0.0, 6.0])
    offset = np.array([1.0, 2.0, 3.0])
    assert np.abs(one["symmetries"][0::2, :3, :3] @ offset + one["symmetries"][0::2, :3, 3] - offset).max() < 1e-14
    assert SY.read_models_info(GOLDEN / "bop_models_info_one_object.json", obj_id=3)["diameter"] == 98.5  # obj_id unused
