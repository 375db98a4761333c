"""Symmetry sets of an object, from the ``symmetries_discrete`` / ``symmetries_continuous`` fields of a BOP
``models_info.json``: the finite set of rigid transforms that BOP's symmetry-aware pose errors (MSSD, MSPD:
``evaluation.symmetric_pose_errors``, csrc/pxt_eval_sym.hip) minimise over.  Host-side float64 numpy, no GPU.

The rule is BOP's (bop_toolkit ``misc.get_symmetry_transformations``) with ONE deviation: a continuous axis is sampled at
``n = ceil(pi / max_step)`` rotations ``2 pi k / n`` for ``k = 0 .. n - 1`` - the toolkit's loop starts at ``k = 1``, so
that its set lacks the bare discrete transforms (and, without discrete ones, the identity).  Here the identity is
always element 0.  The minimum over this set is never larger than over the toolkit's, and a pose that the toolkit's set
scores best is at most one rotation step (``2 pi / n``, 0.02 rad by default) from a member of this one.

Nothing here converts units: the translations of the transforms, a continuous entry's ``offset`` and ``diameter`` are
passed through in the units of the file (BOP: millimetres); the caller scales them to the units of its model points.
"""
from __future__ import annotations

import json
import math
from typing import Dict, Optional, Sequence

import numpy as np

MAX_SYMMETRIES = 1024   # PXT_SYM_ERR_MAX_SYMS
RIGID_TOLERANCE = 1e-6  # max |R^T R - I|


def _rigid_4x4(M, what: str) -> np.ndarray:
    T = np.asarray(M, dtype=np.float64)
    if T.size != 16:
        raise ValueError(f"{what}: expected a 4x4 matrix or 16 row-major floats (got shape {T.shape})")
    T = T.reshape(4, 4).copy()
    if not np.isfinite(T).all():
        raise ValueError(f"{what}: non-finite value")
    R = T[:3, :3]
    if np.abs(R.T @ R - np.eye(3)).max() > RIGID_TOLERANCE:
        raise ValueError(f"{what}: not rigid (|R^T R - I| = {np.abs(R.T @ R - np.eye(3)).max():.3g})")
    if np.linalg.det(R) < 0:
        raise ValueError(f"{what}: a reflection (det R < 0) is no rigid transform")
    if np.abs(T[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > RIGID_TOLERANCE:
        raise ValueError(f"{what}: the last row must be 0 0 0 1")
    T[3] = [0.0, 0.0, 0.0, 1.0]
    return T


def rotation(axis, angle: float) -> np.ndarray:
    """3x3 rotation by ``angle`` about ``axis`` (normalised here; Rodrigues).  ``angle = 0`` is the identity exactly."""
    a = np.asarray(axis, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"axis must hold 3 finite floats (got {axis!r})")
    norm = np.linalg.norm(a)
    if norm == 0.0:
        raise ValueError("a zero axis")
    if angle == 0.0:
        return np.eye(3)
    a = a / norm
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transforms(discrete: Sequence = (), continuous: Sequence[Dict] = (), max_step: float = 0.01) -> np.ndarray:
    """float64 ``[S, 4, 4]``: the symmetry set of an object.

    ``discrete``: 4x4 matrices (arrays, or 16 row-major floats as in ``models_info.json``).  ``continuous``:
    ``{"axis": [3], "offset": [3]}`` entries (``offset`` defaults to 0: a point on the axis).  With
    ``n = ceil(pi / max_step)`` (315 for the default), every continuous entry gives the rotations
    ``R = rot(axis, 2 pi k / n)``, ``t = offset - R offset`` for ``k = 0 .. n - 1``; the discrete list is
    ``[I] + discrete``.  With continuous entries the set is every product ``C D`` (continuous outer, discrete inner), else
    the discrete list.  The identity is element 0 (see the module docstring for how this differs from BOP's toolkit).

    Raises ValueError for a non-rigid matrix (``R^T R`` off the identity by more than 1e-6, or ``det < 0``), a non-finite
    value, a zero axis, ``max_step <= 0`` and a set of more than 1024 transforms."""
    if not (np.isfinite(max_step) and max_step > 0):
        raise ValueError(f"max_step must be a positive number (got {max_step})")
    disc = [np.eye(4)] + [_rigid_4x4(M, f"discrete symmetry {i}") for i, M in enumerate(discrete)]
    entries = []
    for j, entry in enumerate(continuous):
        offset = np.asarray(entry.get("offset", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(-1)
        if offset.shape != (3,) or not np.isfinite(offset).all():
            raise ValueError(f"continuous symmetry {j}: offset must hold 3 finite floats")
        rotation(entry["axis"], 0.0)  # refuses a zero or non-finite axis
        entries.append((entry["axis"], offset))
    n = int(math.ceil(math.pi / float(max_step)))
    count = n * len(entries) * len(disc) if entries else len(disc)
    if count > MAX_SYMMETRIES:
        raise ValueError(f"{count} symmetry transforms (at most {MAX_SYMMETRIES}); raise max_step")
    if not entries:
        return np.stack(disc)
    out = []
    for axis, offset in entries:
        for k in range(n):
            C = np.eye(4)
            C[:3, :3] = rotation(axis, 2.0 * math.pi * k / n)
            C[:3, 3] = offset - C[:3, :3] @ offset
            out.extend(C @ D for D in disc)
    return np.stack(out)


def centred_12(symmetries, centroid) -> np.ndarray:
    """float64 ``[S, 12]`` (R row-major, then t) of ``[S, 4, 4]`` transforms re-expressed for vertices with ``centroid``
    subtracted: with ``u = v - c``, ``S v - c = R u + t'`` where ``t' = R c + t - c``."""
    T = np.asarray(symmetries, dtype=np.float64).reshape(-1, 4, 4)
    c = np.asarray(centroid, dtype=np.float64).reshape(3)
    R = T[:, :3, :3]
    tc = np.einsum("sij,j->si", R, c) + T[:, :3, 3] - c
    plain = np.all(R == np.eye(3), axis=(1, 2)) & np.all(T[:, :3, 3] == 0.0, axis=1)
    tc[plain] = 0.0  # the identity stays the identity bit for bit (R c - c alone is 0 only because R == I)
    return np.concatenate([R.reshape(-1, 9), tc], axis=1)


def read_models_info(path, obj_id: Optional[int] = None) -> Dict:
    """``{"diameter": float | None, "symmetries": [S, 4, 4]}`` from a BOP ``models_info.json``: either the whole file,
    keyed by object id (``obj_id`` is then required), or one object's dict.  ``diameter`` and every translation are in
    the units of the file; no conversion is done here."""
    with open(str(path)) as f:
        info = json.load(f)
    if not isinstance(info, dict):
        raise ValueError(f"{path}: expected a JSON object")
    fields = ("diameter", "symmetries_discrete", "symmetries_continuous", "min_x", "size_x")
    if not any(k in info for k in fields):  # the whole-file form
        if obj_id is None:
            raise ValueError(f"{path} holds several objects ({', '.join(sorted(info, key=str)[:8])} ...): obj_id is required")
        key = str(int(obj_id))
        if key not in info:
            raise KeyError(f"{path}: no object {key}")
        info = info[key]
    diameter = info.get("diameter")
    return {"diameter": None if diameter is None else float(diameter),
            "symmetries": symmetry_transforms(info.get("symmetries_discrete", ()), info.get("symmetries_continuous", ()))}
