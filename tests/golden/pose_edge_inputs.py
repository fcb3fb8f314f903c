"""Inputs of the pose-tail fixture (golden_pose_edges.npz): 6-D rotations at the branch edges of the sampler tails.

NumPy only, seeded. A row is (a1 | a2 | t): a1, a2 the first two columns of a rotation R built in float64, times a
scale, rounded to float32; t = normal(3) * 0.3. The float64 runs take the float32 values widened, so both precisions
see the same numbers.

Well-conditioned families (``WELL``), each at the scales ``SCALES``:
  cube     the 24 signed permutation matrices of determinant +1: exact four-way, two-way and no ties in the
           argmax of matrix_to_quaternion, exact w == 0, q_abs exactly 0
  rand     256 rotations, axis normal(3), angle uniform in (0, pi)
  pi_rand  256 rotations by exactly pi (R = 2 n n^T - I) about random axes
  pi_tie   pi about (1,1,0), (1,0,1), (0,1,1), (1,1,1), (1,-1,0), (-1,1,1), (1,1,-1)
  near_pi  pi - d for d in 1e-1 .. 1e-7, 32 random axes each
  t120     2 pi / 3 + d for d in 0, +-1e-3, +-1e-6, 16 random axes each
Degenerate family ``deg`` (bit comparison only): zero and parallel columns, squares that underflow in float32, a
huge dynamic range, a NaN row and an inf row, each followed by an ordinary row.
"""
from __future__ import annotations

import hashlib
import itertools

import numpy as np

SEED = 20260
SCALES = (1.0, 1e-3, 50.0)
WELL = ("cube", "rand", "pi_rand", "pi_tie", "near_pi", "t120")
FAMILIES = WELL + ("deg",)
NEAR_PI_DELTAS = tuple(10.0 ** -e for e in range(1, 8))
T120_DELTAS = (0.0, 1e-3, -1e-3, 1e-6, -1e-6)
PI_TIE_AXES = ((1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 0), (-1, 1, 1), (1, 1, -1))


def axis_angle(axis: np.ndarray, angle) -> np.ndarray:
    """Rodrigues, float64: axis (n,3) (normalised here), angle (n,) -> (n,3,3)."""
    axis = np.asarray(axis, np.float64).reshape(-1, 3)
    n = axis / np.sqrt((axis * axis).sum(-1, keepdims=True))
    angle = np.broadcast_to(np.asarray(angle, np.float64), (n.shape[0],))
    K = np.zeros((n.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -n[:, 2], n[:, 1]
    K[:, 1, 0], K[:, 1, 2] = n[:, 2], -n[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -n[:, 1], n[:, 0]
    s, c = np.sin(angle)[:, None, None], np.cos(angle)[:, None, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def half_turn(axis: np.ndarray) -> np.ndarray:
    """Rotation by exactly pi: 2 n n^T - I (no sin(pi) residue)."""
    axis = np.asarray(axis, np.float64).reshape(-1, 3)
    n = axis / np.sqrt((axis * axis).sum(-1, keepdims=True))
    return 2 * n[:, :, None] * n[:, None, :] - np.eye(3)[None]


def cube_rotations() -> np.ndarray:
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = signs[r]
            if np.linalg.det(m) > 0:
                out.append(m)
    assert len(out) == 24
    return np.stack(out)


def _generators():
    rng = np.random.default_rng(SEED)
    g = {"cube": cube_rotations(),
         "rand": axis_angle(rng.normal(size=(256, 3)), rng.uniform(0, np.pi, size=256)),
         "pi_rand": half_turn(rng.normal(size=(256, 3))),
         "pi_tie": half_turn(np.array(PI_TIE_AXES, np.float64)),
         "near_pi": np.concatenate([axis_angle(rng.normal(size=(32, 3)), np.pi - d) for d in NEAR_PI_DELTAS]),
         "t120": np.concatenate([axis_angle(rng.normal(size=(16, 3)), 2 * np.pi / 3 + d) for d in T120_DELTAS])}
    return g, rng


def _deg_rows() -> np.ndarray:
    plain = (1, 2, 3, 3, -1, 2)
    rows = [(0, 0, 0, 1, 2, 3),
            (1, 2, 3, 0, 0, 0),
            (0, 0, 0, 0, 0, 0),
            (1, 2, 3, 2, 4, 6),
            (1, 2, 3, -1, -2, -3),
            (1e-30, 0, 0, 0, 1e-30, 0),
            (1e-20, 0, 0, 0, 1, 0),
            (1e15, 0, 0, 0, 1e-15, 0),
            (1, 1e-8, 0, 1, 0, 0),
            (1, np.nan, 3, 3, -1, 2),
            plain,
            (1, np.inf, 3, 3, -1, 2),
            plain]
    return np.array(rows, np.float64)


def build():
    """-> dict: rows (N,9) f32, R (N,3,3) f64 (nan for ``deg``), family (N,) index into FAMILIES, scale (N,) f64,
    and ``slices``: family -> slice of rows."""
    gens, rng = _generators()
    rot6, Rs, fam, scale, slices = [], [], [], [], {}
    at = 0
    for f, name in enumerate(WELL):
        R = gens[name]
        start = at
        for s in SCALES:
            rot6.append(np.concatenate([R[:, :, 0], R[:, :, 1]], -1) * s)
            Rs.append(R)
            fam.append(np.full(len(R), f))
            scale.append(np.full(len(R), s))
            at += len(R)
        slices[name] = slice(start, at)
    d = _deg_rows()
    rot6.append(d)
    Rs.append(np.full((len(d), 3, 3), np.nan))
    fam.append(np.full(len(d), len(WELL)))
    scale.append(np.ones(len(d)))
    slices["deg"] = slice(at, at + len(d))
    rot6 = np.concatenate(rot6)
    t = rng.normal(size=(len(rot6), 3)) * 0.3
    with np.errstate(over="ignore", under="ignore"):
        rows = np.concatenate([rot6, t], -1).astype(np.float32)
    return dict(rows=rows, R=np.concatenate(Rs), family=np.concatenate(fam), scale=np.concatenate(scale),
                slices=slices)


def centers(n_obj: int) -> np.ndarray:
    """Per-object centres, uniform(3), float32 (n_obj,3); a prefix of one seeded stream."""
    return np.random.default_rng(SEED + 1).uniform(size=(4096, 3)).astype(np.float32)[:n_obj].copy()


def well_mask(inp) -> np.ndarray:
    return inp["family"] < len(WELL)


def digest(inp) -> str:
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(inp["rows"]).tobytes())
    h.update(centers(4096).tobytes())
    return h.hexdigest()
