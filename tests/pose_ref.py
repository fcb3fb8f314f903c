"""Operation-by-operation NumPy restatement of the pose tails' device functions, in the dtype it is given.

  gram_schmidt6      csrc/gp_head.h gram_schmidt6<T>
  gram_schmidt6_quad csrc/gp_head.h gram_schmidt6_quad (the four-lanes-per-row form: its result per row)
  quat_from_gs       csrc/gp_head.h quat_from_gs<T> (a second Gram-Schmidt, then matrix_to_quaternion)
  rot6_to_quat       csrc/gp_aggregate.hip rot6_to_quat (one Gram-Schmidt, then matrix_to_quaternion)

Every operation is one NumPy elementwise operation on columns, in the kernels' order and grouping, each rounded on
its own: (v0*v0 + v1*v1) + v2*v2, (b0*v3 + b1*v4) + b2*v5, the cross product term by term, ((1 + m00) + m11) + m22,
``q_abs > 0 ? sqrt : 0``, the first maximum under strict ``>``, 2 * max(q_abs_best, 0.1) and the clamp
``n > 1e-12 ? n : 1e-12`` -- a select, so a NaN norm becomes 1e-12 (np.maximum and torch's clamp_min would keep
the NaN). No reduction or library routine whose order is an implementation detail is used.

These are the bits the kernels are held to (tests/test_gpu_pose_edges.py); the reference's torch output is the
high-precision anchor (tests/test_cpu_pose_edges.py).
"""
from __future__ import annotations

import numpy as np

# Measured on the committed inputs (tests/golden/pose_edge_inputs.py), well-conditioned families, reference-only
# quantities (no device figure enters them); the tests assert MARGIN x each, since the inputs set them.
GS64_VS_REF = 2.220446049250313e-16     # max |gram_schmidt6 float64 - the reference's float64 normalize_rotation|
Q64_VS_REF = 2.220446049250313e-16      # max |quat_from_gs float64 - the reference's float64 quaternion|, equal input
F32_VS_F64 = 1.3631626283316933e-07     # max |float32 restatement - float64 restatement| over GS and q (q mod sign)
QNORM_F32 = 1.0570878405946615e-07      # max | |q| - 1 | of the float32 restatement
MARGIN = 4.0


def _cols(v, n):
    return [np.ascontiguousarray(v[:, i]) for i in range(n)]


def _clamp(n, dt):
    return np.where(n > dt(1e-12), n, dt(1e-12))


def gram_schmidt6(v: np.ndarray) -> np.ndarray:
    """(n,6) -> (n,6), in v.dtype."""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        v0, v1, v2, v3, v4, v5 = _cols(v, 6)
        n1 = _clamp(np.sqrt((v0 * v0 + v1 * v1) + v2 * v2), dt)
        b0, b1, b2 = v0 / n1, v1 / n1, v2 / n1
        d = (b0 * v3 + b1 * v4) + b2 * v5
        c0, c1, c2 = v3 - d * b0, v4 - d * b1, v5 - d * b2
        n2 = _clamp(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2), dt)
        out = np.stack([b0, b1, b2, c0 / n2, c1 / n2, c2 / n2], -1)
    assert out.dtype == v.dtype
    return out


def gram_schmidt6_quad(v: np.ndarray) -> np.ndarray:
    """The row's result of the quad form: lane part 0 holds a1 and normalises it, its b is broadcast to the quad,
    lane part 1 holds a2 and projects it. float32 only, as the kernel."""
    assert v.dtype == np.float32
    dt = np.float32
    with np.errstate(all="ignore"):
        p0 = _cols(v[:, 0:3], 3)                       # lane part 0's registers
        p1 = _cols(v[:, 3:6], 3)                       # lane part 1's registers
        n1 = _clamp(np.sqrt((p0[0] * p0[0] + p0[1] * p0[1]) + p0[2] * p0[2]), dt)
        B0, B1, B2 = p0[0] / n1, p0[1] / n1, p0[2] / n1     # quad_bcast0 of part 0's b
        d = (B0 * p1[0] + B1 * p1[1]) + B2 * p1[2]
        c0, c1, c2 = p1[0] - d * B0, p1[1] - d * B1, p1[2] - d * B2
        n2 = _clamp(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2), dt)
        out = np.stack([B0, B1, B2, c0 / n2, c1 / n2, c2 / n2], -1)
    assert out.dtype == v.dtype
    return out


def _quat_of_columns(g: np.ndarray, want_info: bool):
    """matrix_to_quaternion of R = [b1 b2 b1 x b2] from the Gram-Schmidt'ed (n,6)."""
    dt = g.dtype.type
    with np.errstate(all="ignore"):
        g0, g1, g2, g3, g4, g5 = _cols(g, 6)
        b3x = g1 * g5 - g2 * g4
        b3y = g2 * g3 - g0 * g5
        b3z = g0 * g4 - g1 * g3
        m00, m01, m02 = g0, g3, b3x
        m10, m11, m12 = g1, g4, b3y
        m20, m21, m22 = g2, g5, b3z
        one = dt(1)
        qa = [((one + m00) + m11) + m22, ((one + m00) - m11) - m22, ((one - m00) + m11) - m22,
              ((one - m00) - m11) + m22]
        qa = [np.where(a > dt(0), np.sqrt(np.where(a > dt(0), a, dt(0))), dt(0)) for a in qa]
        best = np.zeros(g.shape[0], np.int64)
        qb = qa[0].copy()
        for i in range(1, 4):                          # strict >: the first maximum stays
            take = qa[i] > qb
            best = np.where(take, i, best)
            qb = np.where(take, qa[i], qb)
        cand = [[qa[0] * qa[0], m21 - m12, m02 - m20, m10 - m01],
                [m21 - m12, qa[1] * qa[1], m10 + m01, m02 + m20],
                [m02 - m20, m10 + m01, qa[2] * qa[2], m12 + m21],
                [m10 - m01, m20 + m02, m21 + m12, qa[3] * qa[3]]]
        den = dt(2) * np.where(qb > dt(0.1), qb, dt(0.1))
        q = np.stack([np.choose(best, [cand[b][i] for b in range(4)]) / den for i in range(4)], -1)
    assert q.dtype == g.dtype
    if want_info:
        return q, dict(best=best, qa_best=qb, qa=np.stack(qa, -1))
    return q


def quat_from_gs(v: np.ndarray, want_info: bool = False):
    """(n,>=6) already Gram-Schmidt'ed -> q (n,4) wxyz; the function runs Gram-Schmidt once more first."""
    return _quat_of_columns(gram_schmidt6(np.ascontiguousarray(v[:, :6])), want_info)


def rot6_to_quat(v: np.ndarray, want_info: bool = False):
    """(n,6) float32 -> q (n,4) wxyz: the aggregation's route, one Gram-Schmidt."""
    return _quat_of_columns(gram_schmidt6(np.ascontiguousarray(v[:, :6])), want_info)


def pose_tail(rows: np.ndarray, center_rows: np.ndarray, quad: bool = False):
    """The samplers' tail on (n,9) rows: Gram-Schmidt of [:6], + the row's centre on [6:], then quat_from_gs ->
    (res (n,9), q (n,7)) in rows.dtype. ``quad``: the float32 tail of the PC step (gram_schmidt6_quad)."""
    gs = gram_schmidt6_quad(rows[:, :6]) if quad else gram_schmidt6(np.ascontiguousarray(rows[:, :6]))
    t = rows[:, 6:] + center_rows.astype(rows.dtype)
    res = np.concatenate([gs, t], -1)
    return res, np.concatenate([quat_from_gs(res), t], -1)


def branch_census(best: np.ndarray) -> list:
    return [int((best == i).sum()) for i in range(4)]
