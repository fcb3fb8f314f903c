"""CPU checks behind tests/test_gpu_pose_edges.py: the inputs (tests/golden/pose_edge_inputs.py), the
operation-by-operation restatement of the pose tails (tests/pose_ref.py), its anchor in the reference's own torch
run (tests/golden/golden_pose_edges.npz) and the probe's argument checks. No GPU is used."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_edge_inputs as pe
import pose_ref as P
from conftest import REPO, golden
from oracle import oracle

NEW = "gp_debug_pose_tail_f32"


@pytest.fixture(scope="module")
def inp():
    return pe.build()


@pytest.fixture(scope="module")
def fx():
    return golden("pose_edges")


@pytest.fixture(scope="module")
def restated(inp):
    """The restatement in both precisions: gs, q of quat_from_gs(gs), and the branch information."""
    out = {}
    for dt in (np.float32, np.float64):
        gs = P.gram_schmidt6(inp["rows"][:, :6].astype(dt))
        q, info = P.quat_from_gs(gs, want_info=True)
        out[dt] = dict(gs=gs, q=q, **info)
    return out


def _same(a, b):
    return bool(np.array_equal(a, b, equal_nan=True)) and a.dtype == b.dtype


def test_input_digest_and_layout(inp, fx):
    assert str(fx["digest"]) == pe.digest(inp)
    n = len(inp["rows"])
    assert inp["rows"].dtype == np.float32 and inp["rows"].shape == (n, 9)
    assert fx["gs_f32"].shape == (n, 6) and fx["q_f64"].shape == (n, 4) and fx["gs_f64"].dtype == np.float64
    sizes = {k: s.stop - s.start for k, s in inp["slices"].items()}
    assert sizes == {"cube": 72, "rand": 768, "pi_rand": 768, "pi_tie": 21, "near_pi": 672, "t120": 240, "deg": 13}
    R = inp["R"][pe.well_mask(inp)]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(R) - 1).max() < 1e-14
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "golden_pose_edges.npz")) < (1 << 20)


def test_branch_census(inp, restated):
    """By the float32 restatement every branch of the four-way argmax takes at least 32 rows of the
    well-conditioned families ([492, 738, 594, 717]) and at least one of ``cube`` (15 / 5 / 3 / 1 at each scale);
    ``cube`` holds exact four-way and two-way ties, exact w == 0 and q_abs exactly 0; the half turns all have
    w == 0 up to rounding and leave branch 0."""
    r = restated[np.float32]
    well = pe.well_mask(inp)
    census = P.branch_census(r["best"][well])
    print("census (well-conditioned):", census)
    assert census == [492, 738, 594, 717] and min(census) >= 32
    cube = inp["slices"]["cube"]
    for s in range(3):
        sl = slice(cube.start + 24 * s, cube.start + 24 * (s + 1))
        assert P.branch_census(r["best"][sl]) == [15, 5, 3, 1]
    qa = r["qa"][cube]
    top = qa == qa.max(-1, keepdims=True)
    assert set(top.sum(-1).tolist()) == {1, 2, 4}                       # no tie, two-way, four-way
    assert (qa == 0).any() and (r["q"][cube][:, 0] == 0).any()          # q_abs exactly 0, w exactly 0
    assert not np.any(r["best"][inp["slices"]["pi_rand"]] == 0)
    assert np.abs(r["q"][inp["slices"]["pi_rand"]][:, 0]).max() < 1e-6


def test_floor_is_out_of_reach_of_finite_rows(inp, restated):
    """The ``2 * max(q_abs_best, 0.1)`` floor. The four q_abs^2 are 1 +- m00 +- m11 +- m22 and sum to exactly 4
    whatever the matrix, so the largest q_abs is at least 1 up to rounding: no finite row, well-conditioned or
    degenerate, comes anywhere near 0.1 (the smallest q_abs_best over every finite row here is 1.0, float32 and
    float64). A row 'within 1e-3 of 0.1' therefore does not exist and no family can be extended to hold one;
    what is asserted instead is that fact, and that the floor's other side is the NaN rows alone: every q_abs
    fails ``> 0``, q_abs_best is 0, the denominator is 0.2 and q = (0, nan, nan, nan). Those rows are in ``deg``
    and are compared bit for bit on the device."""
    for dt in (np.float32, np.float64):
        r = restated[dt]
        finite = np.isfinite(inp["rows"][:, :6]).all(-1)
        assert finite.sum() == len(finite) - 2
        assert r["qa_best"][finite].min() >= 1 - 4 * np.finfo(dt).eps
        assert np.all(r["qa_best"][~finite] == 0)
        q = r["q"][~finite]
        assert np.all(q[:, 0] == 0) and np.isnan(q[:, 1:]).all()


def test_oracle_agrees_with_the_restatement(inp, restated):
    """oracle.gram_schmidt and oracle.matrix_to_quaternion . rot6_to_matrix equal the restatement bit for bit on
    every family and in both precisions -- NumPy's reduction over three elements is the kernels' order -- with one
    exception that is no matter of order: a NaN norm. The kernels clamp with the select ``n > 1e-12 ? n : 1e-12``,
    which turns a NaN norm into 1e-12; np.maximum (the oracle) and torch's clamp_min (the reference's F.normalize)
    keep the NaN. On the row with a NaN in a1 the oracle and the reference give an all-NaN rotation, the kernels
    (1e12, nan, 3e12 | nan, nan, nan); the quaternion is (0, nan, nan, nan) for all of them. Both are pinned."""
    nan_row = inp["slices"]["deg"].start + 9
    assert np.isnan(inp["rows"][nan_row, 1])
    others = np.ones(len(inp["rows"]), bool)
    others[nan_row] = False
    for dt in (np.float32, np.float64):
        r = restated[dt]
        rot6 = inp["rows"][:, :6].astype(dt)
        with np.errstate(all="ignore"):
            og = oracle.gram_schmidt(rot6)
            oq = oracle.matrix_to_quaternion(oracle.rot6_to_matrix(r["gs"]))
        assert _same(og[others], r["gs"][others])
        assert _same(oq, r["q"])
        assert np.isnan(og[nan_row]).all()
        want = np.array([1e12, np.nan, 3e12, np.nan, np.nan, np.nan]).astype(dt)
        if dt == np.float32:
            want[0], want[2] = np.float32(1) / np.float32(1e-12), np.float32(3) / np.float32(1e-12)
        else:
            want[0], want[2] = 1 / 1e-12, 3 / 1e-12
        assert _same(r["gs"][nan_row], want)
    assert _same(P.gram_schmidt6_quad(inp["rows"][:, :6].copy()), restated[np.float32]["gs"])
    assert _same(P.rot6_to_quat(inp["rows"][:, :6].copy()), P.quat_from_gs(inp["rows"][:, :6].copy()))


def test_anchor_in_the_reference(inp, fx, restated):
    """Well-conditioned families. Measured on the committed inputs: the float64 restatement against the
    reference's float64 torch run 2.2e-16 on the Gram-Schmidt and 2.2e-16 on q from equal input; the float32
    restatement against the float64 one 1.36e-7 (Gram-Schmidt 1.36e-7, q 1.20e-7 modulo sign; the sign differs on
    3 rows, where an argmax tie falls the other way). 4x each is asserted: the inputs set these, not the code.
    The reference's float32 torch run differs from the float32 restatement in the last place on 23 % of the rows
    (Gram-Schmidt) and 43 % (q): torch's vector_norm does not sum three squares as (a^2 + b^2) + c^2. Its NaN
    and inf rows agree with the oracle's."""
    well = pe.well_mask(inp)
    r32, r64 = restated[np.float32], restated[np.float64]
    e_gs = float(np.abs(r64["gs"][well] - fx["gs_f64"][well]).max())
    e_q = float(np.abs(P.quat_from_gs(fx["gs_f64"])[well] - fx["q_f64"][well]).max())
    sign = np.sign((r32["q"].astype(np.float64) * r64["q"]).sum(-1, keepdims=True))
    e_32 = max(float(np.abs(r32["gs"][well].astype(np.float64) - r64["gs"][well]).max()),
               float(np.abs(r32["q"][well] * sign[well] - r64["q"][well]).max()))
    qn = float(np.abs(np.sqrt((r32["q"][well].astype(np.float64) ** 2).sum(-1)) - 1).max())
    rate_gs = float(np.mean(np.any(fx["gs_f32"][well] != r32["gs"][well], 1)))
    rate_q = float(np.mean(np.any(fx["q_f32"][well] != r32["q"][well], 1)))
    print(f"gs64 vs reference {e_gs:.3e} | q64 vs reference {e_q:.3e} | f32 vs f64 {e_32:.3e} | | |q| - 1 | {qn:.3e} "
          f"| reference f32 differs on {rate_gs:.1%} (gs) {rate_q:.1%} (q) of rows")
    for got, const in ((e_gs, P.GS64_VS_REF), (e_q, P.Q64_VS_REF), (e_32, P.F32_VS_F64), (qn, P.QNORM_F32)):
        assert abs(got / const - 1) < 1e-3                     # pose_ref's constants are these measurements
    assert e_gs <= P.MARGIN * P.GS64_VS_REF and e_q <= P.MARGIN * P.Q64_VS_REF and e_32 <= P.MARGIN * P.F32_VS_F64
    assert not np.any(sign[well] == 0)
    # the reference's float32 run stays within the same float32 bound of its float64 run
    s = np.sign((fx["q_f32"].astype(np.float64) * fx["q_f64"]).sum(-1, keepdims=True))
    assert np.abs(fx["q_f32"][well] * s[well] - fx["q_f64"][well]).max() <= P.MARGIN * P.F32_VS_F64
    d = inp["slices"]["deg"]
    with np.errstate(all="ignore"):
        assert _same(fx["gs_f32"][d][[9, 11]], oracle.gram_schmidt(inp["rows"][d][[9, 11], :6].copy()))


def test_probe_argument_checks():
    """gp_debug_pose_tail_f32 is declared, bound and exported; null pointers, rows < 0 and k < 1 give a status
    before anything is launched, rows == 0 returns OK; the ABI version stays 7."""
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    assert re.search(r"\b%s\(" % NEW, header) and NEW in _lib.EXPORTED and NEW in set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7 and "#define GP_ABI_VERSION 7" in header
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = lib.gp_debug_pose_tail_f32
    assert fn(p, 0, 1, p, p, p, None) == 0
    for args in [(None, 1, 1, p, p, p), (p, 1, 1, None, p, p), (p, 1, 1, p, None, p), (p, 1, 1, p, p, None),
                 (p, -1, 1, p, p, p), (p, 1, 0, p, p, p), (p, 0, 0, p, p, p)]:
        assert fn(*args, None) == -1, args
        assert b"debug_pose_tail_f32" in lib.gp_last_error()
