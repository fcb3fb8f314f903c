"""The head trunks' activation-plane epilogues (gp_head.h split3_pair / split_act / q8_of) on a real MI355X.

* The e4m3 planes come straight from the packed f16 planes (v_cvt_scalef32_pk_fp8_f16 under the plane's scale):
  every f16 bit pattern x the three planes through gp_debug_q8_probe, against the earlier path
  (v_cvt_pk_fp8_f32 of the converted and multiplied value) and against pack.e4m3_bits on the CPU.
* The residuals and the lo plane are formed without converting a plane back (v_fma_mix_f32, v_fma_mixlo/hi_f16):
  score(), a T = 3 PC run and one ODE attempt must reproduce, bit for bit, what the library of the commit before
  the change produced (tests/golden/golden_plane_epilogue.npz, recorded from that library by
  tests/golden/make_golden_plane_epilogue.py; the calls are tests/golden/plane_epilogue_inputs.py).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANE_EXP = (-7, 4, 16)      # gp_head.h Q8_EXP_HI / _MID / _LO: e4m3 plane = f16 plane x 2^this


@pytest.mark.parametrize("plane", (0, 1, 2))
def test_q8_conversion_exhaustive(plane):
    """All 65,536 f16 bit patterns. On the reachable domain (finite v, |v x 2^e| <= 256; no pattern inside it is
    left out) the helper's bytes equal the earlier path's and pack.e4m3_bits(v x 2^e); outside it nothing is
    asserted. Measured on MI355X: the instruction divides by its scale operand (the helper passes 2^-e), and the
    two paths agree on every finite pattern of every plane, f16 subnormal inputs and e4m3 subnormal results
    included (domain sizes 61,442 / 38,914 / 14,338 patterns for hi / mid / lo)."""
    from genpose2_amd import _lib, pack
    lib = _lib.load()
    bits = np.arange(65536, dtype=np.uint16)
    d_in = torch.from_numpy(bits.view(np.int16).copy()).to(DEV)
    new = torch.full((65536,), 0xAA, dtype=torch.uint8, device=DEV)
    old = torch.full((65536,), 0x55, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gp_debug_q8_probe(ctypes.c_void_p(d_in.data_ptr()), 65536, plane, ctypes.c_void_p(new.data_ptr()),
                                     ctypes.c_void_p(old.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "debug_q8_probe")
    torch.cuda.synchronize()
    new, old = new.cpu().numpy(), old.cpu().numpy()
    v = bits.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = v * 2.0 ** PLANE_EXP[plane]                      # exact in float64
    dom = np.isfinite(v) & (np.abs(np.where(np.isfinite(x), x, np.inf)) <= 256.0)
    want = pack.e4m3_bits(x[dom])
    print(f"plane {plane} (x 2^{PLANE_EXP[plane]}): {int(dom.sum())} patterns in the domain; new != old on "
          f"{int((new[dom] != old[dom]).sum())}, new != CPU on {int((new[dom] != want).sum())}; finite patterns "
          f"outside the domain where the paths differ: {int((new != old)[np.isfinite(v) & ~dom].sum())}")
    assert dom.sum() > 14000 and dom[0] and dom[0x8000]     # both zeros and the subnormals are inside
    assert np.array_equal(new[dom], old[dom])
    assert np.array_equal(new[dom], want)


def test_q8_probe_ragged_count():
    """n that is no multiple of a thread's eight patterns: bytes past n stay untouched."""
    from genpose2_amd import _lib
    lib = _lib.load()
    n = 2051
    bits = (np.arange(n, dtype=np.uint32) * 7 % 0x5800).astype(np.uint16)     # finite, hi plane in range
    d_in = torch.from_numpy(bits.view(np.int16).copy()).to(DEV)
    new = torch.full((n + 13,), 0xAA, dtype=torch.uint8, device=DEV)
    old = torch.full((n + 13,), 0x55, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gp_debug_q8_probe(ctypes.c_void_p(d_in.data_ptr()), n, 0, ctypes.c_void_p(new.data_ptr()),
                                     ctypes.c_void_p(old.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "debug_q8_probe")
    torch.cuda.synchronize()
    new, old = new.cpu().numpy(), old.cpu().numpy()
    assert np.array_equal(new[:n], old[:n]) and (new[n:] == 0xAA).all() and (old[n:] == 0x55).all()


@pytest.fixture(scope="module")
def heads():
    import plane_epilogue_inputs as pi
    h = pi._heads()
    yield h
    h.set_pc_small("auto")
    h.set_arith("f16x3")


def _compare(out):
    import plane_epilogue_inputs as pi
    g = golden("plane_epilogue")
    for name, a in out.items():
        e = pi.entry(a)
        rows_equal = np.array_equal(e["rows"], g[name + "_rows"])
        sha_equal = np.array_equal(e["sha"], g[name + "_sha"])
        if not rows_equal:
            bad = np.nonzero((e["rows"] != g[name + "_rows"]).reshape(e["rows"].shape[0], -1).any(1))[0]
            print(f"{name}: {len(bad)} of {e['rows'].shape[0]} sampled rows differ (sample indices {bad[:8]})")
        print(f"{name}: shape {a.shape}, sampled rows equal {rows_equal}, digest equal {sha_equal}")
        assert rows_equal and sha_equal, name


@pytest.mark.parametrize("case", ("r8250_auto", "r50_fp8", "r50_f16"))
def test_trunk_bits_equal_parent_commit(heads, case):
    """score() at two times and a T = 3 gp_pc_sample with injected z1 / z2 (res, q and every state): R = 8,250
    (K = 50: 64-candidate tiles, ragged last tile, the hybrid kernel the benchmark runs), R = 50 with
    set_pc_small("fp8") (the hybrid form on one ragged 16-row tile) and R = 50 with "f16" (the six-product form).
    Bits, the sign of zeros included (the fixture holds bit patterns and digests of the bytes)."""
    import plane_epilogue_inputs as pi
    name, R, form = next(c for c in pi.PC_CASES if c[0] == case)
    _compare(pi.pc_case(heads, name, R, form))


def test_ode_attempt_bits_equal_parent_commit(heads):
    """One gp_ode_attempt at 4,097 rows (two tiles per workgroup, one row in the last): the six stage derivatives,
    y_new and the error scalars equal the parent's, bit for bit."""
    import plane_epilogue_inputs as pi
    _compare(pi.ode_case(heads))
