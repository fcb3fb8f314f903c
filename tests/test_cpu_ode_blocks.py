"""CPU checks of the references behind tests/test_gpu_ode_blocks.py (tests/ode_blocks_ref.py): scipy's RK45 with a
scripted error norm reproduces the committed solver traces bit for bit, every clamped script walks into the
controller branch it is named for, a float32 network stays under the head bar the device stages are held to, and
the per-object controller's debug entry is declared, bound and exported."""
import json
import math
import os
import re

import numpy as np
import pytest

import ode_blocks_ref as R
from conftest import GOLDEN, REPO

NEW = ("gp_debug_ode_obj_rec_size", "gp_debug_ode_obj_control")
COUNTS = (9, 144, 450, 90, 630)      # rows * 9 of the device cases (batch 1 / 16 / 50 rows, objects of 10 / 70 rows)


@pytest.fixture(scope="module")
def golden_trace():
    with open(os.path.join(GOLDEN, "golden_ode_trace.json")) as f:
        return json.load(f)


def test_debug_entry_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7 and "#define GP_ABI_VERSION 7" in header      # additive: the ABI version stays
    assert lib.gp_debug_ode_obj_rec_size() == 168
    assert lib.gp_ode_ctl_size() == 208


def test_scripted_scipy_reproduces_the_committed_traces(golden_trace):
    """The (t, h) of every attempt, accept / reject and nfev 290 / 278 / 134 / 134 of the four committed solves,
    from scipy's RK45 fed only their error norms and first step size."""
    want_nfev = {"t1_none_ref32": 290, "t1_none_ref64": 278, "t055_s20_ref32": 134, "t055_s20_ref64": 134}
    scripts = R.trace_scripts(golden_trace, -1)
    assert set(scripts) == set(want_nfev)
    for name, (t0, tb, h0, errs, nfev) in scripts.items():
        case, ref = name.rsplit("_", 1)
        att = golden_trace[case][ref]["attempts"]
        tr = R.run_script(t0, tb, h0, errs)
        assert tr.status == 1 and tr.unused == 0 and tr.t == tb
        assert tr.nfev == nfev == want_nfev[name] == R.NFEV0 + 6 * len(att)
        assert [(a["t"], a["h"]) for a in tr.attempts] == [(a[0], a[1]) for a in att], name
        assert [a["accepted"] for a in tr.attempts] == [a[2] < 1 for a in att]
        assert tr.steps[-1] == (tb, tr.h_abs, "finished", nfev)
        rec = R.expected_records(tr)
        assert len(rec) == len(att) + 1 and rec[-1]["status"] == 1 and rec[-1]["nfev"] == nfev
        assert [r["nfev"] for r in rec[:-1]] == [2 + 6 * n for n in range(len(att))]
        # rejections only at attempts 0 and 1 (and once mid-solve in the T0 = 1 float32 run)
        rej = [n for n, a in enumerate(tr.attempts) if not a["accepted"]]
        assert rej[:2] == [0, 1] and len(rej) <= 3, (name, rej)


def test_trace_scripts_run_forward_too(golden_trace):
    """The same error sequences on the reversed interval end on t_bound with the same counts (the device test runs
    both directions)."""
    for name, (t0, tb, h0, errs, nfev) in R.trace_scripts(golden_trace, +1).items():
        tr = R.run_script(t0, tb, h0, errs)
        assert tr.direction == 1.0 and tr.status == 1 and tr.unused == 0 and tr.t == tb and tr.nfev == nfev, name


def _factor(at, n, m):
    """The step-size factor between attempts n and m = n + 1, rounded at 1e-9: the next attempt's h is re-formed
    from t + h, so it carries the rounding of t."""
    return round(at[m]["h_abs_loc"] / at[n]["h_abs_loc"], 9)


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_clamped_scripts_reach_their_branches(direction, count):
    S = R.clamped_scripts(direction)
    t0, tb = R.interval(direction)
    run = {}
    for name, (s0, sb, h0, errs) in S.items():
        sums, eff = R.script_sums(errs, count)
        for s in sums:
            a, b = R.split(s)
            assert (a + b == s and b + a == s) or math.isnan(s)
        run[name] = (R.run_script(s0, sb, h0, eff), eff)

    below1 = R.effective(R.err_sum(R.B1, count), count)
    assert 1.0 - 2.0 ** -52 <= below1 < 1.0 and R.effective(R.err_sum(1.0, count), count) == 1.0

    tr, eff = run["edges"]
    at = tr.attempts
    assert (tr.status, tr.n_accept, tr.n_reject) == (1, 7, 3) and tr.t == tb
    assert at[0]["err"] == 1.0 and not at[0]["accepted"]                         # err == 1 rejects ...
    assert _factor(at, 0, 1) == 0.9                        # ... by 0.9 pow(1, -0.2)
    assert at[2]["accepted"] and at[2]["rejected"] and _factor(at, 2, 3) == 1   # min(1, .)
    assert at[3]["err"] == 0.0 and _factor(at, 3, 4) == 10                  # err == 0: 10
    assert at[4]["err"] == below1 and at[4]["accepted"] and _factor(at, 4, 5) == 0.9
    assert not at[5]["accepted"] and at[5]["t"] not in (t0, tb)                  # a rejection mid-solve
    assert _factor(at, 7, 8) == 10                         # err <= 1e-6: 10 mid-solve
    assert at[-1]["t_new"] == tb and abs(at[-1]["h"]) < at[-2]["h_abs_loc"] * 10   # the last step is clipped

    tr, eff = run["clamp_low"]
    at = tr.attempts
    assert (tr.status, tr.n_accept, tr.n_reject) == (1, 9, 5)
    for n in (0, 1, 2, 5, 7):                                                    # 2000, 1e300 -> Inf, Inf, NaN, Inf
        assert not at[n]["accepted"] and _factor(at, n, n + 1) == 0.2, n
    assert math.isinf(eff[1]) and math.isinf(eff[2]) and math.isnan(eff[5])
    assert at[3]["accepted"] and _factor(at, 3, 4) == 1        # after three rejections: 1
    assert at[6]["accepted"] and at[6]["rejected"] and _factor(at, 6, 7) == 1

    tr, eff = run["nan_fail"]
    assert tr.status == -1 and tr.n_accept == 0 and tr.t == t0 and tr.nfev == 2 + 6 * tr.n_reject
    if direction < 0:
        assert tr.n_reject == 19                                                 # from h = 0.01 at t = 1
    last = tr.attempts[-1]["h_abs_loc"]
    assert last >= R.min_step(t0, direction) > last * 0.2

    tr, eff = run["min_step"]
    ms = R.min_step(t0, direction)
    assert tr.h0 < ms and tr.attempts[0]["h_abs_loc"] == ms and tr.status == 1 and tr.n_reject == 1

    tr, eff = run["land_exact"]
    a = tr.attempts[0]
    assert len(tr.attempts) == 1 and tr.status == 1
    assert a["t"] + tr.h0 * direction == tr.t_bound == a["t_new"]                # reached without the clip


@pytest.mark.parametrize("t,std", [(1.0, 50.0), (0.1, 1.0)])
def test_float32_network_is_under_the_head_bar(score_sd, t, std):
    """The stage bar of the device test (1e-5 of the row's max |float64 score|) on its inputs, for the same network
    in float32 NumPy: a correct fp32 implementation can meet it."""
    p64, p32 = R.head_params(score_sd, np.float64), R.head_params(score_sd, np.float32)
    worst = 0.0
    for rows, k in R.ATTEMPT_SHAPES:
        feat, y = R.attempt_inputs(rows, k, std)
        x = y.astype(np.float32)
        t32 = np.float32(t)
        ref = R.score_np(p64, feat, k, x, t32, np.float64)
        got = R.score_np(p32, feat, k, x, t32, np.float32).astype(np.float64)
        assert got.dtype == np.float64 and ref.shape == (rows, 9)
        worst = max(worst, float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max()))
    print(f"t = {t}: float32 NumPy vs float64, per-row relative max {worst:.2e}")
    assert worst < 1e-5
