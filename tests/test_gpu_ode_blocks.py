"""The RK45 solver's device building blocks, each alone against a plain reference (tests/ode_blocks_ref.py):

1. the batch step controller (ode_control_kernel through gp_ode_auto_attempt_hs(..., what=1)) against scipy's RK45
   with a scripted error norm, record by record;
2. the per-object controller (ode_obj_control_kernel through gp_debug_ode_obj_control) the same way, one script per
   object in one launch;
3. gp_ode_init_norms against math.fsum and gp_ode_dense against scipy's RkDenseOutput;
4. one attempt, teacher-forced: gp_ode_rhs, gp_ode_attempt (stage launches) and gp_ode_auto_attempt what=3 (the
   fused kernel) against float64 NumPy formed from the K's the device wrote.

Bars: decisions, counters and every float whose value a clamp fixes are exact; sigma within 1 float32 ulp and coef
within 8 float64 ulps of the same expressions in NumPy (one double pow, published at 1 ulp, and at most three
roundings); the trace scripts within (n + 1) * 4 float64 ulps after control call n (one pow and three roundings per
control); fp64 combinations within 64 * 2^-52 of the summed magnitudes of their terms; the network at the project's
head bar, 1e-5 of the row's max |reference|.

How the trace bound reads per field (test _floats_ok): the times t, t_old, t_new in ulps of |t0 - t_bound|; the
carried h_abs, a product of factors, in its own ulps. h = t_new - t (and h_abs_loc = |h|, h_last) is the difference
of two times, each within the time bound, so it is held to twice that bound in ulps of the interval: in its own
ulps no bound of this kind can hold, because one ulp of t is 2^5 ulps of a step of 0.02 (8192 own ulps were seen on a
step of 4e-5). After the step that the clip cuts to t_bound, h_abs = |t_bound - t| * factor carries t's distance
times a factor of at most 10, so there it is held to its own (n + 1) * 4 ulps plus ten times the time bound.

Measured on MI355X over every test of this module (test_zz_report_distances prints them): sigma 0 float32 ulps (every
value equal), coef 8.0 float64 ulps at most (at the bar), trace scripts: times 8 ulps of the interval, h_abs 19 own
ulps, h 8 ulps of the interval, h_abs after the clipped step 80 ulps of the interval; every clamped script bit for bit.
The whole module takes 5.3 s, its slowest test 0.7 s (the 8193-row attempt)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import ode_blocks_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIG_MIN, BASE = 0.01, 50.0 / 0.01
DIFF = math.sqrt(2.0 * (math.log(50.0) - math.log(0.01)))
RTOL = ATOL = 1e-5
EPS64 = 2.0 ** -52
CS = (1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0)
A6 = np.zeros((6, 6), dtype=np.float64)
A6[:, :5] = R.A
A6 = np.ascontiguousarray(A6)
B6 = np.ascontiguousarray(R.B, dtype=np.float64)
E7 = np.ascontiguousarray(R.E, dtype=np.float64)
P74 = np.ascontiguousarray(R.P, dtype=np.float64)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _np_p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class OdeObjRec(ctypes.Structure):
    """Host mirror of the per-object controller record (gp_ode.hip OdeObjRec, 168 bytes)."""
    _fields_ = [("t", ctypes.c_double), ("h_abs", ctypes.c_double), ("t_old", ctypes.c_double),
                ("h", ctypes.c_double), ("t_new", ctypes.c_double), ("h_abs_loc", ctypes.c_double),
                ("coef", ctypes.c_double * 6), ("t32", ctypes.c_float * 6), ("sig", ctypes.c_float * 6),
                ("status", ctypes.c_int), ("active", ctypes.c_int), ("rejected", ctypes.c_int),
                ("nfev", ctypes.c_int), ("n_acc", ctypes.c_int), ("pend", ctypes.c_int)]


@pytest.fixture(scope="module")
def heads(score_sd):
    from genpose2_amd.device import HeadModel
    return HeadModel(score_sd, torch.device(DEV))


@pytest.fixture(scope="module")
def golden_trace():
    with open(os.path.join(GOLDEN, "golden_ode_trace.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def status_words():
    """Four pinned int32 words the device can write, and their device-side address."""
    from genpose2_amd import ode
    lease = ode._host_status_words(torch.device(DEV))
    assert lease[0] is not None, "pinned status words are not mapped for the device"
    yield lease
    torch.cuda.synchronize()
    ode._release_status_words(torch.device(DEV), lease)


# Largest distances seen, printed by the tests that measure them (-s shows them).
SEEN = dict.fromkeys(("sig_ulp32", "coef_ulp64", "trace_time", "trace_step", "trace_step_clip", "trace_h",
                      "trace_h_own"), 0.0)


# ================================================================================== shared record checks
def _stage_scalars_ok(rec, time_rows, heads):
    """t32, sig and coef of an active record against the same expressions in NumPy from the record's own t and h;
    time_rows (6,768): the rows the control call wrote, bitwise against HeadModel.time_proj(t32)."""
    t, h = np.float64(rec.t), np.float64(rec.h)
    ts = np.array([t + np.float64(c) * h for c in CS[:4]] + [t + np.float64(1.0) * h, t + h], dtype=np.float64)
    t32 = ts.astype(np.float32)
    assert np.array_equal(np.array(rec.t32[:], dtype=np.float32), t32), (list(rec.t32), t32)
    sig = np.float32(SIG_MIN) * np.power(np.float64(BASE), t32.astype(np.float64)).astype(np.float32)
    g = (np.float64(SIG_MIN) * np.power(np.float64(BASE), ts)) * np.float64(DIFF)
    coef = -(0.5 * (g * g))
    ds = np.abs(np.array(rec.sig[:], dtype=np.float64) - sig.astype(np.float64)) / np.spacing(sig).astype(np.float64)
    dc = np.abs(np.array(rec.coef[:], dtype=np.float64) - coef) / np.spacing(np.abs(coef))
    SEEN["sig_ulp32"] = max(SEEN["sig_ulp32"], float(ds.max()))
    SEEN["coef_ulp64"] = max(SEEN["coef_ulp64"], float(dc.max()))
    assert ds.max() <= 1.0, ("sigma: float32 ulps", ds)
    assert dc.max() <= 8.0, ("coef: float64 ulps", dc)
    if time_rows is not None:
        want = heads.time_proj(torch.from_numpy(t32).to(DEV))
        assert torch.equal(time_rows.view(torch.int32), want.view(torch.int32)), "time rows differ from time_proj"


def _floats_ok(n, rec, e, tr, exact, what):
    """The float fields of the record after control call n against scipy's (e: expected_records entry)."""
    span = float(np.spacing(np.float64(abs(tr.t0 - tr.t_bound))))
    lim = (n + 1) * 4
    for f in ("t", "t_old", "t_new", "h_abs", "h", "h_abs_loc", "h_last"):
        if e.get(f) is None or not hasattr(rec, f):
            continue
        got, want = float(getattr(rec, f)), float(e[f])
        if exact:
            assert got == want, (what, n, f, got, want)
            continue
        if f in ("t", "t_old", "t_new"):
            d = abs(got - want) / span
            SEEN["trace_time"] = max(SEEN["trace_time"], d)
            assert d <= lim, (what, n, f, got, want, d)
        elif f == "h_abs" and not e["clip"]:   # the carried step size: a product of factors, relative to itself
            d = R.ulps(got, want)
            SEEN["trace_step"] = max(SEEN["trace_step"], d)
            assert d <= lim, (what, n, f, got, want, d)
        elif f == "h_abs":
            # after the step that was clipped to t_bound, h_abs = |t_bound - t| * factor: t's distance (within the
            # time bound; t_bound is exact) times a factor of at most 10, and the factor's own ulps
            d = abs(got - want)
            SEEN["trace_step_clip"] = max(SEEN["trace_step_clip"], d / span)
            assert d <= lim * float(np.spacing(np.float64(want))) + 10 * lim * span, (what, n, f, got, want)
        else:
            # h = t_new - t (h_abs_loc = |h|, h_last an earlier h): the difference of two times, each within the
            # time bound, so within twice that; where t and t_new agree with scipy's it is scipy's h bit for bit.
            # Its distance in its own ulps is recorded too (one ulp of t is 2^5 ulps of a step of 0.02).
            d = abs(got - want) / span
            SEEN["trace_h"] = max(SEEN["trace_h"], d)
            SEEN["trace_h_own"] = max(SEEN["trace_h_own"], R.ulps(got, want))
            assert d <= 2 * lim, (what, n, f, got, want, d)


def _ints_ok(n, rec, e, what, batch):
    fields = ("status", "active", "rejected", "nfev", "n_acc") + (("yi",) if batch else ())
    for f in fields:
        assert int(getattr(rec, f)) == int(e[f]), (what, n, f, int(getattr(rec, f)), e[f])
    if batch:
        assert tuple(rec.kidx[:]) == e["kidx"], (what, n, tuple(rec.kidx[:]), e["kidx"])


# ================================================================================== 1. batch controller
class _Batch:
    """A device-controlled workspace driven through its control kernel alone (what = 1)."""

    def __init__(self, heads, rows, status_words):
        from genpose2_amd import _lib, ode
        self.lib, self.heads, self.rows, self.ode = _lib.load(), heads, rows, ode
        self.rec = ctypes.sizeof(ode.OdeCtl)
        assert self.rec == int(self.lib.gp_ode_ctl_size()) == 208
        self.nbytes = int(self.lib.gp_ode_auto_workspace_size(rows))
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device=DEV)
        self.part_off = int(self.lib.gp_ode_auto_partials_offset())
        assert self.part_off == 2 * self.rec + 6 * 768 * 4
        self.nwg = int(self.lib.gp_ode_global_partials(rows, rows, 1, int(heads.w.pe2_h is not None)))
        assert self.part_off + 8 * self.nwg <= self.nbytes
        self.part = self.ws[self.part_off:self.part_off + 8 * self.nwg].view(torch.float64)
        self.dummy = torch.zeros(16, dtype=torch.float64, device=DEV)
        self.hv, self.hdev = status_words[0].numpy(), status_words[1]
        self.count = rows * 9

    def control(self, n, t_bound, direction):
        d = _vp(self.dummy)
        _lib_check(self.lib.gp_ode_auto_attempt_hs(
            ctypes.byref(self.heads.w), d, n, 1, float(t_bound), float(direction), RTOL, ATOL, SIG_MIN, BASE, DIFF,
            d, d, _ptrs([self.dummy] * 7), _np_p(A6), _np_p(B6), _np_p(E7), self.rows, 1, _vp(self.ws), self.nbytes,
            ctypes.c_void_p(self.hdev), _stream()), "ode_auto_attempt_hs")
        torch.cuda.synchronize()
        off = ((n + 1) & 1) * self.rec
        raw = bytes(self.ws[off:off + self.rec].cpu().numpy())
        return self.ode.OdeCtl.from_buffer_copy(raw), raw

    def run(self, t0, t_bound, h0, sums, ncalls):
        """Control calls 0 .. ncalls - 1 with attempt n's error fed as partials summing to sums[n]; then one more
        call, which must leave the finished record as it is. Returns [(record, time rows, status word)]."""
        direction = 1.0 if t_bound > t0 else -1.0
        self.ws.zero_()
        c0 = self.ode.OdeCtl(t=t0, h_abs=h0, nfev=R.NFEV0)
        c0.kidx[:] = list(range(7))
        self.ws[:self.rec].copy_(torch.frombuffer(bytearray(bytes(c0)), dtype=torch.uint8))
        self.hv[:] = -1
        out = []
        for n in range(ncalls + 1):
            if n > 0 and n - 1 < len(sums):
                a, b = R.split(sums[n - 1])
                p = np.zeros(self.nwg)
                if self.nwg == 1:
                    p[0] = sums[n - 1]
                else:
                    p[0], p[-1] = a, b        # the last partial: the sum's second trip from 257 partials on
                self.part.copy_(torch.from_numpy(p))
            else:
                self.part.fill_(float("nan"))
            rec, raw = self.control(n, t_bound, direction)
            rows = self.ws[2 * self.rec:self.part_off].view(torch.float32).view(6, 768).clone() if rec.active else None
            out.append((rec, rows, int(self.hv[n & 3]), raw))
        return out


def _lib_check(rc, what):
    from genpose2_amd import _lib
    _lib.check(rc, what)


def _check_batch_run(b, name, t0, tb, h0, errs, exact, nfev=None):
    sums, eff = R.script_sums(errs, b.count)
    tr = R.run_script(t0, tb, h0, eff)
    exp = R.expected_records(tr)
    got = b.run(t0, tb, h0, sums, len(exp))
    assert len(got) == len(exp) + 1
    for n, e in enumerate(exp):
        rec, rows, word, _ = got[n]
        _ints_ok(n, rec, e, name, batch=True)
        _floats_ok(n, rec, e, tr, exact, name)
        assert word == 4 * n + e["status"] + 1, (name, n, word)
        if rec.active:
            _stage_scalars_ok(rec, rows, b.heads)
    last = exp[-1]
    assert last["status"] == tr.status and (nfev is None or last["nfev"] == nfev)
    if tr.status < 0:   # the step that failed: below the spacing of t, the last rejected one times scipy's factor
        rec = got[len(exp) - 1][0]
        assert rec.h_abs_loc < R.min_step(rec.t, tr.direction)
    # the speculative control after the end (ode._attempts_polled launches one): the record stays as it is
    n = len(exp)
    assert got[n][3][:204] == got[n - 1][3][:204], (name, "record changed after the solve ended")
    assert got[n][2] == 4 * n + tr.status + 1
    return tr


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("rows", [1, 16, 50])
def test_batch_controller_clamped_scripts_vs_scipy(heads, status_words, rows, direction):
    """Every control call of every clamped script (tests/ode_blocks_ref.py clamped_scripts: err == 1, the largest
    error below 1, the 0.2 and 10 clamps, err == 0, min(1, .) after rejections, the clipped and the exactly landing
    last step, NaN until status -1, h_abs below min_step, Inf), backward (1 -> 1e-5) and forward: decisions,
    counters, the FSAL slot swap and every float field equal scipy's bit for bit; t32 exact, sigma within 1 float32
    ulp, coef within 8 float64 ulps, the six time rows equal to time_proj, the host-mapped word 4 n + status + 1,
    and a control call after the end changes nothing. Measured on MI355X: see test_zz_report_distances."""
    heads.set_arith("f32")
    b = _Batch(heads, rows, status_words)
    for name, (t0, tb, h0, errs) in R.clamped_scripts(direction).items():
        tr = _check_batch_run(b, name, t0, tb, h0, errs, exact=True)
        if name == "nan_fail":
            assert tr.status == -1 and (direction > 0 or tr.n_reject == 19)


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("rows", [1, 16, 50])
def test_batch_controller_trace_scripts_vs_scipy(heads, status_words, golden_trace, rows, direction):
    """The four committed error sequences (golden_ode_trace.json) with h_abs from their first attempt: decisions and
    counters exact, nfev 290 / 278 / 134 / 134, float fields within (n + 1) * 4 float64 ulps after control call n
    (times relative to |t0 - t_bound|, the carried step size to the value itself; h = t_new - t as a difference of
    two times: the module docstring). No decision depends on that drift: the errors are scripted and the clip yields
    t_bound itself."""
    heads.set_arith("f32")
    b = _Batch(heads, rows, status_words)
    for name, (t0, tb, h0, errs, nfev) in R.trace_scripts(golden_trace, direction).items():
        tr = _check_batch_run(b, name, t0, tb, h0, errs, exact=False, nfev=nfev)
        assert tr.status == 1 and tr.t == tb and tr.unused == 0


@pytest.mark.parametrize("arith,rows,nwg", [("f32", 4112, 257), ("f16x3", 8250, 129)])
def test_batch_controller_many_partials(heads, status_words, arith, rows, nwg):
    """257 partials of 16 rows (the fixed-order sum's second trip) and 129 partials of 64 rows: the error's sum
    sits in the first and the last partial."""
    heads.set_arith(arith)
    try:
        b = _Batch(heads, rows, status_words)
        assert b.nwg == nwg
        t0, tb, h0, errs = R.clamped_scripts(-1)["edges"]
        _check_batch_run(b, f"edges@{rows}", t0, tb, h0, errs, exact=True)
    finally:
        heads.set_arith("f16x3")


# ================================================================================== 2. per-object controller
class _Objects:
    def __init__(self, heads, nobj, kper, status_words, seed=3):
        from genpose2_amd import _lib
        self.lib, self.heads, self.nobj, self.kper = _lib.load(), heads, nobj, kper
        self.rs = ctypes.sizeof(OdeObjRec)
        assert self.rs == int(self.lib.gp_debug_ode_obj_rec_size()) == 168
        g = torch.Generator().manual_seed(seed)
        # object b's row is the same whatever nobj is
        self.pobj = torch.randn((70, 768), generator=g)[:nobj].contiguous().to(DEV)
        self.recs = torch.zeros((2, nobj, self.rs), dtype=torch.uint8, device=DEV)
        self.rowsq = torch.zeros(nobj * kper, dtype=torch.float64, device=DEV)
        self.init = torch.empty((6, nobj, 768), dtype=torch.float32, device=DEV)
        self.count = torch.zeros(32, dtype=torch.int64, device=DEV)
        self.dstat = torch.zeros(64, dtype=torch.int32, device=DEV)
        self.hv, self.hdev = status_words[0].numpy(), status_words[1]

    def run(self, scripts, t_bound, direction):
        """scripts: per object (t0, h0, sums, ncalls). Calls control until no object runs, then once more. Returns
        per call: (records (nobj) , raw bytes (nobj, 168), status word, device status word)."""
        nobj, kper = self.nobj, self.kper
        first = (OdeObjRec * nobj)()
        for b, (t0, h0, _, _) in enumerate(scripts):
            first[b].t, first[b].h_abs, first[b].nfev = t0, h0, R.NFEV0
        self.recs.zero_()
        self.recs[0].copy_(torch.frombuffer(bytearray(bytes(first)), dtype=torch.uint8).view(nobj, self.rs))
        self.init.fill_(float("nan"))
        self.count.zero_()
        self.hv[:] = -1
        total = max(s[3] for s in scripts)
        out = []
        for n in range(total + 1):
            rq = np.full((nobj, kper), np.nan)          # a row sum no running object owns must not be read
            for b, (_, _, sums, ncalls) in enumerate(scripts):
                if 0 < n < ncalls:
                    S = sums[n - 1]
                    rq[b] = 0.0
                    if kper == 1:
                        rq[b, 0] = S
                    else:
                        rq[b, 0], rq[b, -1] = R.split(S)   # the last row: lane (k - 1) % 64, its second trip at k = 70
            self.rowsq.copy_(torch.from_numpy(rq.reshape(-1)))
            before = self.init.clone()
            _lib_check(self.lib.gp_debug_ode_obj_control(
                ctypes.byref(self.heads.w), _vp(self.pobj), _vp(self.recs[n & 1]), _vp(self.recs[(n + 1) & 1]),
                _vp(self.rowsq), int(n > 0), n, float(t_bound), float(direction), kper, nobj, _vp(self.init),
                _vp(self.count), ctypes.c_void_p(self.hdev), _vp(self.dstat), _stream()), "debug_ode_obj_control")
            torch.cuda.synchronize()
            raw = self.recs[(n + 1) & 1].cpu().numpy().copy()
            recs = [OdeObjRec.from_buffer_copy(bytes(raw[b])) for b in range(nobj)]
            assert int(self.count[0]) == 0, ("arrival counter not zeroed", n)
            self._init_ok(recs, before, n)
            out.append((recs, raw, int(self.hv[n & 3]), int(self.dstat[0])))
        return out

    def _init_ok(self, recs, before, n):
        """init[s][b] = pobj[b] + time_proj(t32[b][s]) (one fp32 add) for the objects that run; the rest untouched."""
        act = [b for b, r in enumerate(recs) if r.active]
        idle = [b for b, r in enumerate(recs) if not r.active]
        if act:
            t32 = np.array([recs[b].t32[:] for b in act], dtype=np.float32)                 # (na, 6)
            tp = self.heads.time_proj(torch.from_numpy(t32.reshape(-1)).to(DEV)).view(len(act), 6, 768)
            want = (self.pobj[act][:, None, :] + tp).permute(1, 0, 2).contiguous()          # (6, na, 768)
            got = self.init[:, act, :].contiguous()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), ("init rows", n)
        if idle:
            assert torch.equal(self.init[:, idle, :].contiguous().view(torch.int32),
                               before[:, idle, :].contiguous().view(torch.int32)), ("idle object's rows written", n)


def _object_scripts(golden_trace, direction, count):
    """name -> (t0, h0, sums, expected records, trace, exact, t_bound). One launch has one t_bound: the T0 = 0.55
    traces run forward end at 0.55, so forward they run in launches of their own."""
    out = {}
    tb = R.interval(direction)[1]
    for name, (t0, sb, h0, errs) in R.clamped_scripts(direction).items():
        assert sb == tb
        sums, eff = R.script_sums(errs, count)
        tr = R.run_script(t0, tb, h0, eff)
        out[name] = (t0, h0, sums, R.expected_records(tr), tr, True, tb)
    for name, (t0, sb, h0, errs, nfev) in R.trace_scripts(golden_trace, direction).items():
        sums, eff = R.script_sums(errs, count)
        tr = R.run_script(t0, sb, h0, eff)
        assert tr.nfev == nfev and tr.status == 1
        out[name] = (t0, h0, sums, R.expected_records(tr), tr, False, sb)
    return out, tb


def _check_objects(o, names, scripts, direction):
    S = [scripts[nm] for nm in names]
    tb = S[0][6]
    assert all(s[6] == tb for s in S)
    got = o.run([(s[0], s[1], s[2], len(s[3])) for s in S], tb, direction)
    total = max(len(s[3]) for s in S)
    assert len(got) == total + 1
    for n, (recs, raw, word, dword) in enumerate(got):
        running = False
        for b, (nm, s) in enumerate(zip(names, S)):
            exp, tr, exact = s[3], s[4], s[5]
            what = f"object {b} ({nm})"
            if n < len(exp):
                e = exp[n]
                _ints_ok(n, recs[b], e, what, batch=False)
                _floats_ok(n, recs[b], e, tr, exact, what)
                # pend: the attempt this call decided was accepted (y_new / K_6 not yet copied to y / K_0)
                pend = int(n > 0 and tr.attempts[n - 1]["accepted"])
                assert recs[b].pend == pend, (what, n, recs[b].pend, pend)
                if recs[b].active:
                    _stage_scalars_ok(recs[b], None, o.heads)
                    running = True
                if n == len(exp) - 1 and tr.status < 0:
                    assert recs[b].h_abs_loc < R.min_step(recs[b].t, direction)
            else:   # finished or failed earlier: byte-identical while the others go on
                assert bytes(raw[b]) == bytes(got[n - 1][1][b]), (what, n, "changed after it ended")
        want = 4 * n + (1 if running else 2)
        assert word == want and dword == want, (n, word, dword, want)
    assert got[-1][2] & 3 == 2
    return got


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("kper", [1, 10, 70])
@pytest.mark.parametrize("nobj", [1, 3, 70])
def test_object_controller_vs_scipy(heads, status_words, golden_trace, nobj, kper, direction):
    """ode_obj_control_kernel alone (gp_debug_ode_obj_control), one script per object in one launch: every object
    follows its own scipy instance as in the batch test (pend included), objects that finished or failed stay
    byte-identical while others run, the status words read 4 n + 1 while any object runs and 4 n + 2 once none
    does, the arrival counter is zero after every call, init[s][b] = pobj[b] + time_proj(t32[b][s]) bitwise, and
    object 0's records are the same alone and among 69 others. k = 70 takes the wave sum's second trip. nobj = 1
    runs every script in turn; nobj = 3 holds a failing, an at-once finishing and a long-running object. A launch
    has one t_bound, so forward the two T0 = 0.55 traces (which end at 0.55) run in launches of their own."""
    heads.set_arith("f32")
    scripts, tb = _object_scripts(golden_trace, direction, kper * 9)
    names = list(scripts)
    o = _Objects(heads, nobj, kper, status_words)
    if nobj == 1:
        for nm in names:
            _check_objects(o, [nm], scripts, direction)
    elif nobj == 3:
        _check_objects(o, ["nan_fail", "land_exact", "edges"], scripts, direction)
        _check_objects(o, ["clamp_low", "t1_none_ref32", "min_step"], scripts, direction)
        _check_objects(o, ["t055_s20_ref32", "t055_s20_ref64", "t055_s20_ref32"], scripts, direction)
    else:
        names = [nm for nm in names if scripts[nm][6] == tb]     # 9 scripts backward, 7 forward
        order = [names[b % len(names)] for b in range(nobj)]
        full = _check_objects(o, order, scripts, direction)
        alone = _check_objects(_Objects(heads, 1, kper, status_words), order[:1], scripts, direction)
        for n in range(len(alone)):
            assert bytes(alone[n][1][0]) == bytes(full[n][1][0]), ("object 0 alone vs among 69 others", n)
        for n in range(len(alone), len(full)):
            assert bytes(full[n][1][0]) == bytes(alone[-1][1][0])


# ================================================================================== 3. init norms, dense output
def _mixed(rng, n):
    """Mixed magnitudes with zeros: the scale atol + |y| rtol crosses from atol- to rtol-dominated."""
    v = rng.normal(size=n) * 10.0 ** rng.integers(-8, 4, size=n)
    v[rng.random(n) < 0.1] = 0.0
    return v


@pytest.mark.parametrize("n", [1, 9, 1023, 1024, 1025, 8191, 8192, 8193, 9 * 12800 + 7])
def test_init_norms_vs_fsum(n):
    """gp_ode_init_norms around the 1024-thread and the 8 x 1024 interleave boundaries, with and without f1,
    against math.fsum in float64. The terms are non-negative, so any order of the sum is within n 2^-53 of it and the
    square root halves that: n 2^-52 relative covers it. Only out[0], out[1] (without f1) or out[2] (with f1) may
    change."""
    from genpose2_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n)
    y0, f0, f1 = _mixed(rng, n), _mixed(rng, n), _mixed(rng, n)
    d = [torch.from_numpy(v).to(DEV) for v in (y0, f0, f1)]
    SENT = -12345.678
    out = torch.full((8,), SENT, dtype=torch.float64, device=DEV)
    _lib.check(lib.gp_ode_init_norms(_vp(d[0]), _vp(d[1]), None, n, ATOL, RTOL, _vp(out), _stream()), "init_norms")
    got = out.cpu().numpy().copy()
    d0, d1 = R.init_norms_ref(y0, f0, None, ATOL, RTOL)
    bound = n * EPS64
    print(f"n={n}: d0 abs {abs(got[0] - d0):.2e} of {d0:.3e}, d1 abs {abs(got[1] - d1):.2e} of {d1:.3e} "
          f"(relative bound {bound:.2e})")
    assert abs(got[0] - d0) <= bound * d0 and abs(got[1] - d1) <= bound * d1
    assert np.all(got[2:] == SENT)
    out.fill_(SENT)
    _lib.check(lib.gp_ode_init_norms(_vp(d[0]), _vp(d[1]), _vp(d[2]), n, ATOL, RTOL, _vp(out), _stream()), "init_norms")
    got = out.cpu().numpy().copy()
    d2 = R.init_norms_ref(y0, f0, f1, ATOL, RTOL)
    print(f"n={n}: d2 abs {abs(got[2] - d2):.2e} of {d2:.3e}")
    assert abs(got[2] - d2) <= bound * d2
    assert np.all(got[:2] == SENT) and np.all(got[3:] == SENT)


NB = 9                                            # rows of the dense output buffer
TEV = np.array([0.93, 0.92, 0.909, 0.907, 0.905, 0.903, 0.9, 0.89, 0.88])   # the step [0.9, 0.91] holds 2..6


@pytest.mark.parametrize("h", [-0.01, 0.01])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 450])
def test_dense_output_vs_scipy(n, h):
    """gp_ode_dense against scipy's RkDenseOutput on the same K (7, n), y_old, t_old and h: 0, 1 and 5 t_eval points
    per call with i0 > 0, reverse 0 / 1 with i_base placing the rows first, last and mid-buffer of a NaN-filled
    buffer (rows outside [i0, i1) stay NaN). Per element within 64 2^-52 (|y_old| + |h| sum_jm |K_j| |P_jm| |x|^m)."""
    from genpose2_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7 * n + (h > 0))
    K = _mixed(rng, 7 * n).reshape(7, n)
    y_old = _mixed(rng, n)
    t_old = 0.91 if h < 0 else 0.9
    tev = TEV if h < 0 else TEV[::-1].copy()
    kd = [torch.from_numpy(np.ascontiguousarray(K[j])).to(DEV) for j in range(7)]
    yd, td = torch.from_numpy(y_old).to(DEV), torch.from_numpy(tev).to(DEV)
    worst = 0.0
    for i0, i1 in ((2, 2), (2, 3), (2, 7)):
        m = i1 - i0
        ref, mag = R.dense_ref(K, y_old, t_old, h, tev[i0:i1])
        for reverse in (0, 1):
            for place in ("first", "last", "mid"):
                lo = {"first": 0, "last": NB - m, "mid": 2}[place]          # rows [lo, lo + m) are written
                i_base = (lo + m - 1 + i0) if reverse else (i0 - lo)
                rows = [(i_base - i) if reverse else (i - i_base) for i in range(i0, i1)]
                assert all(0 <= r < NB for r in rows)
                out = torch.full((NB, n), float("nan"), dtype=torch.float64, device=DEV)
                _lib.check(lib.gp_ode_dense(_ptrs(kd), _np_p(P74), _vp(yd), _vp(td), i0, i1, i_base, reverse,
                                            float(t_old), float(h), n, _vp(out), _stream()), "ode_dense")
                got = out.cpu().numpy()
                for j, r in enumerate(rows):
                    err = np.abs(got[r] - ref[j])
                    nz = mag[j] > 0            # x == 0 on a zero of y_old: the element must be 0 itself
                    worst = max(worst, float((err[nz] / mag[j][nz]).max()) if nz.any() else 0.0)
                    assert np.all(err <= 64 * EPS64 * mag[j]), (n, h, i0, i1, reverse, place, j)
                rest = [r for r in range(NB) if r not in rows]
                assert np.isnan(got[rest]).all(), (n, h, i0, i1, reverse, place)
    print(f"n={n} h={h}: largest |got - scipy| / magnitude {worst:.2e} (bound {64 * EPS64:.2e})")


# ================================================================================== 4. one attempt, teacher-forced
PAD = 64      # NaN rows behind every (R,9) buffer: rows >= R of nothing are written


@pytest.fixture(scope="module")
def p64(score_sd):
    return R.head_params(score_sd, np.float64)


def _padded(v, rows):
    t = torch.full(((rows + PAD) * 9,), float("nan"), dtype=torch.float64, device=DEV)
    if v is not None:
        t[:rows * 9].copy_(torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))
    return t


def _head_bar(got, ref, what):
    rel = float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())
    assert rel < 1e-5, (what, rel)
    return rel


def _check_attempt(p64, feat, k, rows, y, Kd, ynew, h, t32_6, coef_6, part, nwg, err_out, what):
    """Kd (7, rows*9), ynew (rows*9): what the device wrote; part: every error partial the workspace holds."""
    y = y.reshape(-1)
    worst = 0.0
    for s in range(1, 7):
        xin, mag = R.stage_input(y, Kd, s, h)
        if s == 6:
            assert np.all(np.abs(ynew - xin) <= 64 * EPS64 * mag), (what, "y_new")
            xin = ynew                      # K_6 = f(t + h, y_new) of the y_new the device formed
        ref = coef_6[s - 1] * R.score_np(p64, feat, k, xin.astype(np.float32).reshape(rows, 9), t32_6[s - 1])
        worst = max(worst, _head_bar(Kd[s].reshape(rows, 9), ref, f"{what} stage {s}"))
    S_ref, m2 = R.err_sum_ref(y, ynew, Kd, h, ATOL, RTOL)
    assert np.isfinite(part[:nwg]).all() and np.isnan(part[nwg:]).all(), (what, "partials", nwg)
    S_dev = math.fsum(part[:nwg].tolist())
    # a term's fp64 reordering is within 16 2^-53 of its magnitude m, so its square within 16 2^-52 m^2; the sums
    # (at most ~30 roundings deep, of non-negative terms) add 15 2^-52 of the total: 64 2^-52 sum(m^2) covers both
    tol = 64 * EPS64 * m2
    assert abs(S_dev - S_ref) <= tol, (what, "error partials", S_dev, S_ref, tol)
    if err_out is not None:
        want = math.sqrt(S_ref) / math.sqrt(9 * rows)
        assert abs(err_out - want) <= want * (0.5 * tol / S_ref + 4 * EPS64), (what, "error norm", err_out, want)
    return worst, math.sqrt(S_ref / (9 * rows))


def _attempt_both_paths(heads, p64, arith, rows, k, monkeypatch):
    from genpose2_amd import _lib, ode
    lib = _lib.load()
    monkeypatch.delenv("GENPOSE2_ODE_FUSED", raising=False)
    heads.set_arith(arith)
    split = int(heads.w.pe2_h is not None)
    nwg = int(lib.gp_ode_global_partials(rows, rows, 1, split))
    for t, std, h in R.ATTEMPT_TIMES:
        feat, y = R.attempt_inputs(rows, k, std)
        pobj = heads.object_proj(torch.from_numpy(feat).to(DEV))
        what = f"{arith} {rows}x{k} t={t} h={h}"
        # ---- K_0 = f(t, y): gp_ode_rhs
        t32, sig, coef = R.stage_scalars([t])
        ws = torch.full((int(lib.gp_ode_workspace_size(rows)),), 0xFF, dtype=torch.uint8, device=DEV)
        yd, k0 = _padded(y, rows), _padded(None, rows)
        _lib.check(lib.gp_ode_rhs(ctypes.byref(heads.w), _vp(pobj), float(t32[0]), float(sig[0]), float(coef[0]),
                                  _vp(yd), None, None, 0, 0.0, rows, k, _vp(k0), _vp(ws), ws.numel(), _stream()),
                   "ode_rhs")
        k0h = k0.cpu().numpy()
        assert np.isnan(k0h[rows * 9:]).all()
        ref = coef[0] * R.score_np(p64, feat, k, y.astype(np.float32), t32[0])
        r0 = _head_bar(k0h[:rows * 9].reshape(rows, 9), ref, f"{what} rhs")

        # ---- stage launches: gp_ode_attempt
        t32_6, sig_6, coef_6 = R.stage_scalars(R.stage_times(t, h))
        Ks = [k0.clone()] + [_padded(None, rows) for _ in range(6)]
        ynew = _padded(None, rows)
        err = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
        ws.fill_(0xFF)
        _lib.check(lib.gp_ode_attempt(ctypes.byref(heads.w), _vp(pobj), _np_p(t32_6), _np_p(sig_6), _np_p(coef_6),
                                      _vp(yd), _ptrs(Ks), _np_p(A6), _np_p(B6), _np_p(E7), float(h), RTOL, ATOL, rows,
                                      k, _vp(ynew), _vp(err), _vp(ws), ws.numel(), _stream()), "ode_attempt")
        Kh = np.stack([v.cpu().numpy() for v in Ks], 0)
        yh, eh = ynew.cpu().numpy(), err.cpu().numpy()
        assert np.isnan(Kh[:, rows * 9:]).all() and np.isnan(yh[rows * 9:]).all() and np.isnan(eh[1:]).all()
        assert np.array_equal(Kh[0, :rows * 9], k0h[:rows * 9])
        part = ws[6 * 768 * 4:].cpu().numpy()
        part = part[:part.size // 8 * 8].view(np.float64)
        w1, e1 = _check_attempt(p64, feat, k, rows, y, Kh[:, :rows * 9], yh[:rows * 9], h, t32_6, coef_6, part, nwg,
                                float(eh[0]), what + " stages")

        # ---- the fused kernel on a hand-written record: gp_ode_auto_attempt what = 3, attempt 0
        nb = int(lib.gp_ode_auto_workspace_size(rows))
        aws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
        rec = ctypes.sizeof(ode.OdeCtl)
        kidx = [6, 2, 3, 4, 5, 1, 0]                      # logical K_j lives in buffer kidx[j]
        c0 = ode.OdeCtl(t=t, h_abs=abs(h), nfev=R.NFEV0, yi=1)
        c0.kidx[:] = kidx
        aws[:rec].copy_(torch.frombuffer(bytearray(bytes(c0)), dtype=torch.uint8))
        bufs = [_padded(None, rows) for _ in range(7)]
        bufs[kidx[0]].copy_(k0)
        ybuf = [_padded(None, rows), yd]                   # yi = 1: the state is in buffer 1, y_new goes to 0
        direction = 1.0 if h > 0 else -1.0
        tb = 1.0 if h > 0 else 1e-5
        _lib.check(lib.gp_ode_auto_attempt(ctypes.byref(heads.w), _vp(pobj), 0, 3, tb, direction, RTOL, ATOL, SIG_MIN,
                                           BASE, DIFF, _vp(ybuf[0]), _vp(ybuf[1]), _ptrs(bufs), _np_p(A6), _np_p(B6),
                                           _np_p(E7), rows, k, _vp(aws), nb, _stream()), "ode_auto_attempt")
        torch.cuda.synchronize()
        c1 = ode.OdeCtl.from_buffer_copy(bytes(aws[rec:2 * rec].cpu().numpy()))
        assert c1.active == 1 and c1.status == 0 and c1.yi == 1 and list(c1.kidx[:]) == kidx and c1.nfev == R.NFEV0
        assert c1.h == (t + abs(h) * direction) - t and c1.t == t
        Kh = np.stack([bufs[kidx[j]].cpu().numpy() for j in range(7)], 0)
        yh = ybuf[0].cpu().numpy()
        assert np.isnan(Kh[:, rows * 9:]).all() and np.isnan(yh[rows * 9:]).all()
        assert np.array_equal(Kh[0, :rows * 9], k0h[:rows * 9])
        assert torch.equal(ybuf[1][:rows * 9], yd[:rows * 9])
        off = int(lib.gp_ode_auto_partials_offset())
        part = aws[off:].cpu().numpy()
        part = part[:part.size // 8 * 8].view(np.float64)
        w2, e2 = _check_attempt(p64, feat, k, rows, y, Kh[:, :rows * 9], yh[:rows * 9], float(c1.h),
                                np.array(c1.t32[:], dtype=np.float32), np.array(c1.coef[:]), part, nwg, None,
                                what + " fused")
        print(f"  {what}: K vs float64 per-row relative max: rhs {r0:.2e}, stages {w1:.2e}, fused {w2:.2e}; "
              f"error norm {e1:.3g} / {e2:.3g}")


@pytest.mark.parametrize("arith", ["f32", "f16x3"])
@pytest.mark.parametrize("rows,k", R.ATTEMPT_SHAPES)
def test_one_attempt_teacher_forced(heads, p64, monkeypatch, arith, rows, k):
    """gp_ode_rhs, gp_ode_attempt (stage launches) and gp_ode_auto_attempt what=3 on a hand-written record (the
    fused kernel; the state in buffer 1 and the K slots permuted), both arithmetics, y ~ N(0, 50^2) at t = 1 with
    h < 0 and N(0, 1) at t = 0.1 with h > 0, workspace and K slots NaN-filled first. From the K's the device wrote:
    every stage K_s against coef_s score64(float32(y + h sum_j A[s][j] K_j), t32_s) at 1e-5 of the row's max |ref|
    (no accumulation across stages); y_new and the error partials' sum against float64 NumPy within 64 2^-52 of the
    summed magnitudes (the tableau, the scale and the masking of the ragged last tile, independent of the network's
    precision); partials past the last workgroup and rows >= R of every buffer stay NaN."""
    try:
        _attempt_both_paths(heads, p64, arith, rows, k, monkeypatch)
    finally:
        heads.set_arith("f16x3")


@pytest.mark.parametrize("rows,k", R.ATTEMPT_SHAPES_X3)
def test_one_attempt_teacher_forced_wide_tiles(heads, p64, monkeypatch, rows, k):
    """The same at the f16x3 trunk's 32-row (4097 = 17 x 241) and 64-row (8193 = 3 x 2731) tiles, each with a
    one-row last tile."""
    _attempt_both_paths(heads, p64, "f16x3", rows, k, monkeypatch)


def test_zz_report_distances():
    """Prints the largest distances the controller tests of this module measured (run it with them): sigma in
    float32 ulps, coef in float64 ulps, and the trace scripts' float fields in float64 ulps."""
    print("largest distances seen:", {k: round(v, 3) for k, v in SEEN.items()})
