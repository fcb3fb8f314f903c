"""Plain references for the RK45 solver's device building blocks (tests/test_cpu_ode_blocks.py,
tests/test_gpu_ode_blocks.py). Nothing here imports the package's arithmetic: the step controller is scipy's own
``RK45`` with its error norm scripted, the dense output scipy's ``RkDenseOutput``, the norms ``math.fsum`` in
float64 and the network float64 NumPy (weights.head_params only names the parameters).

Scripted controller. ``run_script`` drives ``scipy.integrate.RK45`` on a dummy right-hand side: ``h_abs`` is set by
the script and ``_estimate_error_norm`` pops the script's next value, so accept / reject, every step-size update,
the clip to t_bound and the failure below the spacing of t are scipy's code, line by line. The hook records, per
attempt, what ``_step_impl`` holds at that point (t, h, t_new, its local h_abs and step_rejected: read from the
caller's frame) and what the solver object holds (h_abs, t_old, h_previous, nfev). ``expected_records`` lays these
out as the controller record a device control call must leave behind.

Error norms reach a device controller as partial sums of (err / scale)^2: it forms sqrt(sum) / sqrt(count).
``err_sum`` picks the float64 sum S for a wanted error, ``effective`` is the error both sides then see,
sqrt(S) / sqrt(count) in IEEE float64 (two correctly rounded operations), and ``split`` spreads S over two partials
whose sum is exact in any order."""
import math
import sys

import numpy as np
from scipy.integrate import RK45
from scipy.integrate._ivp.rk import RkDenseOutput

NFEV0 = 2          # RK45.__init__: f(t0, y0) and select_initial_step's Euler probe
B1 = "below1"      # script token: the largest error below 1 that sqrt(S) / sqrt(count) can form

# Dormand-Prince tableau as printed in scipy's RK45 (rk.py), typed here so that the tests do not read the package's
C = RK45.C
A = RK45.A
B = RK45.B
E = RK45.E
P = RK45.P


# ------------------------------------------------------------------------------------------ scripted controller
class _Scripted(RK45):
    def _estimate_error_norm(self, K, h, scale):
        loc = sys._getframe(1).f_locals          # RK45._step_impl
        if not self.script:
            raise IndexError("error script exhausted before the solve ended")
        err = self.script.pop(0)
        self.log.append(dict(t=float(self.t), h=float(h), t_new=float(loc["t_new"]),
                             h_abs_loc=float(loc["h_abs"]), rejected=bool(loc["step_rejected"]),
                             h_abs=float(self.h_abs), t_old=self.t_old, h_last=self.h_previous,
                             nfev=int(self.nfev), err=float(err), accepted=bool(err < 1)))
        return err


class Trace:
    """attempts: the hook's records in order; steps: (t, h_abs, status, nfev) after every step(); status: 1
    finished, -1 failed; unused: errors left in the script."""

    def __init__(self, t0, t_bound, h0, attempts, steps, solver, unused):
        self.t0, self.t_bound, self.h0 = float(t0), float(t_bound), float(h0)
        self.direction = 1.0 if t_bound > t0 else -1.0
        self.attempts, self.steps, self.unused = attempts, steps, unused
        self.status = 1 if solver.status == "finished" else -1
        self.t, self.h_abs, self.nfev = float(solver.t), float(solver.h_abs), int(solver.nfev)
        self.t_old, self.h_last = solver.t_old, solver.h_previous
        self.n_reject = sum(not a["accepted"] for a in attempts)
        self.n_accept = sum(a["accepted"] for a in attempts)


def run_script(t0, t_bound, h0, errs):
    s = _Scripted(lambda t, y: np.zeros_like(y), float(t0), np.zeros(1), float(t_bound), rtol=1e-5, atol=1e-5)
    assert s.nfev == NFEV0
    s.h_abs = float(h0)
    s.script, s.log = [float(e) for e in errs], []
    steps = []
    while s.status == "running":
        s.step()
        steps.append((float(s.t), float(s.h_abs), s.status, int(s.nfev)))
    return Trace(t0, t_bound, h0, s.log, steps, s, len(s.script))


def expected_records(tr):
    """The controller record after control call n, n = 0 .. len(attempts): call n decides attempt n - 1 and prepares
    attempt n; the last one ends the solve. A field that scipy does not define at that point is None. clip: the
    record's h_abs was formed from a step clipped to t_bound."""
    out, n_acc, kidx, clip = [], 0, list(range(7)), False
    for a in tr.attempts:
        out.append(dict(status=0, active=1, rejected=int(a["rejected"]), nfev=a["nfev"] - 6, n_acc=n_acc,
                        yi=n_acc & 1, kidx=tuple(kidx), t=a["t"], h_abs=a["h_abs"], t_old=a["t_old"],
                        h_last=a["h_last"], h=a["h"], t_new=a["t_new"], h_abs_loc=a["h_abs_loc"], clip=clip))
        if a["accepted"]:
            n_acc += 1
            kidx[0], kidx[6] = kidx[6], kidx[0]      # FSAL: f = f_new
            clip = a["t_new"] == tr.t_bound          # h_abs = |t_bound - t| * factor from here on
    out.append(dict(status=tr.status, active=0, rejected=int(tr.status < 0), nfev=tr.nfev, n_acc=n_acc,
                    yi=n_acc & 1, kidx=tuple(kidx), t=tr.t, h_abs=tr.h_abs, t_old=tr.t_old, h_last=tr.h_last,
                    h=None, t_new=None, h_abs_loc=None, clip=clip))
    return out


def min_step(t, direction):
    return 10 * abs(np.nextafter(t, direction * np.inf) - t)


# ------------------------------------------------------------------------------------------ errors as partial sums
def effective(S, count):
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(S)) / np.sqrt(np.float64(count)))


def err_sum(err, count):
    """The float64 S fed to the device for a wanted error norm (B1: the largest S whose error is below 1)."""
    if isinstance(err, str):
        assert err == B1
        S = float(np.nextafter(np.float64(count), 0.0))
        while not effective(S, count) < 1.0:
            S = float(np.nextafter(np.float64(S), 0.0))
        return S
    err = float(err)
    if err == 1.0:
        return float(count)
    with np.errstate(over="ignore"):
        return float(np.float64(err) * np.float64(err) * np.float64(count))


def split(S):
    """(a, b) with a + b == S exactly in any order: a the power of two at or below S."""
    if not (math.isfinite(S) and S > 0.0):
        return S, 0.0
    m, e = math.frexp(S)
    a = math.ldexp(0.5, e)
    b = S - a
    assert a + b == S and (b == 0.0 or abs(b) < a)
    return a, b


def script_sums(errs, count):
    """(S per attempt, the error both sides see per attempt)."""
    S = [err_sum(e, count) for e in errs]
    return S, [effective(s, count) for s in S]


# ------------------------------------------------------------------------------------------ the scripts
ZEROS = [0.0] * 40       # tail: every further step accepted with the factor clamped to 10, until t_bound clips


def interval(direction):
    return (1.0, 1e-5) if direction < 0 else (1e-5, 1.0)


def clamped_scripts(direction):
    """name -> (t0, t_bound, h0, errors). Every error's factor is fixed by a clamp (0.2, 10, min(1, .)) or is exact
    (err = 1 and the largest error below 1: pow gives 1), so each float a control call writes has one right value."""
    t0, tb = interval(direction)
    nan, inf = float("nan"), float("inf")
    # forward, 1e-5 + fl(1 - 1e-5) rounds to 1 itself. Backward no float64 step leads from 1 onto 1e-5 (1 - h is a
    # multiple of 2^-53 for h in [0.5, 1], 1e-5 is not), so that script starts at 2^-16, where t0 - 1e-5 is exact.
    land =(2.0 ** -16, 1e-5, 2.0 ** -16 - 1e-5) if direction < 0 else (1e-5, 1.0, 1.0 - 1e-5)
    return {
        # err == 1 rejects (0.9), twice; accept after rejections: min(1, .); err == 0 and err <= 1e-6: 10 mid-solve;
        # the largest error below 1 accepts; a rejection mid-solve; the last step is clipped to t_bound
        "edges": (t0, tb, 0.01, [1.0, 1.0, 0.25, 0.0, B1, 1.0, 0.4, 1e-7, 1e-6] + ZEROS),
        # err >= 2000, huge and Inf: 0.2; NaN mid-solve: 0.2; accept after three rejections; again after one
        "clamp_low": (t0, tb, 0.05, [2000.0, 1e300, inf, 0.3, 1e-6, nan, 0.49, inf, B1, 0.0] + ZEROS),
        # NaN until the step falls below the spacing of t: status -1
        "nan_fail": (t0, tb, 0.01, [nan] * 64),
        # h_abs below min_step is replaced by min_step and the solve runs on
        "min_step": (t0, tb, 1e-20, [0.0, 1.0, 0.3] + ZEROS),
        # t + h == t_bound exactly, without the clip: finished by >=
        "land_exact": (land[0], land[1], land[2], [0.0]),
    }


def trace_scripts(golden_trace, direction):
    """The four committed error sequences with h_abs from their first attempt; forward: the same interval
    reversed."""
    out = {}
    for case, refs in golden_trace.items():
        for ref, d in refs.items():
            att = d["attempts"]
            t0, tb = float(att[0][0]), 1e-5
            if direction > 0:
                t0, tb = tb, t0
            out[f"{case}_{ref}"] = (t0, tb, abs(float(att[0][1])), [float(a[2]) for a in att], int(d["nfev"]))
    return out


# ------------------------------------------------------------------------------------------ norms, dense output
def init_norms_ref(y0, f0, f1, atol, rtol):
    """select_initial_step's RMS norms (scipy _ivp/common.py) with math.fsum: (d0, d1) or d2 * h0."""
    scale = atol + np.abs(y0) * rtol
    n = y0.size

    def rms(v):
        return math.sqrt(math.fsum((v * v).tolist())) / math.sqrt(n)
    if f1 is None:
        return rms(y0 / scale), rms(f0 / scale)
    return rms((f1 - f0) / scale)


def dense_ref(K, y_old, t_old, h, te):
    """scipy's RkDenseOutput at the points te -> (len(te), n), and the magnitude sum of its terms per element."""
    Q = K.T.dot(P)
    sol = RkDenseOutput(t_old, t_old + h, y_old, Q)
    sol.h = h                                    # the step's own h (t_old + h - t_old need not return it)
    y = np.stack([sol(t) for t in te], 0) if len(te) else np.zeros((0, y_old.size))
    x = (np.asarray(te, dtype=np.float64) - t_old) / h
    pw = np.abs(np.stack([x, x ** 2, x ** 3, x ** 4], 1))          # (m, 4)
    mag = np.abs(y_old)[None, :] + abs(h) * (pw @ (np.abs(K).T @ np.abs(P)).T)
    return y, mag


# ------------------------------------------------------------------------------------------ one attempt
# rows x candidates per object: one row; one object over a ragged second tile; objects straddling tiles with a
# ragged tail; every row its own object
ATTEMPT_SHAPES = ((1, 1), (17, 17), (50, 10), (33, 1))
# the f16x3 trunk's wider tiles: 32 rows from 4097 rows, 64 rows from 8193, each with a one-row last tile
ATTEMPT_SHAPES_X3 = ((4097, 241), (8193, 2731))
# (t, std of y, h): the prior's scale at t = 1 stepping backward, unit scale at t = 0.1 stepping forward
ATTEMPT_TIMES = ((1.0, 50.0, -0.011), (0.1, 1.0, 0.004))


def attempt_inputs(rows, k, std, seed=0):
    """feat (B,1024) fp32 with a scale per object, y (rows,9) fp64 ~ N(0, std^2)."""
    assert rows % k == 0
    nobj = rows // k
    rng = np.random.default_rng(1000 * rows + k + seed)
    feat = np.maximum(rng.normal(size=(nobj, 1024)), 0).astype(np.float32)
    feat *= np.linspace(0.5, 2.0, nobj, dtype=np.float32)[:, None]
    return feat, rng.normal(size=(rows, 9)) * std


def head_params(sd, dtype):
    from genpose2_amd import weights
    return {k: np.asarray(v).astype(dtype) for k, v in weights.head_params(sd).items()}


def score_np(p, feat, k, x, t32, dtype=np.float64):
    """PoseScoreNet.forward (scorenet.py:215-275) in `dtype` NumPy: feat (B,1024) one row per object, x (B*k, 9),
    one float32 time value. The object and time terms of head layer 1 are formed once per object."""
    t = dtype(np.float32(t32))
    x = np.asarray(x).astype(dtype)
    feat = np.asarray(feat).astype(dtype)
    xp = t * p["gfp_w"] * dtype(2.0) * dtype(np.pi)
    tf = np.maximum(p["te_w"] @ np.concatenate([np.sin(xp), np.cos(xp)]) + p["te_b"], dtype(0))
    h = np.maximum(x @ p["pe0_w"].T + p["pe0_b"], dtype(0))
    pf = np.maximum(h @ p["pe2_w"].T + p["pe2_b"], dtype(0))
    out = []
    for i in range(3):
        ob = feat @ p["h1_pts"][i].T + p["h1_t"][i] @ tf + p["h1_b"][i]
        u = np.maximum(np.repeat(ob, k, 0) + pf @ p["h1_pose"][i].T, dtype(0))
        out.append(u @ p["h2_w"][i].T + p["h2_b"][i])
    sig = dtype(0.01) * dtype(np.power(np.float64(5000.0), np.float64(t)))
    return np.concatenate(out, 1) / (sig + dtype(1e-7))


def stage_scalars(ts):
    """t32, sigma(t32) (fp32) and coef = -(0.5 g(t)^2) (fp64) of stage times ts, as ode_func forms them
    (samplers.py:209-216): inputs of a host-controlled attempt."""
    ts = np.asarray(ts, dtype=np.float64)
    t32 = ts.astype(np.float32)
    sig = (np.float32(0.01) * np.power(5000.0, t32.astype(np.float64)).astype(np.float32)).astype(np.float32)
    g = 0.01 * np.power(5000.0, ts) * math.sqrt(2.0 * math.log(5000.0))
    return t32, sig, -(0.5 * (g * g))


def stage_times(t, h):
    return [t + c * h for c in C[1:]] + [t + h]


def stage_input(y, K, s, h):
    """Input of stage s = 1..5 (rk_step: y + (K[:s].T @ A[s, :s]) h) or of stage 6 (y_new = y + h K[:6].T @ B),
    with the magnitude sum of its terms."""
    a = A[s][:s] if s < 6 else B
    dy = np.dot(K[:len(a)].T, a) * h
    mag = np.abs(y) + abs(h) * np.dot(np.abs(K[:len(a)]).T, np.abs(a))
    return y + dy, mag


def err_sum_ref(y, y_new, K, h, atol, rtol):
    """scipy's _estimate_error_norm as a sum: S = sum((K.T @ E h / scale)^2) by fsum, with the sum m2 of the
    squared term magnitudes (|h| sum_j |E_j K_j| / scale)."""
    scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
    e = np.dot(K.T, E) * h / scale
    m = abs(h) * np.dot(np.abs(K).T, np.abs(E)) / scale
    return math.fsum((e * e).tolist()), math.fsum((m * m).tolist())


def ulps(a, b, ref=None):
    """|a - b| in units of the spacing of float64 at `ref` (default b)."""
    ref = b if ref is None else ref
    if a == b:
        return 0.0
    return abs(a - b) / float(np.spacing(np.float64(abs(ref))))
