"""GPU checks of the energy agent on the ODE sampler (GenPoseConfig.energy_ode): the gp_ode_*_energy entries, the
energy backend of ode.DeviceRk45 and PoseNet.pred_func, against the reference's own runs
(tests/golden/make_golden_energy_ode.py).

The energy's gradient is discontinuous at ReLU kinks, so the reference's float32 net lands only about 1e-3 from
its own float64 run and no whole-solve parity to float32 rounding exists. The checks are built around that:
1. composition, bit for bit (immune to kinks): an attempt equals six gp_energy_score_eval calls plus the stage
   arithmetic in float64 NumPy;
2. the forced trajectory: the device stepped through the float64 solve's (t, h), held to 2x the reference float32
   net's own distance from it;
3. the three controllers (fused attempts under the device controller, stage launches under the host controller,
   the C entry) agree;
4. end to end, pred_func within 2x the reference's own float32 / float64 spread over six seeds;
5. refusals, and the score agent's ODE untouched.
Every solve here is 30 rows and about 30 attempts: milliseconds."""
import ctypes
import math

import numpy as np
import pytest
import torch

import energy_ode_inputs as ei
import ode_blocks_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = ATOL = 1e-5
EPS = 1e-5
ROWS = ei.B * ei.K
A6 = np.zeros((6, 6), dtype=np.float64)
A6[:, :5] = R.A
A6 = np.ascontiguousarray(A6)
B6 = np.ascontiguousarray(R.B, dtype=np.float64)
E7 = np.ascontiguousarray(R.E, dtype=np.float64)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _np_p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _make_agent(**kw):
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    cfg = dict(device=DEV, agent_type="energy", sampler_mode=["ode"], sampling_steps=ei.STEPS, energy_ode=True)
    cfg.update(kw)
    return PoseNet(GenPoseConfig(**cfg)).eval()


@pytest.fixture(scope="module")
def score_before():
    """The score agent's pred_func ODE on golden_ode, run before this module builds its first energy agent (the
    module's first fixture: every other one depends on it)."""
    return _score_ode_run()


def _score_ode_run():
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("ode")
    tag = "t055_s20"
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=int(g[f"{tag}_steps"]))).eval()
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    data = {"pts": torch.from_numpy(g[f"{tag}_pts"]).to(DEV),
            "pts_center": torch.from_numpy(g[f"{tag}_pts_center"]).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=5, T0=float(g[f"{tag}_T0"]))
    return pose.cpu().numpy(), q.cpu().numpy(), agent.last_nfev


@pytest.fixture(scope="module")
def agent(score_before):
    return _make_agent()


class _Fx:
    def __init__(self, agent):
        from genpose2_amd import sde
        g = self.g = golden("energy_ode")
        self.h = agent.heads
        self.feat = torch.from_numpy(g["pts_feat"]).to(DEV)
        self.pobj = self.h.object_proj(self.feat)
        self.center = torch.from_numpy(g["pts_center"]).to(DEV)
        self.x0 = (torch.from_numpy(g["prior"]).to(DEV) * sde.prior_sigma(ei.T0)).contiguous()   # fp32, as _ode forms it
        self.data = {"pts": torch.zeros((ei.B, 1, 3), device=DEV), "pts_feat": self.feat, "pts_center": self.center}


@pytest.fixture(scope="module")
def fx(agent):
    return _Fx(agent)


@pytest.fixture(scope="module")
def forced(agent, fx):
    """The host-controlled energy backend stepped through trace64's (t, h), accepting where norm64 < 1: the error
    norm per attempt, the final state, and a snapshot of (y, K_0, t, h) at the middle attempt."""
    from genpose2_amd.ode import DeviceRk45
    be = DeviceRk45(fx.h, fx.pobj, fx.x0, ei.K, energy_grad=True)
    be.rhs0(ei.T0)
    tr = fx.g["trace64"]
    norms, snap = [], None
    for i, (t, h, n64) in enumerate(tr):
        t, h = np.float64(t), np.float64(h)
        if i == len(tr) // 2:
            snap = (be.y.cpu().numpy().copy(), be.K[0].cpu().numpy().copy(), float(t), float(h))
        norms.append(float(be.attempt(t, h)))
        if n64 < 1:
            be.accept(t, t + h)
    torch.cuda.synchronize()
    return np.asarray(norms), be.y.cpu().numpy().copy(), snap


# ------------------------------------------------------------------------------------------ 1. composition
def _score(fx, pobj, t32, sig, x32, k):
    """gp_energy_score_eval on float32 rows at one time value -> (rows, 9) float32."""
    trow = fx.h.time_proj(torch.tensor([t32], dtype=torch.float32).to(DEV))
    return fx.h.energy_score(pobj, trow, float(sig), torch.from_numpy(np.ascontiguousarray(x32)).to(DEV), k).cpu().numpy()


def _combine(y, Ks, a, h):
    """y + (sum_j a_j K_j) h, the terms added in order, each operation rounded on its own (rk_step's order)."""
    acc = Ks[0] * a[0]
    for j in range(1, len(a)):
        acc = acc + Ks[j] * a[j]
    return y + acc * h


def _case(fx, forced, rows, k):
    """(pobj, y, K0, t, h) of the first `rows` rows of the snapshot; k = 1: one object row per pose row."""
    y, k0, t, h = forced[2]
    assert k in (1, ei.K)
    pobj = fx.pobj if k == ei.K else fx.pobj.repeat_interleave(ei.K, 0)[:rows].contiguous()
    return pobj, y[: rows * 9].copy(), k0[: rows * 9].copy(), t, h


@pytest.mark.parametrize("rows,k", [(30, 10), (1, 10), (16, 10), (17, 10), (30, 1)])
def test_attempt_is_the_composition_bit_for_bit(agent, fx, forced, rows, k):
    """One gp_ode_attempt_energy on a state mid-solve (y, K_0, t, h of the forced run's middle attempt) against six
    gp_energy_score_eval calls on float32(y_in) and the stage arithmetic in float64 NumPy, in scipy's order: K_1..K_6
    and y_new bitwise, the error norm against math.fsum of the same terms to 1e-12 relative. One row, a full tile, a
    tile and one row, two tiles with objects straddling them, and every row its own object."""
    from genpose2_amd import _lib
    lib = _lib.load()
    pobj, y, k0, t, h = _case(fx, forced, rows, k)
    n = rows * 9
    t32, sig, coef = R.stage_scalars(R.stage_times(t, h))
    K = np.zeros((7, n))
    K[0] = k0
    for s in range(1, 7):
        yin = _combine(y, K, R.A[s][:s] if s < 6 else R.B, h)
        if s == 6:
            y_new = yin
        sc = _score(fx, pobj, t32[s - 1], sig[s - 1], yin.reshape(rows, 9).astype(np.float32), k)
        K[s] = coef[s - 1] * sc.astype(np.float64).reshape(-1)
    scale = ATOL + np.maximum(np.abs(y), np.abs(y_new)) * RTOL
    e = (_combine(np.zeros(n), K, R.E, 1.0) * h) / scale
    want = math.sqrt(math.fsum((e * e).tolist())) / math.sqrt(n)

    yd = torch.from_numpy(y).to(DEV)
    Kd = [torch.from_numpy(k0).to(DEV)] + [torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
                                            for _ in range(6)]
    ynew = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    err = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.gp_ode_workspace_size(rows)), dtype=torch.uint8, device=DEV)
    w, gw = ctypes.byref(fx.h.w), ctypes.byref(fx.h.grad_weights)
    _lib.check(lib.gp_ode_attempt_energy(w, gw, _vp(pobj), _np_p(t32), _np_p(sig), _np_p(coef), _vp(yd), _ptrs(Kd),
                                         _np_p(A6), _np_p(B6), _np_p(E7), h, RTOL, ATOL, rows, k, _vp(ynew), _vp(err),
                                         _vp(ws), ws.numel(), _stream()), "ode_attempt_energy")
    torch.cuda.synchronize()
    assert np.array_equal(ynew.cpu().numpy(), y_new)
    for s in range(1, 7):
        got = Kd[s].cpu().numpy()
        assert np.abs(got).max() > 0
        assert np.array_equal(got, K[s]), (s, np.abs(got - K[s]).max())
    got = float(err.cpu()[0])
    print(f"rows {rows} k {k}: error norm {got:.17g} vs fsum {want:.17g} ({abs(got / want - 1):.1e} relative)")
    assert abs(got / want - 1) <= 1e-12

    # gp_ode_rhs_energy: the derivative at y itself (nk = 0) and at stage 3's input (nk = 3)
    for nk, s in ((0, 0), (3, 3)):
        if nk == 0:
            t1 = R.stage_scalars([t])
            yin = y
        else:
            t1 = (t32[s - 1:s], sig[s - 1:s], coef[s - 1:s])
            yin = _combine(y, K, R.A[s][:s], h)
        sc = _score(fx, pobj, t1[0][0], t1[1][0], yin.reshape(rows, 9).astype(np.float32), k)
        ref = float(t1[2][0]) * sc.astype(np.float64).reshape(-1)
        out = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        karr = _ptrs(Kd[:nk]) if nk else None
        aarr = (ctypes.c_double * nk)(*R.A[s][:s]) if nk else None
        _lib.check(lib.gp_ode_rhs_energy(w, gw, _vp(pobj), float(t1[0][0]), float(t1[1][0]), float(t1[2][0]), _vp(yd),
                                         karr, aarr, nk, h, rows, k, _vp(out), _vp(ws), ws.numel(), _stream()),
                   "ode_rhs_energy")
        assert np.array_equal(out.cpu().numpy(), ref), nk


def test_denoise_is_the_restated_step(agent, fx, forced):
    """gp_ode_denoise_energy against samplers.py:240-257 restated in float64 from gp_energy_score_eval's score at
    eps: x + (0 - g^2 grad) * step, Gram-Schmidt, + pts_center. The score path has no stand-alone denoise test; its
    final pose, which ends in this step, is held to rotation 1e-4 absolute and translation 1e-5 of max |t|
    (test_ode_pred_func_vs_golden): those bars. q carries the pose's translation and its rotation."""
    import energy_ref
    from genpose2_amd import sde
    from genpose2_amd.aggregate import quaternion_to_matrix, rot6_to_matrix
    from genpose2_amd.ode import time_scalars
    x = forced[1]
    t32, sig, _ = time_scalars(EPS)
    g2 = float(sde.diffusion(torch.full((1,), EPS, dtype=torch.float32)).to(torch.float32) ** 2)
    step = float(np.float32((1 - EPS) / ei.STEPS))
    xd = torch.from_numpy(x).to(DEV)
    ws = torch.empty(int(fx.h.lib.gp_ode_workspace_size(ROWS)), dtype=torch.uint8, device=DEV)
    pose, q = fx.h.ode_denoise(fx.pobj, t32, sig, g2, step, xd, ei.K, fx.center, ws, energy_grad=True)
    grad = _score(fx, fx.pobj, t32, sig, x.reshape(ROWS, 9).astype(np.float32), ei.K).astype(np.float64)
    mean = x.reshape(ROWS, 9) + (0.0 - g2 * grad) * step
    want = energy_ref.gs6(torch.from_numpy(mean)).numpy()
    want[:, 6:] += np.repeat(fx.g["pts_center"], ei.K, 0).astype(np.float64)
    got = pose.cpu().numpy()
    rot = np.abs(got[:, :6] - want[:, :6]).max()
    tr = np.abs(got[:, 6:] - want[:, 6:]).max() / np.abs(want[:, 6:]).max()
    print(f"denoise: rotation {rot:.2e}, translation rel {tr:.2e}")
    assert pose.dtype == torch.float64 and rot < 1e-4 and tr < 1e-5
    assert torch.equal(q[:, 4:], pose[:, 6:])
    assert float((quaternion_to_matrix(q[:, :4].cpu()) - rot6_to_matrix(pose[:, :6].cpu())).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------ 2. forced trajectory
def test_forced_trajectory_vs_reference(fx, forced):
    """The device through the float64 solve's steps. Per attempt |norm / norm64 - 1| within 2x the largest such
    value of the reference's float32 net forced the same way; the final state's per-row error against y64 within
    2x the reference float32's in median and in 90th percentile over the 30 rows (rows are independent under
    forcing; the maximum is set by single kink flips, so it is printed, not asserted). 2x is the margin the
    calibrated tests of this suite give another float32 summation order."""
    g = fx.g
    norms, y, _ = forced
    n64 = g["trace64"][:, 2]
    ours = np.abs(norms / n64 - 1)
    ref = np.abs(g["norm32_forced"] / n64 - 1)
    print(f"forced norms: ours max {ours.max():.3e} (attempt {int(ours.argmax())}) | reference fp32 max {ref.max():.3e}")
    eo = np.abs(y - g["y64"]).reshape(ROWS, 9).max(1)
    er = np.abs(g["y32_forced"] - g["y64"]).reshape(ROWS, 9).max(1)
    print(f"final state row error vs y64: ours median {np.median(eo):.3e} p90 {np.percentile(eo, 90):.3e} max "
          f"{eo.max():.3e} | reference fp32 median {np.median(er):.3e} p90 {np.percentile(er, 90):.3e} max {er.max():.3e}")
    assert np.array_equal(norms < 1, n64 < 1)
    assert ours.max() <= 2 * ref.max()
    assert np.median(eo) <= 2 * np.median(er) and np.percentile(eo, 90) <= 2 * np.percentile(er, 90)


# ------------------------------------------------------------------------------------------ 3. controllers agree
def _three_ways(agent, fx, T0, steps, init_x=None):
    """(pose, q, nfev) of rk45_device, rk45_drive and gp_ode_sample_energy, free-running from the same x0."""
    from genpose2_amd import sde
    from genpose2_amd.ode import DeviceRk45, rk45_device, rk45_drive, time_scalars
    x0 = torch.from_numpy(fx.g["prior"]).to(DEV) * sde.prior_sigma(T0)
    if init_x is not None:
        x0 = init_x.to(torch.float32) + x0
    t_eval = None if steps is None else np.linspace(T0, EPS, steps)
    t32, sig, _ = time_scalars(EPS)
    g2 = float(sde.diffusion(torch.full((1,), EPS, dtype=torch.float32)).to(torch.float32) ** 2)
    step = float(np.float32((1 - EPS) / (1000 if steps is None else steps)))
    out = []
    be = DeviceRk45(fx.h, fx.pobj, x0, ei.K, energy_grad=True)
    x, nfev, status = rk45_device(be, T0, EPS, t_eval=t_eval)
    assert status == 1
    out.append(fx.h.ode_denoise(fx.pobj, t32, sig, g2, step, x, ei.K, fx.center, be.ws, energy_grad=True) + (nfev,))
    be = DeviceRk45(fx.h, fx.pobj, x0, ei.K, energy_grad=True)
    _, nfev, status = rk45_drive(be, T0, EPS, t_eval=t_eval, keep_all=False)
    assert status == 0
    out.append(fx.h.ode_denoise(fx.pobj, t32, sig, g2, step, be.outputs()[-1], ei.K, fx.center, be.ws,
                                energy_grad=True) + (nfev,))
    pose, q, nfev, status = fx.h.ode_sample_energy(fx.pobj, x0, ei.K, fx.center, T0, EPS, steps)
    assert status == 1
    out.append((pose, q, nfev))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ["steps20", "steps_none", "init_x_t015"])
def test_controllers_agree(agent, fx, case):
    """Free-running, the fused attempts under the device controller (rk45_device), the stage launches under the host
    controller (rk45_drive) and the C entry (gp_ode_sample_energy) give the same nfev, and pose and q bit for bit.
    The arithmetic is one: the energy backend's host-controlled attempts and rk45_drive's step-size factor take
    their powers from the device (ode.DeviceRk45._device_stage_scalars / err_pow). With the host's pow in the stage
    scalars the poses were 1.3e-14 apart, with it in the factor alone 2.2e-16, at equal nfev."""
    if case == "init_x_t015":
        init = torch.from_numpy(fx.g["pred_pose32"].astype(np.float32)).to(DEV).clone()
        init[:, 6:] -= fx.center.repeat_interleave(ei.K, 0)
        runs = _three_ways(agent, fx, 0.15, ei.STEPS, init)
    else:
        runs = _three_ways(agent, fx, ei.T0, ei.STEPS if case == "steps20" else None)
    names = ("rk45_device", "rk45_drive", "gp_ode_sample_energy")
    for name, (pose, q, nfev) in zip(names, runs):
        d = float((pose - runs[0][0]).abs().max())
        print(f"{case}: {name} nfev {nfev}, max |pose - rk45_device's| {d:.3e}")
    for name, (pose, q, nfev) in zip(names[1:], runs[1:]):
        assert nfev == runs[0][2], name
        assert torch.equal(pose, runs[0][0]) and torch.equal(q, runs[0][1]), name


# ------------------------------------------------------------------------------------------ 4. end to end
def _pred(agent, fx, **kw):
    from genpose2_amd.agent import NoiseFeed
    agent.noise_feed = NoiseFeed(torch.from_numpy(fx.g["prior"]))
    try:
        return agent.pred_func(dict(fx.data), repeat_num=ei.K, T0=ei.T0, extract_feature=False, **kw)
    finally:
        agent.noise_feed = None


def test_pred_func_end_to_end(agent, fx):
    """pred_func(energy_ode=True) on the fixture: a finished solve, finite outputs, orthonormal rotation columns and
    unit quaternions; nfev within two attempts either side of the reference's own range over the six seeds; the
    pose within 2x the reference's own float32 / float64 spread over those seeds of its float64 run (the energy
    and the score agent's poses differ by 1.4 on these inputs: a wrong gradient, sign, sigma or coef cannot pass).
    nfev equality with the reference is not asked: the reference does not have it with itself."""
    g = fx.g
    pose, q = _pred(agent, fx)
    nfev = agent.last_nfev
    assert pose.dtype == torch.float64 and tuple(pose.shape) == (ei.B, ei.K, 9) and tuple(q.shape) == (ei.B, ei.K, 7)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(q).all())
    p = pose.view(ROWS, 9).cpu().numpy()
    a, b = p[:, :3], p[:, 3:6]
    assert np.abs((a * a).sum(1) - 1).max() < 1e-12 and np.abs((b * b).sum(1) - 1).max() < 1e-12
    assert np.abs((a * b).sum(1)).max() < 1e-12
    assert np.abs(np.linalg.norm(q.view(ROWS, 7)[:, :4].cpu().numpy(), axis=1) - 1).max() < 1e-12
    rot, tr = ei.row_errors(p, g["pred_pose64"])
    print(f"pred_func: nfev {nfev} (reference {int(g['nfev_lo'])} .. {int(g['nfev_hi'])}); vs pred_pose64: rotation "
          f"{rot.max():.3e} (spread {float(g['spread_rot']):.3e}), translation {tr.max():.3e} (spread "
          f"{float(g['spread_trans']):.3e})")
    assert int(g["nfev_lo"]) - 12 <= nfev <= int(g["nfev_hi"]) + 12
    assert rot.max() <= 2 * float(g["spread_rot"]) and tr.max() <= 2 * float(g["spread_trans"])


def test_pred_func_process_and_trace(agent, fx):
    """return_process gives (B, K, 20, 9) whose last slice is the un-denoised solve at eps (Gram-Schmidt, +
    pts_center) of the host controller kept alone. ode_trace fills."""
    from genpose2_amd import device as dev
    from genpose2_amd.ode import DeviceRk45, rk45_drive
    pose, proc = _pred(agent, fx, return_process=True)
    assert tuple(proc.shape) == (ei.B, ei.K, ei.STEPS, 9) and proc.dtype == torch.float64
    be = DeviceRk45(fx.h, fx.pobj, fx.x0, ei.K, energy_grad=True)
    _, nfev, _ = rk45_drive(be, ei.T0, EPS, t_eval=np.linspace(ei.T0, EPS, ei.STEPS), keep_all=False)
    last, _ = dev.pose_epilogue_f64(be.outputs()[-1].view(ROWS, 9).clone(), ei.K, fx.center)
    assert agent.last_nfev == nfev
    assert torch.equal(proc[:, :, -1].reshape(ROWS, 9), last)
    trace = []
    agent.ode_trace = trace
    try:
        pose2, _ = _pred(agent, fx)
    finally:
        agent.ode_trace = None
    assert len(trace) * 6 + 2 == agent.last_nfev and all(len(a) == 3 for a in trace)
    assert trace[0][0] == ei.T0 and torch.equal(pose2, pose)


# ------------------------------------------------------------------------------------------ 5. refusals, neighbours
def test_refusals(agent, fx):
    data = dict(fx.data)
    with pytest.raises(NotImplementedError, match="ODE.*energy_ode"):
        _make_agent(energy_ode=False).pred_func(dict(data), repeat_num=2, extract_feature=False)
    with pytest.raises(NotImplementedError, match="ode_coupling='object'"):
        _make_agent(ode_coupling="object").pred_func(dict(data), repeat_num=2, extract_feature=False)
    agent.global_batch = object()
    try:
        with pytest.raises(NotImplementedError, match="global-batch"):
            agent.pred_func(dict(data), repeat_num=2, extract_feature=False)
    finally:
        agent.global_batch = None
    with pytest.raises(NotImplementedError, match="get_likelihood"):
        agent.get_likelihood(dict(data), torch.zeros((ei.B, 2, 9), device=DEV), extract_feature=False)


def test_raw_entries_refuse_a_null_plane(agent, fx):
    """Every raw entry with a null gw plane returns a status and a message, and launches nothing: the outputs keep
    their fill."""
    from genpose2_amd import _lib
    lib = _lib.load()
    h = fx.h
    n = ROWS * 9
    good = h.grad_weights
    bad = _lib.HeadGradWeights(pe0_wt=good.pe0_wt, pe2_wt=None, h1p_wt=good.h1p_wt)
    w, gw = ctypes.byref(h.w), ctypes.byref(bad)
    y = fx.x0.to(torch.float64).reshape(-1).contiguous()
    fill = 7.25
    K = [torch.full((n,), fill, dtype=torch.float64, device=DEV) for _ in range(7)]
    y1 = torch.full((n,), fill, dtype=torch.float64, device=DEV)
    err = torch.full((1,), fill, dtype=torch.float64, device=DEV)
    pose = torch.full((ROWS, 9), fill, dtype=torch.float64, device=DEV)
    q = torch.full((ROWS, 7), fill, dtype=torch.float64, device=DEV)
    ws = torch.zeros(int(lib.gp_ode_sample_workspace_size(ROWS)), dtype=torch.uint8, device=DEV)
    t32, sig, coef = R.stage_scalars(R.stage_times(0.5, -0.01))
    s = _stream()
    nfev, status = ctypes.c_int(-5), ctypes.c_int(-5)
    calls = {
        "ode_rhs_energy": lambda g: lib.gp_ode_rhs_energy(w, g, _vp(fx.pobj), float(t32[0]), float(sig[0]), float(coef[0]),
                                                          _vp(y), None, None, 0, 0.0, ROWS, ei.K, _vp(K[1]), _vp(ws),
                                                          ws.numel(), s),
        "ode_attempt_energy": lambda g: lib.gp_ode_attempt_energy(w, g, _vp(fx.pobj), _np_p(t32), _np_p(sig), _np_p(coef),
                                                                  _vp(y), _ptrs(K), _np_p(A6), _np_p(B6), _np_p(E7), -0.01,
                                                                  RTOL, ATOL, ROWS, ei.K, _vp(y1), _vp(err), _vp(ws),
                                                                  ws.numel(), s),
        "ode_auto_attempt_energy": lambda g: lib.gp_ode_auto_attempt_energy(
            w, g, _vp(fx.pobj), 0, 3, EPS, -1.0, RTOL, ATOL, 0.01, 5000.0, 4.0, _vp(y), _vp(y1), _ptrs(K), _np_p(A6),
            _np_p(B6), _np_p(E7), ROWS, ei.K, _vp(ws), ws.numel(), None, s),
        "ode_denoise_energy": lambda g: lib.gp_ode_denoise_energy(w, g, _vp(fx.pobj), float(t32[0]), float(sig[0]), 1.0,
                                                                  0.05, _vp(y), ROWS, ei.K, _vp(fx.center), _vp(pose),
                                                                  _vp(q), _vp(ws), ws.numel(), s),
        "ode_sample_energy": lambda g: lib.gp_ode_sample_energy(w, g, _vp(fx.pobj), _vp(fx.x0), ROWS, ei.K, ei.T0, EPS,
                                                                ei.STEPS, RTOL, ATOL, _vp(fx.center), _vp(pose), _vp(q),
                                                                ctypes.byref(nfev), ctypes.byref(status), _vp(ws),
                                                                ws.numel(), s),
    }
    for name, call in calls.items():
        for g in (gw, None):
            assert call(g) != 0, name
            assert name in lib.gp_last_error().decode(), (name, lib.gp_last_error())
    torch.cuda.synchronize()
    for t in K + [y1, err, pose, q]:
        assert bool((t == fill).all())
    assert not bool(ws.any()) and nfev.value == -5 and status.value == -5


def test_score_agent_ode_is_untouched(score_before, agent, fx):
    """The score agent's pred_func ODE on golden_ode after this module's energy agents were built and ran equals the
    run made before the first of them existed, bit for bit: no state is shared between the two."""
    _pred(agent, fx)
    pose, q, nfev = _score_ode_run()
    assert nfev == score_before[2]
    assert np.array_equal(pose, score_before[0]) and np.array_equal(q, score_before[1])
