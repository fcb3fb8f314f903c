"""GPU checks of per-object PC sampling (cfg.pc_coupling = "object", gp_pc_sample_object): the corrector's step size
from each object's own candidates. Against the reference called once per object (golden_pc_object), and the
contract itself: an object's rows are bit-identical whatever else the call holds and however a batch is split into
calls. Tolerances where bits may differ are the small-golden PC ones of test_oracle_golden.py: rotation <= 1e-4
absolute, translation <= 1e-5 of max |t|."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _agent(**kw):
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    return PoseNet(GenPoseConfig(device=DEV, **kw)).eval()


@pytest.fixture(scope="module")
def agent():
    return _agent(pc_coupling="object", sampler_mode=["pc"], sampling_steps=6)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _within(got, want, what):
    """The PC tolerances on [rot6 | t] rows (or [quat | t] rows with nq = 4)."""
    got, want = _np(got) if isinstance(got, torch.Tensor) else got, _np(want) if isinstance(want, torch.Tensor) else want
    nr = got.shape[-1] - 3
    rot = np.abs(got[..., :nr] - want[..., :nr]).max()
    tr = np.abs(got[..., nr:] - want[..., nr:]).max() / np.abs(want[..., nr:]).max()
    print(f"  {what}: rotation abs {rot:.2e}, translation rel {tr:.2e}")
    assert rot <= 1e-4 and tr <= 1e-5, (what, rot, tr)


@pytest.mark.parametrize("arith", ["f16x3", "f32"])
def test_pred_func_vs_reference_per_object(arith):
    """PoseNet.pred_func with pc_coupling='object' on golden_pc_object (features, prior and z1 / z2 injected; 30
    rows: objects straddle the 16-row tiles, the last tile is partial) against the reference's per-object calls."""
    import pc_object_inputs as pi
    from genpose2_amd.agent import NoiseFeed
    g = golden("pc_object")
    B, K, T = pi.B, pi.K, pi.T
    a = _agent(pc_coupling="object", sampler_mode=["pc"], sampling_steps=T)
    a.heads.set_arith(arith)
    data = {"pts": torch.zeros((B, 1, 3), device=DEV), "pts_feat": torch.from_numpy(g["pts_feat"]).to(DEV),
            "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    a.noise_feed = NoiseFeed(torch.from_numpy(g["prior"]), torch.from_numpy(g["z1"]), torch.from_numpy(g["z2"]))
    pose, q = a.pred_func(dict(data), repeat_num=K, extract_feature=False)
    pose2, proc = a.pred_func(dict(data), repeat_num=K, extract_feature=False, return_process=True)
    assert pose.dtype == torch.float32 and tuple(pose.shape) == (B, K, 9) and tuple(q.shape) == (B, K, 7)
    assert tuple(proc.shape) == (B, K, T, 9) and torch.equal(pose, pose2)
    _within(pose.view(B * K, 9), g["pred_pose32"].astype(np.float64), "pred_pose")
    _within(q.view(B * K, 7), g["pred_q32"].astype(np.float64), "pred_q")
    _within(proc.view(B * K, T, 9), g["xs32"].astype(np.float64), "xs")
    # and the fixture does tell the semantics apart for this result too: the whole-batch reference is far away
    assert np.abs(_np(pose.view(B * K, 9)) - g["pred_pose32_batch"]).max() > 1e-2


class _Raw:
    """Raw gp_pc_sample_object runs on B objects x K candidates, T steps, through HeadModel.pc_sample."""

    def __init__(self, heads, B, K, T=6, seed=907, center=True):
        from genpose2_amd import arch, sde
        self.h, self.B, self.K, self.T = heads, B, K, T
        R = self.R = B * K
        rng = np.random.default_rng(seed)
        feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
        feat *= np.linspace(0.5, 2.0, B, dtype=np.float32)[:, None]      # objects with different score norms
        self.pobj = heads.object_proj(torch.from_numpy(feat).to(DEV))
        self.x0 = torch.from_numpy(rng.standard_normal((R, 9)).astype(np.float32)).to(DEV) * sde.prior_sigma(arch.SDE_T)
        self.z1 = torch.from_numpy(rng.standard_normal((T, R, 9)).astype(np.float32)).to(DEV)
        self.z2 = torch.from_numpy(rng.standard_normal((T, R, 9)).astype(np.float32)).to(DEV)
        c = 0.1 * rng.standard_normal((B, 3)) if center else np.zeros((B, 3))
        self.center = torch.from_numpy(c.astype(np.float32)).to(DEV)
        self.tab = sde.pc_step_table(T)
        self.tproj = heads.time_proj(torch.from_numpy(self.tab[:, 0]).to(DEV))

    def run(self, lo=0, hi=None, inject=True, rows_total=None, seed=0, coupling="object", pobj=None, x0=None):
        """Objects [lo, hi) as one call, as rows [lo*K, hi*K) of a batch of rows_total rows (default: all B objects')
        -> (res, q, xs, x)."""
        hi = self.B if hi is None else hi
        K, rows = self.K, slice(lo * self.K, hi * self.K)
        pobj = self.pobj if pobj is None else pobj
        x = (self.x0 if x0 is None else x0)[rows].clone()
        z1 = self.z1[:, rows].contiguous() if inject else None
        z2 = self.z2[:, rows].contiguous() if inject else None
        kw = {}
        if coupling == "object":
            kw = dict(coupling="object", rows_total=self.R if rows_total is None else rows_total, row_off=lo * K)
        res, q, xs = self.h.pc_sample(pobj[lo:hi].contiguous(), self.tproj, self.tab, x, K, self.center[lo:hi].contiguous(),
                                      z1, z2, seed=seed, want_xs=True, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xs).all())
        return res, q, xs, x


def _same(a, b, rows=None, what=""):
    for u, v, name in zip(a, b, ("res", "q", "xs", "x")):
        assert torch.equal(u if rows is None else u[rows], v), (what, name)


@pytest.fixture(scope="module")
def raw5(agent):
    return _Raw(agent.heads, 5, 10)


def test_composition_invariance_exact(raw5):
    """B = 5 x K = 10 (objects straddle the 16-row tiles), injected noise: the batch of 5 against each object alone
    (its own z rows, its row_off, rows_total = 50), bit for bit; then object 3 replaced by another object, and
    objects 0, 1, 2, 4 keep their bits."""
    r, K = raw5, raw5.K
    full = r.run()
    for b in range(r.B):
        _same(full, r.run(b, b + 1), slice(b * K, (b + 1) * K), f"object {b} alone")
    pobj, x0 = r.pobj.clone(), r.x0.clone()
    pobj[3] = 0.25 * r.pobj[0] + 1.5 * r.pobj[4]
    x0[3 * K:4 * K] = -2.0 * r.x0[0:K]
    other = r.run(pobj=pobj, x0=x0)
    for b in (0, 1, 2, 4):
        rows = slice(b * K, (b + 1) * K)
        _same(full, tuple(t[rows] for t in other), rows, f"object {b} beside another object 3")
    assert not torch.equal(full[0][3 * K:4 * K], other[0][3 * K:4 * K])
    # the batch coupling does not have the property: the same replacement moves the other objects
    b0 = r.run(coupling="batch")
    b1 = r.run(coupling="batch", pobj=pobj, x0=x0)
    assert not torch.equal(b0[0][:K], b1[0][:K])


def test_split_invariance_philox_exact(raw5, agent):
    """The same 5 objects with device draws: one call against two calls on objects [0,2) and [2,5) with matching
    row_off / rows_total and the same seed, bit for bit -- raw, and through PoseNet.object_window."""
    r, K = raw5, raw5.K
    seed = 20261
    one = r.run(inject=False, seed=seed)
    _same(one, r.run(0, 2, inject=False, seed=seed), slice(0, 2 * K), "objects [0,2)")
    _same(one, r.run(2, 5, inject=False, seed=seed), slice(2 * K, 5 * K), "objects [2,5)")
    assert not torch.equal(one[0], r.run(inject=False, seed=seed + 1)[0])
    assert not torch.equal(one[0], r.run()[0])                    # and the draws are not the injected ones

    rng = np.random.default_rng(11)
    feat = torch.from_numpy(np.maximum(rng.normal(size=(5, 1024)), 0).astype(np.float32)).to(DEV)
    center = torch.from_numpy((0.1 * rng.standard_normal((5, 3))).astype(np.float32)).to(DEV)

    def call(lo, hi, window):
        # every call restarts the agent's noise state, as ranks of a sharded run hold the same state
        agent._calls = 0
        agent._gen.manual_seed(agent.cfg.noise_seed)
        agent.object_window = window
        try:
            data = {"pts": torch.zeros((hi - lo, 1, 3), device=DEV), "pts_feat": feat[lo:hi].contiguous(),
                    "pts_center": center[lo:hi].contiguous()}
            return agent.pred_func(data, repeat_num=K, extract_feature=False)
        finally:
            agent.object_window = None

    pose, q = call(0, 5, None)
    for lo, hi in ((0, 2), (2, 5)):
        p, qq = call(lo, hi, (5, lo))
        assert torch.equal(p, pose[lo:hi]) and torch.equal(qq, q[lo:hi]), (lo, hi)
    assert torch.equal(call(0, 5, (5, 0))[0], pose)


def _teacher_forced(r):
    """Every step of an object-coupled run against the update of samplers.py:143-169 recomputed in torch float32 per
    object (energy_ref.pc_step on that object's rows: grad_norm over them alone) from gp_score_eval on the state
    that entered the step: within 1e-5 of max |x|, the bar of test_gpu_energy_score's per-step check (pts_center
    = 0, so xs is the state)."""
    import energy_ref
    K = r.K
    res, q, xs, x = r.run()
    for i in range(r.T):
        enter = r.x0 if i == 0 else xs[:, i - 1].contiguous()
        s = r.h.score(r.pobj, r.tproj[i].contiguous(), float(r.tab[i, 1]), enter, K)
        nx, mean = [], []
        for b in range(r.B):
            rows = slice(b * K, (b + 1) * K)
            n, m = energy_ref.pc_step(enter[rows].cpu(), s[rows].cpu(), r.z1[i, rows].cpu(), r.z2[i, rows].cpu(),
                                      torch.tensor(r.tab[i, 2]), torch.tensor(r.tab[i, 3]), torch.tensor(r.tab[i, 4]))
            nx.append(n), mean.append(m)
        nx, mean = torch.cat(nx), torch.cat(mean)
        got = xs[:, i].cpu()
        err = float((got - nx).abs().max() / got.abs().max())
        print(f"step {i}: |xs - recomputed update| / max|x| = {err:.2e}")
        assert err <= 1e-5, (i, err)
    want = energy_ref.gs6(mean)
    assert float((res.cpu() - want).abs().max() / want.abs().max()) <= 1e-5
    assert torch.equal(x, xs[:, -1])
    return res, q, xs, x


def test_object_wider_than_a_tile(agent):
    """B = 2 x K = 50: each object spans four 16-row tiles, so its mean gathers row norms that other workgroups
    wrote. Each object alone has the same bits, and every step is the per-object update."""
    r = _Raw(agent.heads, 2, 50, center=False)
    full = _teacher_forced(r)
    for b in range(2):
        _same(full, r.run(b, b + 1), slice(b * 50, (b + 1) * 50), f"object {b} alone")


def test_one_candidate_per_object(agent):
    """K = 1, B = 3: the mean is over one row."""
    _teacher_forced(_Raw(agent.heads, 3, 1, center=False))


@pytest.mark.parametrize("rows_total,tile", [(6000, 32), (12800, 64)])
def test_wide_tile_classes_on_a_tiny_grid(agent, rows_total, tile):
    """B = 2 x K = 50 as a slice of a batch of rows_total rows: the 32- / 64-candidate kernels with two workgroups.
    Bit-identical to object-alone calls under the same rows_total; within the PC tolerances of the 16-candidate
    result (the f16x3 arithmetic differs by tile class)."""
    lib = agent.heads.lib
    assert lib.gp_pc_tile_rows(rows_total, 1) == tile and lib.gp_pc_tile_rows(100, 1) == 16
    r = _Raw(agent.heads, 2, 50)
    wide = r.run(rows_total=rows_total)
    for b in range(2):
        _same(wide, r.run(b, b + 1, rows_total=rows_total), slice(b * 50, (b + 1) * 50), f"object {b} alone")
    narrow = r.run()
    _within(wide[0], narrow[0], "res"), _within(wide[1], narrow[1], "q"), _within(wide[2], narrow[2], "xs")


def test_single_object_matches_batch_coupling(agent):
    """B = 1: both couplings average over the same rows; only the order of the sum differs."""
    r = _Raw(agent.heads, 1, 10)
    o, b = r.run(), r.run(coupling="batch")
    _within(o[0], b[0], "res"), _within(o[1], b[1], "q"), _within(o[2], b[2], "xs")


def test_refusals(agent, raw5):
    data = {"pts": torch.zeros((1, 1, 3), device=DEV), "pts_feat": torch.zeros((1, 1024), device=DEV),
            "pts_center": torch.zeros((1, 3), device=DEV)}
    with pytest.raises(NotImplementedError, match="pc_coupling='object'"):
        _agent(pc_coupling="object", sampler_mode=["ode"]).pred_func(dict(data), repeat_num=2, extract_feature=False)
    with pytest.raises(NotImplementedError, match="pc_coupling='object'"):
        _agent(pc_coupling="object", agent_type="energy", sampling_steps=2).pred_func(dict(data), repeat_num=2,
                                                                                      extract_feature=False)
    with pytest.raises(NotImplementedError, match="pc_coupling='object'"):
        agent.pred_func(dict(data), repeat_num=2, extract_feature=False, return_average_res=True)
    agent.global_batch = object()
    try:
        with pytest.raises(NotImplementedError, match="pc_coupling='object'"):
            agent.pred_func(dict(data), repeat_num=2, extract_feature=False)
    finally:
        agent.global_batch = None
    r = raw5
    with pytest.raises(NotImplementedError):
        r.h.pc_sample(r.pobj, r.tproj, r.tab, r.x0.clone(), r.K, r.center, coupling="object", energy_grad=True)
    with pytest.raises(NotImplementedError):
        r.h.pc_sample(r.pobj, r.tproj, r.tab, r.x0.clone(), r.K, r.center, coupling="object", global_batch=object())

    # the raw entry: a status and a message, and nothing launched (the outputs keep their fill)
    from genpose2_amd import _lib
    lib, h = r.h.lib, r.h
    ws = torch.empty(int(lib.gp_pc_object_workspace_size(r.R)), dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(r.tab, np.float32)
    x = r.x0.clone()
    res = torch.full((r.R, 9), float("nan"), device=DEV)
    q = torch.full((r.R, 7), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(rows, k, rows_total, row_off):
        return lib.gp_pc_sample_object(ctypes.byref(h.w), p(r.pobj), p(r.tproj), tab.ctypes.data_as(ctypes.c_void_p), r.T,
                                       p(x), rows, k, p(r.center), p(r.z1), p(r.z2), ctypes.c_uint64(0),
                                       ctypes.c_float(0.16), p(res), p(q), None, rows_total, row_off, p(ws), ws.numel(),
                                       h._s())

    for args, word in (((r.R - 1, r.K, r.R, 0), "whole objects"), ((r.R - r.K, r.K, r.R, 5), "row_off"),
                       ((r.R, r.K, r.R - r.K, 0), "rows_total")):
        assert raw(*args) != 0, args
        assert word in lib.gp_last_error().decode(), (args, lib.gp_last_error())
        with pytest.raises(_lib.GenPoseHipError, match=word):
            _lib.check(raw(*args), "pc_sample_object")
    torch.cuda.synchronize()
    assert bool(torch.isnan(res).all()) and bool(torch.isnan(q).all()) and torch.equal(x, r.x0)
    assert raw(r.R, r.K, r.R, 0) == 0                                # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res).all())
