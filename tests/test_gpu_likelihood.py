"""GPU checks of the likelihood mode: the forward-mode score + divergence kernels (gp_score_div_eval,
gp_like_rhs, gp_like_attempt) and PoseNet.get_likelihood against the reference's own runs
(tests/golden/make_golden_likelihood.py)."""
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
    a = _agent(sampler_mode=["ode"])
    yield a
    a.heads.set_arith("f16x3")


@pytest.fixture(scope="module")
def eval_runs(agent):
    """gp_score_div_eval on golden_like_eval's inputs in both arithmetics: {arith: (score (4,50,9), div (4,50))}."""
    from genpose2_amd import sde
    g = golden("like_eval")
    K = g["pose"].shape[0] // g["pts_feat"].shape[0]
    x = torch.from_numpy(g["pose"]).to(DEV)
    eps = torch.from_numpy(g["eps"]).to(DEV)
    out = {}
    for arith in ("f16x3", "f32"):
        agent.heads.set_arith(arith)
        pobj = agent.heads.object_proj(torch.from_numpy(g["pts_feat"]).to(DEV))
        ss, dd = [], []
        for t in g["t"]:
            t32 = torch.tensor([t], dtype=torch.float32)
            trow = agent.heads.time_proj(t32.to(DEV))
            s, d = agent.heads.score_div(pobj, trow, float(sde.sigma(t32)[0]), x, eps, K)
            ss.append(s.cpu().numpy()), dd.append(d.cpu().numpy())
        out[arith] = (np.stack(ss), np.stack(dd))
    agent.heads.set_arith("f16x3")
    return out


@pytest.mark.parametrize("arith", ("f16x3", "f32"))
def test_score_div_eval_vs_reference(eval_runs, arith):
    """Score within the head bar (1e-5 of max |score| per time) of the reference's float32 score. Divergence:
    the error against the reference's float64 divergence, normalised by that time's max |div64|, within 2x the
    reference float32's own, in max and in mean over the rows of all four times outside the kink margin
    (the calibrated rule of the large fixtures; see make_golden_likelihood.py for the margin)."""
    import like_inputs as li
    g = golden("like_eval")
    score, div = eval_runs[arith]
    keep = g["margin"] >= li.KINK_MARGIN
    print(f"{arith}: rows excluded under the kink margin: {int((~keep).sum())} of {keep.size}")
    assert (~keep).sum() <= li.MAX_EXCLUDED * keep.size
    eo, er = [], []
    for j, t in enumerate(g["t"]):
        es = np.abs(score[j] - g["score32"][j]).max() / np.abs(g["score32"][j]).max()
        sc = np.abs(g["div64"][j]).max()
        o = np.abs(div[j].astype(np.float64) - g["div64"][j]) / sc
        r = np.abs(g["div32"][j].astype(np.float64) - g["div64"][j]) / sc
        print(f"  t={t:g}: score rel {es:.2e} | div error / max|div64|: ours max {o[keep[j]].max():.2e} mean "
              f"{o[keep[j]].mean():.2e}, reference fp32 max {r[keep[j]].max():.2e} mean {r[keep[j]].mean():.2e}")
        assert es < 1e-5, (t, es)
        eo.append(o[keep[j]]), er.append(r[keep[j]])
    eo, er = np.concatenate(eo), np.concatenate(er)
    print(f"  all times: ours max {eo.max():.3e} mean {eo.mean():.3e} | reference fp32 max {er.max():.3e} mean "
          f"{er.mean():.3e}")
    assert eo.max() <= 2 * er.max() and eo.mean() <= 2 * er.mean(), (eo.max(), er.max(), eo.mean(), er.mean())


def test_divergence_arith_vs_float64(eval_runs):
    """In the style of test_head_gemm_arith_vs_float64: on the R = 50 fixture the f16x3 trunk's divergence error
    against float64 is <= the exact-fp32 trunk's, in mean and in max (rows outside the kink margin)."""
    import like_inputs as li
    g = golden("like_eval")
    keep = g["margin"] >= li.KINK_MARGIN
    stats = {}
    for arith in ("f16x3", "f32"):
        e = np.concatenate([(np.abs(eval_runs[arith][1][j].astype(np.float64) - g["div64"][j]) /
                             np.abs(g["div64"][j]).max())[keep[j]] for j in range(len(g["t"]))])
        stats[arith] = {"max": float(e.max()), "mean": float(e.mean())}
    print("divergence error vs float64 / max|div64|:", stats)
    assert stats["f16x3"]["mean"] <= stats["f32"]["mean"] and stats["f16x3"]["max"] <= stats["f32"]["max"], stats


class _Like:
    """Raw calls of gp_like_rhs / gp_like_attempt on R rows (K per object)."""

    def __init__(self, agent, R, K, seed):
        from genpose2_amd import _lib, ode
        self.lib, self.ode, self.h = _lib.load(), ode, agent.heads
        self.R, self.K, self.n = R, K, 10 * R
        rng = np.random.default_rng(seed)
        B = (R + K - 1) // K
        feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
        self.pobj = self.h.object_proj(torch.from_numpy(feat).to(DEV))
        x = rng.normal(size=(R, 9))
        x[:, 6:] *= 0.3
        self.y = torch.from_numpy(np.concatenate([x.reshape(-1), 0.1 * rng.normal(size=R)])).to(DEV)
        self.eps = torch.from_numpy((rng.standard_normal((R, 9)) * 50.0).astype(np.float32)).to(DEV)
        self.ws = torch.empty(int(self.lib.gp_like_workspace_size(R)), dtype=torch.uint8, device=DEV)

    def _s(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rhs(self, t, kin=(), acoef=(), h=0.0, rows=None, y=None, eps=None, pobj=None):
        R = self.R if rows is None else rows
        y = self.y if y is None else y
        eps = self.eps if eps is None else eps
        pobj = self.pobj if pobj is None else pobj
        t32, sig, coef = self.ode.time_scalars(t)
        kout = torch.empty(10 * R, dtype=torch.float64, device=DEV)
        nk = len(kin)
        karr = self.ode._ptr_array(list(kin)) if nk else None
        aarr = (ctypes.c_double * nk)(*acoef) if nk else None
        ws = torch.empty(int(self.lib.gp_like_workspace_size(R)), dtype=torch.uint8, device=DEV)
        self.ode.check(self.lib.gp_like_rhs(
            ctypes.byref(self.h.w), ctypes.c_void_p(pobj.data_ptr()), t32, sig, coef, ctypes.c_void_p(y.data_ptr()),
            ctypes.c_void_p(eps.data_ptr()), karr, aarr, nk, float(h), R, self.K, ctypes.c_void_p(kout.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._s()), "like_rhs")
        torch.cuda.synchronize()
        return kout


def _attempt_vs_six_rhs(agent, arith, R, K, seed):
    """gp_like_attempt at R rows against the same step built from six gp_like_rhs calls: the same K_1..K_6 and
    y_new bits, and an error norm within 1e-12 relative of scipy's expression in float64 NumPy over the downloaded
    stages (all 10 R entries under one RMS norm)."""
    from genpose2_amd import ode
    agent.heads.set_arith(arith)
    try:
        L = _Like(agent, R, K, seed)
        t, h, rtol, atol = 0.3, 2e-3, 1e-5, 1e-5
        K0 = L.rhs(t)
        # stage by stage
        Ks = [K0]
        for s in range(1, 6):
            Ks.append(L.rhs(t + ode.C[s] * h, Ks[:s], list(ode.A[s][:s]), h))
        # a NumPy float64 time, as rk_step's t + h is (time_scalars forms g in float32 for a Python float)
        Ks.append(L.rhs(np.float64(t) + h, Ks[:6], list(ode.B), h))
        # one attempt
        Ka = [K0.clone()] + [torch.zeros(L.n, dtype=torch.float64, device=DEV) for _ in range(6)]
        stage_t = [t + c * h for c in ode.C[1:]] + [t + h]
        t32, sig, coef = ode.stage_scalars(stage_t)
        ynew = torch.zeros(L.n, dtype=torch.float64, device=DEV)
        err = torch.zeros(1, dtype=torch.float64, device=DEV)
        ode.check(L.lib.gp_like_attempt(
            ctypes.byref(L.h.w), ctypes.c_void_p(L.pobj.data_ptr()), t32.ctypes.data_as(ctypes.c_void_p),
            sig.ctypes.data_as(ctypes.c_void_p), coef.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(L.y.data_ptr()),
            ctypes.c_void_p(L.eps.data_ptr()), ode._ptr_array(Ka), ode._A6.ctypes.data_as(ctypes.c_void_p),
            ode._B6.ctypes.data_as(ctypes.c_void_p), ode._E7.ctypes.data_as(ctypes.c_void_p), float(h), rtol, atol,
            L.R, L.K, ctypes.c_void_p(ynew.data_ptr()), ctypes.c_void_p(err.data_ptr()),
            ctypes.c_void_p(L.ws.data_ptr()), L.ws.numel(), L._s()), "like_attempt")
        torch.cuda.synchronize()
        for s in range(1, 7):
            assert torch.equal(Ks[s], Ka[s]), s
        Kn = np.stack([k.cpu().numpy() for k in Ka])
        y = L.y.cpu().numpy()
        # rk_step: y_new = y + h * (K[:-1].T @ B) up to the summation order of the dot product
        want = y + h * np.dot(Kn[:-1].T, ode.B)
        np.testing.assert_allclose(ynew.cpu().numpy(), want, rtol=1e-12, atol=1e-13)
        assert np.all(Kn[:, 9 * L.R:] != 0.0)                     # the logp entries are written by every stage
        yn = ynew.cpu().numpy()
        scale = atol + np.maximum(np.abs(y), np.abs(yn)) * rtol
        e = np.dot(Kn.T, ode.E) * h / scale
        norm = np.linalg.norm(e) / e.size ** 0.5
        got = float(err.cpu()[0])
        print(f"{arith}: error norm {got:.17g} vs NumPy {norm:.17g}")
        assert e.size == 10 * L.R and abs(got - norm) <= 1e-12 * norm
    finally:
        agent.heads.set_arith("f16x3")


@pytest.mark.parametrize("arith", ("f16x3", "f32"))
def test_like_attempt_equals_six_rhs_calls(agent, arith):
    """_attempt_vs_six_rhs at R = 10."""
    _attempt_vs_six_rhs(agent, arith, 10, 5, 17)


def test_like_attempt_equals_six_rhs_calls_two_primal_tiles(agent):
    """_attempt_vs_six_rhs at R = 4,097, the smallest row count at which the f16x3 likelihood stages take two
    primal tiles per workgroup (the attempt's last stage with y_new and the error partials included; its last
    workgroup holds one row)."""
    _attempt_vs_six_rhs(agent, "f16x3", 4097, 1, 29)


def test_like_rhs_tilings_agree_bitwise(agent):
    """gp_like_rhs takes two primal tiles per workgroup from 4,097 rows (f16x3 trunk). Rows evaluated at that
    smallest row count of the wide tiling equal the same rows evaluated 16 at a time in the single-tile path,
    bit for bit: the first, a middle and the last (1-row) tile are compared."""
    agent.heads.set_arith("f16x3")
    R, K = 4097, 1
    L = _Like(agent, R, K, 23)
    t = 0.4
    wide = L.rhs(t)
    for r0 in (0, 2064, 4096):
        n = min(16, R - r0)
        y = torch.cat([L.y[9 * r0: 9 * (r0 + n)], L.y[9 * R + r0: 9 * R + r0 + n]]).contiguous()
        small = L.rhs(t, rows=n, y=y, eps=L.eps[r0:r0 + n].contiguous(), pobj=L.pobj[r0:r0 + n].contiguous())
        assert torch.equal(small[:9 * n], wide[9 * r0: 9 * (r0 + n)]), r0
        assert torch.equal(small[9 * n:], wide[9 * R + r0: 9 * R + r0 + n]), r0


def test_get_likelihood_vs_reference(agent):
    """PoseNet.get_likelihood on golden_like_ode (B = 2 x K = 5, eps injected through noise_feed) against the
    reference's float64 run: within 2x the spread of the reference's own float32 runs (as is, and with pts_feat
    scaled by 1 + 2e-7 / 1 - 3e-7) about it, in max and in mean. The solve is chaotic at solver-tolerance scale
    (~2,100 attempts), so nfev is printed, not asserted."""
    from genpose2_amd.agent import NoiseFeed
    g = golden("like_ode")
    agent.heads.set_arith("f16x3")
    B, K = g["pose_samples"].shape[:2]
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    agent.noise_feed = NoiseFeed(torch.from_numpy(g["eps_unit"]))
    try:
        ll, z = agent.get_likelihood(data, torch.from_numpy(g["pose_samples"]).to(DEV), return_latent=True)
    finally:
        agent.noise_feed = None
    assert ll.dtype == torch.float64 and tuple(ll.shape) == (B, K)
    assert z.dtype == torch.float64 and tuple(z.shape) == (B, K, 9)
    ll64 = g["ll64"]
    refs = [np.abs(g[k] - ll64) for k in ("ll32", "ll32_p1", "ll32_p2")]
    spread = {"max": max(float(e.max()) for e in refs), "mean": max(float(e.mean()) for e in refs)}
    e = np.abs(ll.cpu().numpy() - ll64)
    ours = {"max": float(e.max()), "mean": float(e.mean())}
    print(f"get_likelihood vs ll64: ours {ours}, reference fp32 spread {spread}; nfev {agent.last_nfev} "
          f"(reference fp32 {int(g['nfev32'])}, float64 {int(g['nfev64'])}); |ll64| in "
          f"[{np.abs(ll64).min():.1f}, {np.abs(ll64).max():.1f}]")
    assert ours["max"] <= 2 * spread["max"] and ours["mean"] <= 2 * spread["mean"], (ours, spread)
    # the latent is y[:9R] of the solve's last state: the same solve driven here gives it bit for bit, and its
    # logp entries give ll back through the final formula (samplers.py:100-109)
    from genpose2_amd import arch, ode, sde
    R = B * K
    pose = torch.from_numpy(g["pose_samples"]).to(DEV).reshape(R, -1).clone()
    pose[:, -3:] -= data["pts_center"].unsqueeze(1).repeat(1, K, 1).view(R, -1)
    eps = torch.from_numpy(g["eps_unit"]).to(DEV) * sde.prior_sigma(arch.SDE_T)
    be = ode.LikelihoodRk45(agent.heads, agent.heads.object_proj(data["pts_feat"]), pose, eps, K)
    _, nfev, status = ode.rk45_drive(be, arch.SAMPLING_EPS, 1.0, keep_all=False)
    assert status == 0 and nfev == agent.last_nfev
    y = be.ys[-1]
    assert torch.equal(z.reshape(-1), y[:9 * R])
    sig = float(np.float32(arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** 1.0))
    zz, dl = y[:9 * R].cpu().numpy().reshape(R, 9), y[9 * R:].cpu().numpy()
    want = (-4.5 * np.log(2 * np.pi * sig ** 2) - (zz ** 2).sum(-1) / (2 * sig ** 2) + dl) / np.log(2)
    np.testing.assert_allclose(ll.cpu().numpy().reshape(-1), want, rtol=1e-6)
