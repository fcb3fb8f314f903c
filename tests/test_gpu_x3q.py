"""The hybrid form of the PC step's two per-candidate GEMMs (gp_head.h X3Q: hi*hi, hi*mid, mid*hi on f16 MFMA,
the three products of plane order 2 on block-scaled FP8 MFMA with OCP e4m3 planes) on a real MI355X.

* Error: one score evaluation of the 12,800 golden states (steps 1 and 400) through the hybrid trunk and in
  exact fp32, against the same network in float64: the hybrid's mean and 99.9th percentile <= exact fp32's,
  max < 1e-5 (the statistic of test_gpu_large.test_head_gemm_arith_vs_float64_r12800).
* Rows and wrapping: the hybrid PC step on ragged row counts of every tile width against the six-product form.
* Determinism, and edge columns / weights without a lo plane.

The bound of the comparisons against the six-product form is never taken from the hybrid itself: it is twice
the difference the exact-fp32 arithmetic shows against the six-product form on the same inputs.
"""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float32).eps)


def _heads(sd=None):
    from genpose2_amd import device, weights
    return device.HeadModel(weights.synthetic_state_dict("score") if sd is None else sd, torch.device(DEV))


def _stats(s, ref):
    e = np.abs(s.astype(np.float64) - ref) / np.abs(ref).max(1, keepdims=True)
    return {"max": float(e.max()), "p999": float(np.percentile(e, 99.9)), "mean": float(e.mean())}


def test_hybrid_score_error_vs_float64_r12800():
    """Measured on MI355X (per-row relative score error against float64; mean / p99.9 / max;
    profiles/r7/x3q_gpu_error.txt): step 1 hybrid 2.3255e-7 / 1.795e-6 / 3.13e-6, six products 2.3253e-7 /
    1.813e-6 / 3.04e-6, exact fp32 2.834e-7 / 1.907e-6 / 3.04e-6; step 400 hybrid 1.0844e-7 / 5.35e-7 / 8.50e-7,
    six products 1.0857e-7 / 5.36e-7 / 8.50e-7, exact fp32 1.793e-7 / 8.94e-7 / 1.48e-6."""
    import large_noise
    from genpose2_amd import weights
    from test_gpu_large import _agent, _score64
    g = golden("large_steps_r12800")
    src = str(g["src"])
    _, _, B, K, T, _, _ = large_noise.CASES[src]
    pts, _, _, _, _ = large_noise.inputs(src)
    agent = _agent(sampling_steps=T)
    agent.encoder.set_arith("f32")
    feat = agent.encoder.forward(torch.from_numpy(pts).to(DEV))
    heads = agent.heads
    pobj = heads.object_proj(feat)
    tab, tproj = agent._pc_table(T)
    feat_rows = np.repeat(feat.cpu().numpy().astype(np.float64), K, 0)
    sd = weights.synthetic_state_dict("score")
    for j in (int(s) for s in g["steps"]):
        x = torch.from_numpy(g[f"x_{j}"]).to(DEV).contiguous()
        ref = _score64(sd, feat_rows, g[f"x_{j}"], tab[j, 0])
        out = {}
        for name in ("hybrid", "f16x3", "f32"):
            heads.set_pc_small("fp8" if name == "hybrid" else "f16")
            heads.set_arith("f32" if name == "f32" else "f16x3")
            out[name] = heads.score(pobj, tproj[j], float(tab[j, 1]), x, K).cpu().numpy()
        stats = {k: _stats(v, ref) for k, v in out.items()}
        d = np.abs(out["hybrid"].astype(np.float64) - out["f16x3"]) / np.abs(ref).max(1, keepdims=True)
        print(f"step {j} score vs float64 (per-row relative): hybrid {stats['hybrid']}  f16x3 {stats['f16x3']}  "
              f"exact fp32 {stats['f32']}; hybrid vs f16x3 mean {d.mean():.3e} max {d.max():.3e}")
        assert not np.array_equal(out["hybrid"], out["f16x3"])      # the hybrid trunk did run
        assert stats["hybrid"]["max"] < 1e-5, (j, stats)
        assert stats["hybrid"]["mean"] <= stats["f32"]["mean"] and stats["hybrid"]["p999"] <= stats["f32"]["p999"], stats
    heads.set_pc_small("auto")
    heads.set_arith("f16x3")


def _pc_inputs(R, K, T, seed):
    from genpose2_amd import sde
    rng = np.random.default_rng(seed)
    B = R // K
    assert B * K == R
    feat = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32)).to(DEV)
    x0 = torch.from_numpy(rng.standard_normal((R, 9)).astype(np.float32)).to(DEV)
    z = torch.from_numpy(rng.standard_normal((2, T, R, 9)).astype(np.float32)).to(DEV)
    center = torch.zeros((B, 3), device=DEV)
    return feat, x0, z[0].contiguous(), z[1].contiguous(), center, sde.pc_step_table(T)


def _pc_run(heads, form, arith, feat, x0, z1, z2, center, tab, K, seed=None):
    heads.set_pc_small(form)
    heads.set_arith(arith)
    pobj = heads.object_proj(feat)
    tproj = heads.time_proj(torch.from_numpy(tab[:, 0]).to(DEV))
    kw = dict(seed=seed) if seed is not None else dict(z1=z1, z2=z2)
    res, q, xs = heads.pc_sample(pobj, tproj, tab, x0.clone(), K, center, want_xs=True, **kw)
    return res.cpu().numpy(), xs.cpu().numpy()


@pytest.mark.parametrize("R", [50, 4150, 8250])
def test_hybrid_pc_rows_vs_six_product(R):
    """R = 50 (one ragged 16-row tile path), 4,150 (32-wide tiles, ragged), 8,250 (64-wide, ragged), T = 3, injected
    noise: every state of the hybrid run within twice the largest difference the exact-fp32 arithmetic shows
    against the six-product form on the same inputs.
    Measured on MI355X (largest |pose difference| against the six-product form per step, in fp32 epsilons; the
    poses reach |x| ~ 50 at sigma(1) = 50; profiles/r7/x3q_gpu_error.txt): R=50 exact fp32 768, 896, 896, hybrid 256,
    256, 256; R=4,150 exact fp32 1024, 1280, 1280, hybrid 512, 512, 512; R=8,250 exact fp32 1024, 1292, 1280, hybrid
    512, 512, 512. The bound is 2 x the exact-fp32 figure of the same step, computed in the test.
    The default form ("auto") must equal the hybrid run at R=8,250 and the six-product run below it, bit for bit."""
    K, T = 50, 3
    heads = _heads()
    inp = _pc_inputs(R, K, T, 700 + R)
    six, six_xs = _pc_run(heads, "f16", "f16x3", *inp, K)
    f32, f32_xs = _pc_run(heads, "f16", "f32", *inp, K)
    hyb, hyb_xs = _pc_run(heads, "fp8", "f16x3", *inp, K)
    assert np.isfinite(hyb).all() and np.isfinite(hyb_xs).all()
    ref_d = np.abs(f32_xs.astype(np.float64) - six_xs).max((0, 2))      # per step
    hyb_d = np.abs(hyb_xs.astype(np.float64) - six_xs).max((0, 2))
    print(f"R={R}: per-step max |pose difference| / eps vs the six-product form: exact fp32 {ref_d / EPS}, "
          f"hybrid {hyb_d / EPS}")
    assert (ref_d > 0).all()
    assert (hyb_d <= 2 * ref_d).all(), (hyb_d / EPS, ref_d / EPS)
    assert np.abs(hyb.astype(np.float64) - six).max() <= 2 * np.abs(f32.astype(np.float64) - six).max()
    # the default ("auto") takes the hybrid form on 64-candidate tiles only
    auto, auto_xs = _pc_run(heads, "auto", "f16x3", *inp, K)
    want, want_xs = (hyb, hyb_xs) if R >= 8193 else (six, six_xs)
    assert np.array_equal(auto, want) and np.array_equal(auto_xs, want_xs)
    assert not np.array_equal(hyb_xs, six_xs)
    heads.set_pc_small("auto")


def test_hybrid_pc_deterministic():
    K, T, R = 50, 3, 4150
    heads = _heads()
    inp = _pc_inputs(R, K, T, 31)
    a, a_xs = _pc_run(heads, "fp8", "f16x3", *inp, K, seed=9)
    b, b_xs = _pc_run(heads, "fp8", "f16x3", *inp, K, seed=9)
    assert np.array_equal(a, b) and np.array_equal(a_xs, b_xs)
    c, c_xs = _pc_run(heads, "fp8", "f16x3", *inp, K)
    d, d_xs = _pc_run(heads, "fp8", "f16x3", *inp, K)
    assert np.array_equal(c, d) and np.array_equal(c_xs, d_xs)


@pytest.mark.parametrize("weights_case", ["synthetic", "no_lo_plane"])
def test_hybrid_edge_columns(weights_case):
    """A pose of zeros, a pose with one entry at the largest magnitude of the golden states, and (no_lo_plane) weights
    that hi + mid hold exactly: finite scores, each within twice the largest difference exact fp32 shows against the
    six-product form over the batch (64 golden rows and the edge rows), relative to the row's largest |score|.
    Measured on MI355X: synthetic weights exact fp32 1.142e-6, hybrid 2.538e-7 (edge rows 1.666e-7); no lo plane
    exact fp32 1.014e-6, hybrid 3.173e-7 (edge rows 2.809e-7)."""
    from genpose2_amd import pack, weights
    sd = weights.synthetic_state_dict("score")
    if weights_case == "no_lo_plane":
        sd = dict(sd)
        names = ["pose_score_net.pose_encoder.2.weight"]
        p = weights.head_params(sd)
        e2 = pack.split_exponent(p["pe2_w"])
        eh = pack.split_exponent(p["h1_pose"].reshape(-1, p["h1_pose"].shape[-1]))

        def two_planes(w, e):
            r = (np.asarray(w, np.float32) * np.float32(2.0 ** e)).astype(np.float32)
            hi = r.astype(np.float16).astype(np.float32)
            mid = (r - hi).astype(np.float16).astype(np.float32)
            return ((hi + mid) * np.float32(2.0 ** -e)).astype(np.float32)
        sd[names[0]] = two_planes(sd[names[0]], e2)
        from genpose2_amd import arch
        for h in arch.HEAD_NAMES:
            k = f"pose_score_net.{h}.0.weight"
            w = np.array(sd[k], np.float32, copy=True)
            w[:, 1024 + 128:] = two_planes(w[:, 1024 + 128:], eh)
            sd[k] = w
        packed = pack.pack_heads(sd)
        for key in ("pe2_h", "h1p_h"):
            lo = packed[key].view(np.float16).reshape(-1, 3, 64 * 8)[:, 2]
            assert lo.size and not lo.any(), key
    heads = _heads(sd)
    g = golden("large_steps_r12800")
    xg = g["x_400"][:64]
    big = float(np.abs(np.concatenate([g["x_1"], g["x_400"]])).max())
    edge = np.zeros((16, 9), np.float32)
    for o in range(9):
        edge[1 + o, o] = big if o % 2 == 0 else -big
    x = torch.from_numpy(np.concatenate([xg, edge]).astype(np.float32)).to(DEV)
    R = x.shape[0]
    rng = np.random.default_rng(3)
    feat = torch.from_numpy(rng.standard_normal((1, 1024)).astype(np.float32)).to(DEV)
    out = {}
    for name in ("hybrid", "f16x3", "f32"):
        heads.set_pc_small("fp8" if name == "hybrid" else "f16")
        heads.set_arith("f32" if name == "f32" else "f16x3")
        pobj = heads.object_proj(feat)
        tproj = heads.time_proj(torch.tensor([0.3], device=DEV))
        out[name] = heads.score(pobj, tproj[0], 1.0, x, R).cpu().numpy().astype(np.float64)
    scale = np.abs(out["f16x3"]).max(1, keepdims=True)
    ref_d = (np.abs(out["f32"] - out["f16x3"]) / scale).max()
    hyb_d = np.abs(out["hybrid"] - out["f16x3"]) / scale
    print(f"{weights_case}: max relative difference vs the six-product form: exact fp32 {ref_d:.3e}, hybrid "
          f"{hyb_d.max():.3e} (edge rows {hyb_d[64:].max():.3e})")
    assert np.isfinite(out["hybrid"]).all()
    assert ref_d > 0 and hyb_d.max() <= 2 * ref_d, (hyb_d.max(), ref_d)
