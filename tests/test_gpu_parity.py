"""HIP path vs oracle / golden vectors on a real MI355X (all calls go through libgenpose_hip.so).

Tolerances (written here, per north_star): indices bit-exact; fp32 features/scores within
1e-5 of max |ref|; PC/ODE rotation components within 1e-4 absolute; translations within 1e-5
relative to max |t| (1e-4 for the ODE T0=1 case, whose adaptive step controller may take a
different accept/reject path, see tests/test_oracle_golden.py).
"""
import os

import numpy as np
import pytest
import torch

from conftest import ARITHS, ARITHS3, golden, set_arith
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def score_agent():
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    return PoseNet(GenPoseConfig(device=DEV, sampling_steps=20)).eval()


# ---------------------------------------------------------------- operator level
@pytest.mark.parametrize("n,m,grid", [(1024, 512, False), (2048, 512, False), (300, 64, True),
                                      (1024, 256, True), (37, 37, True), (4096, 128, False)])
def test_fps_op_bit_exact(n, m, grid):
    from genpose2_amd import pointnet2_utils as pu
    from oracle import oracle
    rng = np.random.default_rng(n + m)
    xyz = (rng.integers(0, 5, size=(3, n, 3)) if grid else rng.normal(size=(3, n, 3))).astype(np.float32)
    got = pu.furthest_point_sample(torch.from_numpy(xyz).to(DEV), m).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.furthest_point_sample(xyz, m))


@pytest.mark.parametrize("radius,ns,n,m", [(0.2, 16, 1024, 128), (0.5, 32, 500, 33), (0.05, 16, 1024, 64),
                                           (10.0, 8, 100, 7)])
def test_ball_query_group_gather_ops(radius, ns, n, m):
    from genpose2_amd import pointnet2_utils as pu
    from oracle import oracle
    rng = np.random.default_rng(ns + n)
    xyz = rng.uniform(-0.5, 0.5, size=(2, n, 3)).astype(np.float32)
    xyz[:, n // 2:] = xyz[:, : n - n // 2]          # duplicates
    new_xyz = xyz[:, rng.choice(n, m, replace=False)].copy()
    new_xyz[:, 0] = 100.0                             # a centroid with no neighbour
    idx = pu.ball_query(radius, ns, torch.from_numpy(xyz).to(DEV), torch.from_numpy(new_xyz).to(DEV))
    np.testing.assert_array_equal(idx.cpu().numpy(), oracle.ball_query(radius, ns, xyz, new_xyz))
    feats = rng.normal(size=(2, 5, n)).astype(np.float32)
    g = pu.grouping_operation(torch.from_numpy(feats).to(DEV), idx)
    np.testing.assert_array_equal(g.cpu().numpy(), oracle.grouping_operation(feats, idx.cpu().numpy()))
    fidx = torch.from_numpy(rng.integers(0, n, size=(2, m)).astype(np.int32)).to(DEV)
    ga = pu.gather_operation(torch.from_numpy(feats).to(DEV), fidx)
    np.testing.assert_array_equal(ga.cpu().numpy(), oracle.gather_operation(feats, fidx.cpu().numpy()))


# ---------------------------------------------------------------- encoder
@pytest.mark.parametrize("arith", ["split_f16", "f32"])
@pytest.mark.parametrize("tag", ["n1024", "n2048"])
def test_encoder_levels_vs_golden(tag, arith, score_agent):
    """Every level against the reference's own per-level outputs: FPS / ball-query indices bit-exact,
    features within 1e-5 of max|ref|, for the split-f16 levels 2-3 (default) and exact fp32."""
    g = golden("encoder")
    pts = torch.from_numpy(g[f"{tag}_pts"]).to(DEV)
    score_agent.encoder.set_arith(arith)
    try:
        feat, ws = score_agent.encoder.forward(pts, return_workspace=True)
    finally:
        score_agent.encoder.set_arith("split_f16")
    torch.cuda.synchronize()
    B, N = pts.shape[:2]
    levels = score_agent.encoder.levels(B, N, ws)
    for lv in range(4):
        np.testing.assert_array_equal(levels[lv]["fps_idx"].cpu().numpy(), g[f"{tag}_l{lv}_fps"])
        np.testing.assert_array_equal(levels[lv]["new_xyz"].cpu().numpy(), g[f"{tag}_l{lv}_new_xyz"])
        for b in range(2):
            np.testing.assert_array_equal(levels[lv]["ball_idx"][b].cpu().numpy(), g[f"{tag}_l{lv}_ball{b}"])
        f0 = levels[lv]["features"][0].cpu().numpy().T        # point-major -> (C, M)
        assert rel(f0, g[f"{tag}_l{lv}_feat0"]) < 1e-5, lv
    assert rel(feat, g[f"{tag}_feat"]) < 1e-5


@pytest.mark.parametrize("n,grid", [(1024, True), (2048, True), (1500, False), (600, True), (4096, True)])
def test_encoder_fps_chain_vs_oracle(n, grid, score_agent):
    """The encoder's per-object FPS chain (one wave per object) vs the serialized oracle, level by
    level, on tie-heavy integer grids and ragged sizes; and the two ball lists of every level the same
    forward() wrote, against the oracle's ball query over those centroids."""
    from genpose2_amd import arch
    from oracle import oracle
    rng = np.random.default_rng(n)
    pts = (rng.integers(0, 6, size=(2, n, 3)) * 0.05 if grid else rng.normal(size=(2, n, 3)) * 0.1)
    pts = pts.astype(np.float32)
    _, ws = score_agent.encoder.forward(torch.from_numpy(pts).to(DEV), return_workspace=True)
    levels = score_agent.encoder.levels(2, n, ws)
    cur = pts
    for lv in range(4):
        idx = oracle.furthest_point_sample(cur, arch.NPOINTS[lv])
        np.testing.assert_array_equal(levels[lv]["fps_idx"].cpu().numpy(), idx, err_msg=f"level {lv}")
        prev, cur = cur, np.take_along_axis(cur, idx[..., None].astype(np.int64), 1)
        np.testing.assert_array_equal(levels[lv]["new_xyz"].cpu().numpy(), cur)
        for b, (radius, ns) in enumerate(zip(arch.RADII[lv], arch.NSAMPLES[lv])):
            np.testing.assert_array_equal(levels[lv]["ball_idx"][b].cpu().numpy(),
                                          oracle.ball_query(radius, ns, prev, cur), err_msg=f"level {lv} radius {radius}")


@pytest.mark.parametrize("n,B", [(1024, 64), (2048, 64), (1024, 3)])
def test_encoder_split_matches_f32_full_size(n, B, score_agent):
    """64 objects (config-2 batch; N=2048 as config 5), and 3 (a ragged last GroupAll point block): the
    split-f16 levels 0-3 and GroupAll against the exact fp32 kernels level by level (1e-5 of max per
    object) and the final 1024-d feature."""
    from genpose2_amd import synthetic
    pts, _ = synthetic.make_batch(2, B, n, n_unique_every=5)
    t = torch.from_numpy(pts).to(DEV)
    enc = score_agent.encoder
    out = {}
    for arith in ("f32", "split_f16"):
        enc.set_arith(arith)
        feat, ws = enc.forward(t, return_workspace=True)
        lv = enc.levels(B, n, ws)
        out[arith] = (feat.cpu().numpy(), [lv[i]["features"].cpu().numpy() for i in (0, 1, 2, 3)])
    enc.set_arith("split_f16")
    for a, r in zip(out["split_f16"][1] + [out["split_f16"][0]], out["f32"][1] + [out["f32"][0]]):
        err = np.abs(a - r).reshape(B, -1).max(1) / np.abs(r).reshape(B, -1).max(1)
        assert err.max() < 1e-5, err.max()
    assert not np.array_equal(out["split_f16"][0], out["f32"][0])   # the two paths differ in arithmetic


@pytest.mark.parametrize("N", [1024, 2048])
def test_encoder_shared_geometry_bit_exact(N, score_agent):
    """gp_encoder_geometry + gp_encoder_forward_geom: the EnergyNet encoder over the ScoreNet encoder's
    geometry of the same points, and the ScoreNet encoder over its own, equal the self-contained
    gp_encoder_forward bit for bit (split-f16 and exact fp32), and the geometry equals what a forward
    pass leaves in the workspace."""
    from genpose2_amd import synthetic
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    energy = PoseNet(GenPoseConfig(device=DEV, agent_type="energy")).eval()
    pts, _ = synthetic.make_batch(21, 10, N, n_unique_every=5)
    p = torch.from_numpy(pts).to(DEV)
    for arith, overlap in (("split_f16", True), ("split_f16", False), ("f32", True)):
        for a in (score_agent, energy):
            a.encoder.set_arith(arith)
        # overlap: levels 1-3 of the geometry on a side stream while level 0's MLPs run (EncoderGeometry.event0)
        score_agent.encoder.geometry_overlap = overlap
        ref_s, ws_s = score_agent.encoder.forward(p, return_workspace=True)
        lv_ref = [{k: (v.clone() if torch.is_tensor(v) else [x.clone() for x in v]) for k, v in d.items()
                   if k != "features"} for d in score_agent.encoder.levels(10, N, ws_s)]
        ref_e = energy.encoder.forward(p)
        data = {"pts": p}
        score_agent.encode_geometry(data)
        got_e = energy.encoder.forward(p, geometry=data["enc_geometry"])
        got_s = score_agent.encoder.forward(p, geometry=data["enc_geometry"])
        torch.cuda.synchronize()
        assert (data["enc_geometry"].event0 is not None) == overlap
        assert torch.equal(got_s, ref_s) and torch.equal(got_e, ref_e), (arith, overlap)
        for d0, d1 in zip(lv_ref, score_agent.encoder.levels(10, N, data["enc_geometry"].ws)):
            for k in d0:
                if torch.is_tensor(d0[k]):
                    assert torch.equal(d0[k], d1[k]), k
                else:
                    assert all(torch.equal(x, y) for x, y in zip(d0[k], d1[k])), k
        with pytest.raises(ValueError):
            energy.encoder.forward(p.clone(), geometry=data["enc_geometry"])   # other points
        score_agent.encoder.forward(p[:5].contiguous())                        # the producer re-encodes
        with pytest.raises(ValueError, match="stale"):
            energy.encoder.forward(p, geometry=data["enc_geometry"])
    for a in (score_agent, energy):
        a.encoder.set_arith("split_f16")
    score_agent.encoder.geometry_overlap = True


def test_encoder_geometry_then_forward_unsynchronised(score_agent):
    """The producer's own writes are ordered after its side-stream geometry (levels 1-3): geometry() followed at
    once -- no synchronize, no consumer waiting on its event -- by a self-contained forward() of other points, and
    by a second geometry(), leave the workspace and features exactly as an isolated forward() does."""
    from genpose2_amd import synthetic
    enc = score_agent.encoder
    pts, _ = synthetic.make_batch(31, 64, 1024, n_unique_every=7)
    other, _ = synthetic.make_batch(32, 64, 1024, n_unique_every=7)
    p, o = torch.from_numpy(pts).to(DEV), torch.from_numpy(other).to(DEV)
    ref_p = enc.forward(p).clone()
    ref_o = enc.forward(o).clone()
    torch.cuda.synchronize()
    assert enc.geometry_overlap
    for _ in range(3):
        enc.geometry(p)
        got_o = enc.forward(o)          # rewrites every level's geometry while the side stream may still run
        enc.geometry(o)
        enc.geometry(p)                 # a second geometry() over level 0 while levels 1-3 of the first run
        g = enc.geometry(p)
        got_p = enc.forward(p, geometry=g)
        torch.cuda.synchronize()
        assert torch.equal(got_o, ref_o) and torch.equal(got_p, ref_p)


def test_encoder_batch_independence(score_agent):
    from genpose2_amd import synthetic
    pts, _ = synthetic.make_batch(5, 6, 1024, n_unique_every=4)
    full = score_agent.encoder.forward(torch.from_numpy(pts).to(DEV)).cpu()
    part = score_agent.encoder.forward(torch.from_numpy(pts[2:4].copy()).to(DEV)).cpu()
    assert torch.equal(full[2:4], part)   # objects are independent: bitwise


# ---------------------------------------------------------------- heads
def test_score_and_energy_heads_vs_golden(score_agent):
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("heads")
    for kind, agent in (("score", score_agent), ("energy", PoseNet(GenPoseConfig(device=DEV, agent_type="energy")))):
        feat = torch.from_numpy(g["pts_feat"]).to(DEV)
        pobj = agent.heads.object_proj(feat)              # one object per row (k=1)
        out = []
        for r in range(g["t"].shape[0]):
            trow, sig = agent._time_row_and_sigma(agent.heads, float(g["t"][r, 0]))
            x = torch.from_numpy(g["pose"][r:r + 1]).to(DEV)
            if kind == "score":
                out.append(agent.heads.score(pobj[r:r + 1], trow, sig, x, 1))
            else:
                out.append(agent.heads.energy(pobj[r:r + 1], trow, sig, x, 1))
        out = torch.cat(out).cpu().numpy()
        ref = g[kind]
        err = np.abs(out - ref).max(1) / np.abs(ref).max(1)
        assert err.max() < 1e-5, kind


# ---------------------------------------------------------------- PC sampler
@pytest.mark.parametrize("name", ["pc_k10_t100", "pc_k50_t20"])
def test_pc_pred_func_vs_golden(name):
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden(name)
    K, T = int(g["K"]), int(g["T"])
    agent = PoseNet(GenPoseConfig(device=DEV, sampling_steps=T)).eval()
    agent.noise_feed = NoiseFeed(*(torch.from_numpy(g[k]) for k in ("prior", "z1", "z2")))
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    pose, q, q_avg, xs = agent.pred_func(data, repeat_num=K, return_average_res=True, return_process=True)
    ref = g["pred_pose"]
    assert pose.dtype == torch.float32 and pose.shape == ref.shape
    assert data["rgb_feat"] is None and rel(data["pts_feat"], g["pts_feat"]) < 1e-5
    p = pose.cpu().numpy()
    assert np.abs(p[..., :6] - ref[..., :6]).max() < 1e-4
    assert rel(p[..., 6:], ref[..., 6:]) < 1e-5
    assert np.abs(q.cpu().numpy()[..., :4] - g["pred_q"][..., :4]).max() < 1e-4
    assert rel(q.cpu().numpy()[..., 4:], g["pred_q"][..., 4:]) < 1e-5
    if "xs" in g.files:
        assert np.abs(xs.cpu().numpy()[..., :6] - g["xs"][..., :6]).max() < 1e-4
    qa, qa_ref = q_avg.cpu().numpy(), g["pred_q_avg"]
    assert np.abs(qa[:, :4] - qa_ref[:, :4]).max() < 1e-3 and rel(qa[:, 4:], qa_ref[:, 4:]) < 1e-5


def test_load_ckpt_reproduces_golden(tmp_path):
    """PoseNet.load_ckpt on a reference-format checkpoint (save_ckpt layout, model_path=True as
    evaluation_single.py passes it) rebuilds the device model and reproduces golden_pc_k10_t100."""
    from conftest import write_reference_checkpoint
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("pc_k10_t100")
    K, T = int(g["K"]), int(g["T"])
    path = write_reference_checkpoint(str(tmp_path / "score.pth"), "score", prefix="module.")
    agent = PoseNet(GenPoseConfig(device=DEV, sampling_steps=T, seed=5)).eval()   # other weights first
    agent.load_ckpt(model_dir=path, model_path=True)
    assert agent.weights_source == path
    agent.noise_feed = NoiseFeed(*(torch.from_numpy(g[k]) for k in ("prior", "z1", "z2")))
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=K)
    p = pose.cpu().numpy()
    assert np.abs(p[..., :6] - g["pred_pose"][..., :6]).max() < 1e-4
    assert rel(p[..., 6:], g["pred_pose"][..., 6:]) < 1e-5
    with pytest.raises(ValueError):
        agent.load_ckpt(name="latest", model_dir=str(tmp_path))


def test_pc_full_size_properties():
    """Config 2 (B=64, N=1024, K=50, T=500) with device Philox noise: size-independent checks."""
    from genpose2_amd import synthetic
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    pts, center = synthetic.make_batch(2, 64, 1024)
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    a1 = PoseNet(GenPoseConfig(device=DEV, sampling_steps=500, noise_seed=3)).eval()
    a2 = PoseNet(GenPoseConfig(device=DEV, sampling_steps=500, noise_seed=3)).eval()
    p1, q1 = a1.pred_func(dict(data), repeat_num=50)
    p2, q2 = a2.pred_func(dict(data), repeat_num=50)
    assert p1.shape == (64, 50, 9) and q1.shape == (64, 50, 7)
    assert torch.isfinite(p1).all() and torch.isfinite(q1).all()
    assert torch.equal(p1, p2) and torch.equal(q1, q2)                  # deterministic given the seed
    r = p1.reshape(-1, 9).double()
    b1, b2 = r[:, :3], r[:, 3:6]
    assert (b1.norm(dim=1) - 1).abs().max() < 1e-5 and (b2.norm(dim=1) - 1).abs().max() < 1e-5
    assert (b1 * b2).sum(1).abs().max() < 1e-5                            # Gram-Schmidt output
    assert (q1[..., :4].double().norm(dim=-1) - 1).abs().max() < 1e-5     # unit quaternions
    p3, _ = a1.pred_func(dict(data), repeat_num=50)                      # next call, next noise
    assert not torch.equal(p1, p3)


def _f16x3_vs_f32(B, T):
    from genpose2_amd import synthetic
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    pts, center = synthetic.make_batch(5, B, 1024)
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    out = {}
    for arith in ("f16x3", "f32"):
        a = PoseNet(GenPoseConfig(device=DEV, sampling_steps=T, noise_seed=7)).eval()
        a.heads.set_arith(arith)
        out[arith] = a.pred_func(dict(data), repeat_num=50)[0].cpu().numpy()
    return out["f16x3"], out["f32"]


@pytest.mark.parametrize("B,T", [(16, 100), (96, 20)])
def test_pc_f16x3_matches_exact_f32(B, T):
    """The f16x3 head GEMMs (default) against the exact fp32 MFMA path on identical inputs and noise,
    at the PC golden tests' tolerances (1e-4 rotation, 1e-5 relative translation). 800 rows run
    16-candidate tiles; 4800 rows (> PC_SPLIT_NT2_MIN = 4096) run the f16x3 path's 32-candidate
    tiles against the fp32 path's 16-candidate tiles. The two differ only in how fp32 products are
    accumulated, which the Langevin trajectories amplify unevenly (measured on the round-4 build: p99.9
    1.7e-5 / 2.4e-5, max 2.3e-5 / 2.5e-5). The bar, 5e-5 at p99.9 and 1e-4 at the worst candidate, is
    about 2x the measured spread, so the test holds the f16x3 accuracy claim rather than the old split-f16 bar
    (p99.9 < 1e-4, max < 3e-4). The bar against the reference itself is
    test_pc_large_rows_vs_reference."""
    p, ref = _f16x3_vs_f32(B, T)
    err = np.abs(p[..., :6] - ref[..., :6]).max(-1)
    print(f"B={B} T={T}: f16x3 vs exact fp32 rotation p99.9 {np.quantile(err, 0.999):.2e} max {err.max():.2e}")
    assert np.quantile(err, 0.999) < 5e-5 and err.max() < 1e-4, (np.quantile(err, 0.999), err.max())
    assert rel(p[..., 6:], ref[..., 6:]) < 1e-5
    assert not np.array_equal(p, ref)   # the two paths really differ in arithmetic


@pytest.mark.parametrize("arith", ARITHS3)
@pytest.mark.parametrize("name", ["pc_r4800_t100", "pc_r12800_t100", "pc_r12800_t500"])
def test_pc_large_rows_vs_reference(name, arith):
    """The kernels the north-star shapes run (R = 4800 / 12,800 rows: the split path's 32-candidate
    tiles) against the reference itself at those sizes, with the reference's noise (regenerated from
    committed seeds, tests/golden/large_noise.py). The bar is calibrated on the reference's own fp32
    error against its float64 run (check_pc_calibrated); translations additionally within 1e-5
    relative of the reference's fp32 output."""
    import large_noise
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden(f"large_{name}")
    _, _, B, K, T, _, _ = large_noise.CASES[name]
    pts, center, prior, z1, z2 = large_noise.inputs(name)
    agent = PoseNet(GenPoseConfig(device=DEV, sampling_steps=T)).eval()
    set_arith(agent, arith)
    agent.noise_feed = NoiseFeed(torch.from_numpy(prior), torch.from_numpy(np.ascontiguousarray(z1)),
                                 torch.from_numpy(np.ascontiguousarray(z2)))
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=K)
    p = pose.cpu().numpy()
    stats = large_noise.check_pc_calibrated(p, g)
    print(name, arith, stats)
    assert rel(p[..., 6:], g["pred_pose"][..., 6:]) < 1e-5
    assert torch.isfinite(q).all()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", ["ode_r4800", "ode_r12800"])
def test_ode_large_rows_vs_reference(name, arith):
    """The shipped ODE setting (T0=0.55, RK45) at R = 4800 / 12,800 against the reference: identical
    nfev; rotation within the north-star 1e-4 of both the reference's fp32 run and its float64 run,
    translation within 1e-5 relative (large_noise.check_ode, which says why RK45 solutions differ at
    the solver's tolerance scale). `arith` sets both the head GEMMs and the encoder's levels 2-3."""
    import large_noise
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden(f"large_{name}")
    _, _, B, K, _, T0, _ = large_noise.CASES[name]
    pts, center, prior, _, _ = large_noise.inputs(name)
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None)).eval()
    set_arith(agent, arith)
    agent.noise_feed = NoiseFeed(torch.from_numpy(prior))
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=K, T0=T0)
    p = pose.cpu().numpy()
    assert agent.last_nfev == int(g["nfev"])
    print(name, arith, large_noise.check_ode(p, g))


# ---------------------------------------------------------------- ODE sampler
def test_ode_pred_func_vs_golden():
    """The shipped setting (T0=0.55, t_eval of 20 steps): identical nfev, final pose within the north-star
    1e-4 / 1e-5, and the whole returned trajectory (return_process, host controller) within the same bar."""
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("ode")
    tag, rot_tol, tr_rel = "t055_s20", 1e-4, 1e-5
    steps = int(g[f"{tag}_steps"])
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=steps))
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    data = {"pts": torch.from_numpy(g[f"{tag}_pts"]).to(DEV),
            "pts_center": torch.from_numpy(g[f"{tag}_pts_center"]).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=5, T0=float(g[f"{tag}_T0"]))
    ref = g[f"{tag}_pred_pose"]
    assert pose.dtype == torch.float64
    p = pose.cpu().numpy()
    assert np.abs(p[..., :6] - ref[..., :6]).max() < rot_tol
    assert rel(p[..., 6:], ref[..., 6:]) < tr_rel
    assert np.abs(q.cpu().numpy()[..., :4] - g[f"{tag}_pred_q"][..., :4]).max() < rot_tol * 10
    assert agent.last_nfev == int(g[f"{tag}_nfev"])
    # return_process: the whole trajectory (solve_ivp outputs, GS'ed, + pts_center) from the host controller
    # (device pow() vs glibc: last-bit scalar differences, which agree to 1e-6 at this T0)
    nfev_dev = agent.last_nfev
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    pose2, xs = agent.pred_func(data, repeat_num=5, T0=float(g[f"{tag}_T0"]), return_process=True)
    assert agent.last_nfev == nfev_dev
    assert (pose2 - pose).abs().max().item() < 1e-6 * max(1.0, pose.abs().max().item())
    xr = g[f"{tag}_xs"]
    assert xs.shape == xr.shape
    x = xs.cpu().numpy()
    err = np.abs(x[..., :6] - xr[..., :6])
    print(f"{tag}: xs rotation max {err.max():.2e}, translation rel {rel(x[..., 6:], xr[..., 6:]):.2e}")
    assert err.max() < rot_tol and rel(x[..., 6:], xr[..., 6:]) < tr_rel


@pytest.mark.parametrize("arith", ARITHS)
def test_ode_t1_calibrated_vs_float64(arith):
    """T0=1 with t_eval unset (golden_ode "t1_none"). RK45 at rtol=atol=1e-5 from sigma(1)=50 lets the
    float32 rounding of the score steer its accept/reject path: the reference itself takes 290 evaluations
    with its float32 network and 278 with the same network in float64, and the two trajectories part by
    1.4e-4 in rotation (golden_ode_trace.json, golden_ode_t1_grid.npz; tests/golden/make_ode_trace.py). So
    this case is held to the calibrated bar, like the large PC fixtures: against the reference's float64 run,
    the final pose and the whole trajectory -- compared on a fixed grid of 101 times through the t_eval
    output, which RK45 interpolates without changing its steps -- within 2x the reference float32 run's own
    error (rotation max, translation max relative). nfev and the first attempt where the controller parts
    from the reference's float32 run are printed for the record."""
    import json
    from conftest import GOLDEN
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("ode")
    cal = np.load(f"{GOLDEN}/golden_ode_t1_grid.npz")
    with open(f"{GOLDEN}/golden_ode_trace.json") as f:
        ref_trace = json.load(f)["t1_none"]["ref32"]["attempts"]
    tag = "t1_none"
    data = {"pts": torch.from_numpy(g[f"{tag}_pts"]).to(DEV),
            "pts_center": torch.from_numpy(g[f"{tag}_pts_center"]).to(DEV)}
    # final pose (t_eval unset: denoise step (1 - eps) / 1000), device controller and host controller
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None))
    set_arith(agent, arith)
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    pose = agent.pred_func(dict(data), repeat_num=5, T0=1.0)[0].cpu().numpy()
    nfev = agent.last_nfev
    trace = []
    agent.ode_trace = trace
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    pose_h = agent.pred_func(dict(data), repeat_num=5, T0=1.0)[0].cpu().numpy()
    agent.ode_trace = None
    assert agent.last_nfev == nfev
    ref32, ref64 = g[f"{tag}_pred_pose"], cal["pred_pose64"]

    def errs(a, b):
        return float(np.abs(a[..., :6] - b[..., :6]).max()), rel(a[..., 6:], b[..., 6:])
    r_rot, r_tr = errs(ref32, ref64)
    o_rot, o_tr = errs(pose, ref64)
    h_rot, h_tr = errs(pose_h, ref64)
    part = next((i for i, (a, b) in enumerate(zip(trace, ref_trace)) if (a[2] < 1) != (b[2] < 1)), None)
    print(f"t1_none {arith}: nfev {nfev} (reference fp32 {int(cal['nfev32'])}, float64 {int(cal['nfev64'])}); "
          f"first accept/reject decision differing from the reference fp32 run: attempt {part} "
          f"({trace[part] if part is not None else None} vs {ref_trace[part] if part is not None else None}); "
          f"final pose vs float64: rotation {o_rot:.2e} (host controller {h_rot:.2e}), translation rel {o_tr:.2e} "
          f"(reference fp32 {r_rot:.2e} / {r_tr:.2e}); vs reference fp32 rotation {errs(pose, ref32)[0]:.2e}")
    assert o_rot <= 2 * r_rot and o_tr <= 2 * r_tr
    assert h_rot <= 2 * r_rot and h_tr <= 2 * r_tr
    # the trajectory on the grid
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=len(cal["grid"])))
    set_arith(agent, arith)
    agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
    _, xs = agent.pred_func(dict(data), repeat_num=5, T0=1.0, return_process=True)
    assert agent.last_nfev == nfev    # t_eval interpolates; the steps are those of the run above
    x = xs.cpu().numpy()
    assert x.shape == cal["xs64"].shape
    x_rot, x_tr = errs(x, cal["xs64"])
    rx_rot, rx_tr = errs(cal["xs32"], cal["xs64"])
    print(f"t1_none {arith}: trajectory on the grid vs float64: rotation {x_rot:.2e}, translation rel {x_tr:.2e} "
          f"(reference fp32 {rx_rot:.2e} / {rx_tr:.2e}); vs reference fp32 rotation {errs(x, cal['xs32'])[0]:.2e}")
    assert x_rot <= 2 * rx_rot and x_tr <= 2 * rx_tr


@pytest.mark.parametrize("tag", ["t055_s20", "t1_none"])
def test_ode_device_controller_matches_host_controller(tag):
    """The device-resident RK45 controller (default) takes the same accept/reject path as the
    host restatement of scipy (rk45_drive): same nfev; poses equal up to the last-bit differences of
    device pow() in the per-stage sigma/g scalars."""
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("ode")
    steps = int(g[f"{tag}_steps"])
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None if steps < 0 else steps))
    data = {"pts": torch.from_numpy(g[f"{tag}_pts"]).to(DEV),
            "pts_center": torch.from_numpy(g[f"{tag}_pts_center"]).to(DEV)}
    out = {}
    for host in (False, True):
        agent.ode_host_control = host
        agent.noise_feed = NoiseFeed(torch.from_numpy(g[f"{tag}_prior"]))
        pose, q = agent.pred_func(dict(data), repeat_num=5, T0=float(g[f"{tag}_T0"]))
        out[host] = (pose.cpu().numpy(), agent.last_nfev)
    if tag == "t055_s20":
        assert out[False][1] == out[True][1]
        assert np.abs(out[False][0] - out[True][0]).max() < 1e-6 * max(1.0, np.abs(out[True][0]).max())
    else:
        # T0=1: the adaptive path amplifies last-bit scalar differences; both controllers must meet the
        # golden bar (test_ode_pred_func_vs_golden's tolerances) and agree to 1e-4 relative
        ref = g[f"{tag}_pred_pose"]
        for pz, _ in out.values():
            assert np.abs(pz[..., :6] - ref[..., :6]).max() < 5e-4 and rel(pz[..., 6:], ref[..., 6:]) < 1e-4
        assert np.abs(out[False][0] - out[True][0]).max() < 1e-4 * max(1.0, np.abs(out[True][0]).max())


@pytest.mark.parametrize("case", ["t1_none", "ode_r4800", "ode_r12800"])
def test_ode_fused_attempt_equals_stage_launches(case, monkeypatch):
    """The device-controlled RK45 attempt as ONE launch (ode_attempt_kernel: the six stages back to back in
    each workgroup, default) against six stage launches (GENPOSE2_ODE_FUSED=0): the same nfev and the same
    bits, at 16-, 32- and 64-candidate tiles (R = 5, 4800, 12,800 rows; T0 = 1 is the case whose
    accept/reject path follows last-bit differences)."""
    import large_noise
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    if case == "t1_none":
        g = golden("ode")
        pts, center, prior, K, T0 = (g["t1_none_pts"], g["t1_none_pts_center"], g["t1_none_prior"], 5, 1.0)
    else:
        _, _, B, K, _, T0, _ = large_noise.CASES[case]
        pts, center, prior, _, _ = large_noise.inputs(case)
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None)).eval()
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GENPOSE2_ODE_FUSED", fused)
        agent.noise_feed = NoiseFeed(torch.from_numpy(prior))
        pose, q = agent.pred_func(dict(data), repeat_num=K, T0=T0)
        out[fused] = (pose.cpu().numpy(), q.cpu().numpy(), agent.last_nfev)
    assert out["1"][2] == out["0"][2]
    np.testing.assert_array_equal(out["1"][0], out["0"][0])
    np.testing.assert_array_equal(out["1"][1], out["0"][1])


def test_ode_device_controller_full_size():
    """Config-2 shape (B=64, K=50, T0=0.55): device and host controllers agree on nfev, outputs are
    finite, rotations orthonormal."""
    from genpose2_amd import synthetic
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    pts, center = synthetic.make_batch(2, 64, 1024)
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None))
    prior = torch.randn(64 * 50, 9, generator=torch.Generator().manual_seed(11))
    res = {}
    for host in (False, True):
        agent.ode_host_control = host
        agent.noise_feed = NoiseFeed(prior)
        pose, q = agent.pred_func(dict(data), repeat_num=50, T0=0.55)
        res[host] = (pose, agent.last_nfev)
    assert res[False][1] == res[True][1]
    p = res[False][0]
    assert torch.isfinite(p).all()
    r = p.reshape(-1, 9)
    assert (r[:, :3].norm(dim=1) - 1).abs().max() < 1e-9 and (r[:, 3:6].norm(dim=1) - 1).abs().max() < 1e-9
    assert (res[False][0] - res[True][0]).abs().max() < 1e-5


@pytest.mark.parametrize("mode", ["pc", "ode"])
def test_tracking_warm_start_vs_golden(mode):
    """init_x + T0=0.2 as the tracking runner calls pred_func."""
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("tracking")
    K, T, T0 = int(g["K"]), int(g["T"]), float(g["T0"])
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=[mode], sampling_steps=T if mode == "pc" else None))
    agent.noise_feed = NoiseFeed(*(torch.from_numpy(g[k]) for k in ("prior", "z1", "z2")))
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    pose, q = agent.pred_func(data, repeat_num=K, T0=T0, init_x=torch.from_numpy(g["init_x"]).to(DEV))
    ref = g[f"{mode}_pred_pose"]
    p = pose.cpu().numpy()
    assert np.abs(p[..., :6] - ref[..., :6]).max() < 1e-4
    assert rel(p[..., 6:], ref[..., 6:]) < 1e-5
    assert np.abs(q.cpu().numpy()[..., :4] - g[f"{mode}_pred_q"][..., :4]).max() < 1e-3
    if mode == "ode":
        assert agent.last_nfev == int(g["ode_nfev"])


# ---------------------------------------------------------------- energy / ranking / scale
def test_energy_ranking_aggregate_scale_vs_golden():
    from genpose2_amd import aggregate
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("pipeline")
    e_agent = PoseNet(GenPoseConfig(device=DEV, agent_type="energy")).eval()
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    pose = torch.from_numpy(g["pred_pose"]).to(DEV)
    energy = e_agent.get_energy(data, pose, T=1e-5, mode="test", extract_feature=True)
    assert rel(energy, g["energy"]) < 1e-5
    order_ref = np.argsort(-g["energy"], axis=1, kind="stable")
    order = np.argsort(-energy.cpu().numpy(), axis=1, kind="stable")
    np.testing.assert_array_equal(order, order_ref)                      # identical candidate ranking
    sp, se = aggregate.sort_poses_by_energy(pose, torch.from_numpy(g["energy"]).to(DEV))
    np.testing.assert_array_equal(sp.cpu().numpy(), g["sorted_pose"])
    for c in (0, 1):
        agg = aggregate.aggregate_pose(pose, torch.from_numpy(g["energy"]).to(DEV), clustering=c)
        assert np.abs(agg.cpu().numpy() - g[f"aggregated_c{c}"]).max() < 1e-4
    agg = aggregate.aggregate_pose(torch.from_numpy(g["cl_pose"]).to(DEV), torch.from_numpy(g["cl_energy"]).to(DEV))
    assert np.abs(agg.cpu().numpy() - g["cl_aggregated"]).max() < 1e-4
    s_agent = PoseNet(GenPoseConfig(device=DEV, agent_type="scale")).eval()
    axes, length = s_agent.pred_scale_func({"pts_feat": torch.from_numpy(g["pts_feat"]).to(DEV), "rgb_feat": None,
                                            "axes": torch.from_numpy(g["scale_axes"]).to(DEV)})
    assert rel(length, g["scale_length"]) < 1e-5


@pytest.mark.parametrize("B,K", [(4, 16), (96, 50), (256, 50)])
def test_pc_step_score_equals_eval_score(B, K):
    """The PC step's score (16, 32 or 64 candidates per workgroup: head_pick_nt by row count) equals the
    score-evaluation kernel's (16 per workgroup) on the same states bit for bit: both run the same
    trunk, and per-candidate arithmetic does not depend on the tile (scripts/head_nt_diff.py)."""
    from genpose2_amd import sde
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    torch.manual_seed(B)
    h = PoseNet(GenPoseConfig(device=DEV, sampling_steps=2)).eval().heads
    R = B * K
    tab = sde.pc_step_table(2)
    tproj = h.time_proj(torch.from_numpy(tab[:, 0]).to(DEV))
    pobj = h.object_proj(torch.rand(B, 1024, device=DEV))
    x0 = torch.randn(R, 9, device=DEV)
    z = torch.zeros(2, R, 9, device=DEV)
    _, _, xs = h.pc_sample(pobj, tproj, tab, x0.clone(), K, torch.zeros(B, 3, device=DEV), z1=z, z2=z, want_xs=True)
    s_pc = h._pc_ws[: R * 9 * 4].view(torch.float32).view(R, 9).clone()
    s_ev = h.score(pobj, tproj[1:2].contiguous(), float(tab[1, 1]), xs[:, 0].contiguous(), K)
    assert torch.equal(s_pc, s_ev)


def test_energy_per_object_t_batched():
    """get_energy(T=None) (posenet_agent.py:677-687): per-object t drawn from torch's default generator
    with the reference's call shape, evaluated per distinct t; equal to get_energy at each object's fixed t."""
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("pipeline")
    e_agent = PoseNet(GenPoseConfig(device=DEV, agent_type="energy")).eval()
    pts, center = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["pts_center"]).to(DEV)
    pose = torch.from_numpy(g["pred_pose"]).to(DEV)
    bs = pts.shape[0]
    torch.manual_seed(11)
    e = e_agent.get_energy({"pts": pts, "pts_center": center}, pose, T=None, mode="test").cpu()
    torch.manual_seed(11)
    ts = PoseNet.per_object_energy_t(bs)
    assert len(torch.unique(ts)) > 1
    for b in range(bs):
        eb = e_agent.get_energy({"pts": pts[b:b + 1], "pts_center": center[b:b + 1]}, pose[b:b + 1], T=float(ts[b]),
                                mode="test").cpu()
        assert rel(e[b:b + 1], eb.numpy()) < 1e-6


def test_energy_after_encode_func_equals_extracting_call():
    """encode_func forms the energy net's object projection with the features (the runner runs it beside the
    score sampler); get_energy(extract_feature=False) on that dict equals the extracting call bit for bit, and
    a replaced pts_feat is not paired with the stale projection."""
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    g = golden("pipeline")
    e_agent = PoseNet(GenPoseConfig(device=DEV, agent_type="energy")).eval()
    pts, center = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["pts_center"]).to(DEV)
    pose = torch.from_numpy(g["pred_pose"]).to(DEV)
    e_ref = e_agent.get_energy({"pts": pts, "pts_center": center}, pose, T=1e-5, mode="test")
    data = {"pts": pts, "pts_center": center}
    e_agent.encode_func(data)
    assert "_energy_pobj" in data
    assert torch.equal(e_agent.get_energy(data, pose, T=1e-5, mode="test", extract_feature=False), e_ref)
    data["pts_feat"] = data["pts_feat"].flip(0).contiguous()
    e_flip = e_agent.get_energy(data, pose, T=1e-5, mode="test", extract_feature=False)
    plain = {"pts_feat": data["pts_feat"], "pts_center": center}
    assert torch.equal(e_flip, e_agent.get_energy(plain, pose, T=1e-5, mode="test", extract_feature=False))
    assert not torch.equal(e_flip, e_ref)


def test_runner_pipeline_smoke():
    from genpose2_amd import synthetic
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.runner import EvaluationPipeline
    pts, center = synthetic.make_batch(3, 8, 1024)
    pipe = EvaluationPipeline(GenPoseConfig(device=DEV, sampling_steps=50, eval_repeat_num=50), with_scale=True)
    out = pipe.run({"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)})
    assert out.pred_pose.shape == (8, 50, 9) and out.energy.shape == (8, 50, 2)
    assert out.aggregated.shape == (8, 4, 4) and out.length.shape == (8, 3)
    assert torch.isfinite(out.aggregated).all() and torch.isfinite(out.length).all()


# ---------------------------------------------------------------- device ranking / aggregation
def _clustered_candidates(rng, B, K, modes=3, spread=0.02):
    """K candidates per object around `modes` random rotations (6D) + noise, random translations."""
    from oracle import oracle
    pose = np.zeros((B, K, 9), np.float32)
    for b in range(B):
        centers = oracle.rot6_to_matrix(rng.normal(size=(modes, 6)).astype(np.float32))
        which = rng.integers(0, modes, size=K)
        R = centers[which] + rng.normal(scale=spread, size=(K, 3, 3)).astype(np.float32)
        pose[b, :, :3] = R[:, :, 0]
        pose[b, :, 3:6] = R[:, :, 1]
        pose[b, :, 6:] = rng.normal(scale=0.3, size=(K, 3))
    return pose


@pytest.mark.parametrize("B,K,ties", [(64, 50, False), (16, 100, True), (5, 7, True), (3, 300, False)])
def test_rank_aggregate_vs_oracle(B, K, ties):
    from genpose2_amd import aggregate
    from oracle import oracle
    rng = np.random.default_rng(B * K)
    pose = _clustered_candidates(rng, B, K)
    energy = rng.normal(size=(B, K, 2)).astype(np.float32)
    if ties:   # quantised energies: many equal values -> order by lower candidate index
        energy = np.round(energy * 2) / 2
    tp, te = torch.from_numpy(pose).to(DEV), torch.from_numpy(energy).to(DEV)
    sp, se = aggregate.sort_poses_by_energy(tp, te)
    rsp, rse, _, _ = oracle.sort_poses_by_energy(pose, energy)
    np.testing.assert_array_equal(sp.cpu().numpy(), rsp)
    np.testing.assert_array_equal(se.cpu().numpy(), rse)
    for c in (0, 1):
        if c and int(0.1667 * int(K * 0.4)) < 1:   # sklearn rejects min_samples=0; so does the kernel
            from genpose2_amd._lib import GenPoseHipError
            with pytest.raises(GenPoseHipError):
                aggregate.aggregate_pose(tp, te, clustering=c)
            continue
        agg = aggregate.aggregate_pose(tp, te, clustering=c)
        ref = oracle.aggregate_pose(pose, energy, clustering=c)
        assert np.abs(agg.cpu().numpy() - ref).max() < 1e-5, c


def test_rank_aggregate_edge_cases():
    from genpose2_amd import aggregate
    from oracle import oracle
    rng = np.random.default_rng(7)
    pose = _clustered_candidates(rng, 4, 3, modes=1)
    energy = rng.normal(size=(4, 3, 2)).astype(np.float32)
    tp, te = torch.from_numpy(pose).to(DEV), torch.from_numpy(energy).to(DEV)
    # retain one candidate
    agg = aggregate.aggregate_pose(tp, te, retain_ratio=0.34, clustering=0)
    ref = oracle.aggregate_pose(pose, energy, retain_ratio=0.34, clustering=0)
    assert np.abs(agg.cpu().numpy() - ref).max() < 1e-5
    # eps so small that DBSCAN labels everything noise with min_samples 2 -> plain average
    pose = _clustered_candidates(rng, 8, 50, modes=4, spread=0.2)
    energy = rng.normal(size=(8, 50, 2)).astype(np.float32)
    tp, te = torch.from_numpy(pose).to(DEV), torch.from_numpy(energy).to(DEV)
    for eps, mp in ((1e-6, 0.1), (0.05, 0.9), (10.0, 0.1)):
        agg = aggregate.aggregate_pose(tp, te, clustering_eps=eps, clustering_minpts=mp)
        ref = oracle.aggregate_pose(pose, energy, clustering_eps=eps, clustering_minpts=mp)
        assert np.abs(agg.cpu().numpy() - ref).max() < 1e-5, (eps, mp)
    # empty batch and invalid arguments fail with a status, not a crash
    e = aggregate.aggregate_pose(tp[:0], te[:0])
    assert e.shape == (0, 4, 4)
    from genpose2_amd._lib import GenPoseHipError
    with pytest.raises((GenPoseHipError, ValueError)):
        aggregate.aggregate_pose(tp, te, retain_ratio=0.0)
    with pytest.raises(GenPoseHipError):
        aggregate.aggregate_pose(_t(np.zeros((1, 2000, 9))), _t(np.zeros((1, 2000, 2))))


def test_rank_with_nan_and_inf_energies():
    """NaN / +-inf energies: the device ranks form a permutation in torch.sort(descending=True) order
    (NaN first, ties by index) and the aggregation stays finite (NaN ranks used to leave
    unwritten order slots)."""
    from genpose2_amd import aggregate
    rng = np.random.default_rng(11)
    B, K = 6, 50
    pose = _clustered_candidates(rng, B, K)
    energy = np.round(rng.normal(size=(B, K, 2)), 1).astype(np.float32)
    for b in range(B):
        idx = rng.choice(K, size=10, replace=False)
        energy[b, idx[:4], 0] = np.nan
        energy[b, idx[4:6], 1] = np.nan
        energy[b, idx[6], 0], energy[b, idx[7], 1] = np.inf, -np.inf
        energy[b, idx[8:], :] = np.nan
    energy[0, :, :] = np.nan                       # an object with no finite energy at all
    tp, te = torch.from_numpy(pose).to(DEV), torch.from_numpy(energy).to(DEV)
    sp, se = aggregate.sort_poses_by_energy(tp, te)
    rsp, rse, _, _ = oracle.sort_poses_by_energy(pose, energy)
    np.testing.assert_array_equal(sp.cpu().numpy(), rsp)
    np.testing.assert_array_equal(se.cpu().numpy(), rse)             # NaN == NaN positions
    for c in (0, 1):
        agg = aggregate.aggregate_pose(tp, te, clustering=c)
        ref = oracle.aggregate_pose(pose, energy, clustering=c)
        assert torch.isfinite(agg).all()
        assert np.abs(agg.cpu().numpy() - ref).max() < 1e-5, c


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(DEV)


# ---------------------------------------------------------------- device noise
def test_randn_matches_philox_restatement():
    from genpose2_amd import device
    from oracle import oracle
    for seed, stream, rows, cols in [(1234, 0, 5000, 9), (2**40 + 7, 17, 999, 13), (0, 5, 3, 1)]:
        got = device.randn(seed, stream, rows, cols, DEV).cpu().numpy().astype(np.float64)
        ref = oracle.randn(seed, stream, rows, cols)
        # hardware log2 / sin / cos / sqrt in the Box-Muller transform: a few ulp, not bit-exact
        assert np.abs(got - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), (seed, stream)
    z = device.randn(99, 1, 1 << 18, 9, DEV).double()
    assert abs(z.mean().item()) < 5e-3 and abs(z.std().item() - 1) < 5e-3
    assert abs(((z ** 4).mean() / (z ** 2).mean() ** 2).item() - 3) < 0.05   # Gaussian kurtosis


@pytest.mark.parametrize("B,K", [(4, 8), (90, 50), (164, 50)])
def test_pc_philox_equals_injected_draws(score_agent, B, K):
    """The in-kernel draws are exactly gp_randn's streams 2j / 2j+1: feeding those as injected
    noise reproduces the Philox run bit for bit (so the injected-noise parity tests cover it).
    32 rows (16-candidate tiles), 4500 rows (32-candidate tiles, ragged last tile) and 8200 rows
    (64-candidate tiles, 8 rows in the last one)."""
    from genpose2_amd import device, sde
    T, seed = 10, 77
    R = B * K
    heads = score_agent.heads
    tab = sde.pc_step_table(T)
    tproj = heads.time_proj(torch.from_numpy(tab[:, 0]).to(DEV))
    pobj = heads.object_proj(torch.rand(B, 1024, device=DEV))
    center = torch.rand(B, 3, device=DEV)
    x0 = torch.randn(R, 9, device=DEV) * 50
    res_p, q_p, xs_p = heads.pc_sample(pobj, tproj, tab, x0.clone(), K, center, seed=seed, want_xs=True)
    z1 = torch.stack([device.randn(seed, 2 * j, R, 9, DEV) for j in range(T)])
    z2 = torch.stack([device.randn(seed, 2 * j + 1, R, 9, DEV) for j in range(T)])
    res_i, q_i, xs_i = heads.pc_sample(pobj, tproj, tab, x0.clone(), K, center, z1=z1, z2=z2, want_xs=True)
    assert torch.equal(res_p, res_i) and torch.equal(q_p, q_i) and torch.equal(xs_p, xs_i)


# ---------------------------------------------------------------- stage hand-off
@pytest.mark.parametrize("n,c", [(1024, 3), (1000, 6), (2048, 3)])
def test_points_mean_and_bbox_length_vs_oracle(n, c):
    from genpose2_amd import device as dev
    rng = np.random.default_rng(n + c)
    B = 5
    pcl = (rng.normal(size=(B, n, c)) * 0.05 + 0.3).astype(np.float32)
    center = dev.points_mean(torch.from_numpy(pcl).to(DEV)).cpu().numpy()
    assert rel(center, oracle.points_mean(pcl)) < 1e-6
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    pose = np.zeros((B, 4, 4), np.float32)
    pose[:, :3, :3] = oracle.quaternion_to_matrix(q.astype(np.float32))
    pose[:, :3, 3] = center
    pose[:, 3, 3] = 1
    length = dev.bbox_length(torch.from_numpy(pcl).to(DEV), torch.from_numpy(pose).to(DEV)).cpu().numpy()
    assert rel(length, oracle.bbox_length(pcl, pose)) < 1e-6


def _loader(seed, nb, B, N):
    from genpose2_amd import synthetic
    out = []
    for i in range(nb):
        pts, _ = synthetic.make_batch(seed + i, B, N)
        out.append({"pcl_in": torch.from_numpy(pts), "sym_info": torch.zeros(B, 4),
                    "rotation": torch.eye(3).expand(B, 3, 3).clone(), "translation": torch.zeros(B, 3)})
    return out


def test_stage_files_match_reference_format(tmp_path):
    """inference_score -> inference_energy -> aggregate_pose -> inference_scale through pickle files
    in the reference's formats (evaluation_single.py:120,157,219,254,288), against the in-memory
    calls on the same batches."""
    import pickle
    from genpose2_amd import aggregate, runner
    from genpose2_amd.config import GenPoseConfig
    cfg = GenPoseConfig(device=DEV, sampling_steps=20, eval_repeat_num=20, T0=1.0)
    loader = _loader(300, 2, 3, 1024)
    sp, ep, ap, fp = (str(tmp_path / f) for f in ("score.pkl", "energy.pkl", "agg.pkl", "final.pkl"))
    runner.inference_score(cfg, loader, sp)
    runner.inference_energy(cfg, loader, sp, ep)
    runner.aggregate_pose(cfg, sp, ep, ap)
    runner.inference_scale(cfg, loader, sp, ap, fp)
    with open(sp, "rb") as f:
        poses, feats = pickle.load(f)
    with open(ep, "rb") as f:
        energies = pickle.load(f)
    with open(ap, "rb") as f:
        aggs = pickle.load(f)
    with open(fp, "rb") as f:
        finals, lengths = pickle.load(f)
    assert len(poses) == len(feats) == len(energies) == len(aggs) == len(finals) == len(lengths) == 2
    for i, batch in enumerate(loader):
        assert poses[i].shape == (3, 20, 9) and poses[i].is_cuda and poses[i].dtype == torch.float32
        assert set(feats[i]) == {"pts_feat", "rgb_feat"} and feats[i]["rgb_feat"] is None
        assert feats[i]["pts_feat"].shape == (3, 1024) and not feats[i]["pts_feat"].is_cuda
        assert energies[i].shape == (3, 20, 2) and not energies[i].is_cuda
        agg = aggregate.aggregate_pose(poses[i], energies[i].to(DEV), cfg.retain_ratio, cfg.clustering,
                                       cfg.clustering_eps, cfg.clustering_minpts).cpu()
        assert aggs[i].shape == (3, 4, 4) and torch.equal(aggs[i], agg)
        assert torch.equal(finals[i], aggs[i])                       # no ScaleNet: aggregated poses
        ref_len = oracle.bbox_length(batch["pcl_in"].numpy(), aggs[i].numpy())
        assert rel(lengths[i].numpy(), ref_len) < 1e-6
        # pts_center of process_batch == mean of the points
        pb = runner.process_batch(batch, DEV)
        assert rel(pb["pts_center"].cpu().numpy(), oracle.points_mean(batch["pcl_in"].numpy())) < 1e-6
        assert pb["gt_pose"].shape == (3, 9)


def test_stage_scale_with_scalenet(tmp_path):
    """inference_scale with a ScaleNet agent: final rotation = pred_scale_func's axes, lengths (B,3)."""
    import pickle
    from genpose2_amd import runner
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    cfg = GenPoseConfig(device=DEV, sampling_steps=20, eval_repeat_num=20, T0=1.0)
    loader = _loader(310, 1, 2, 1024)
    sp, ap, fp = (str(tmp_path / f) for f in ("score.pkl", "agg.pkl", "final.pkl"))
    runner.inference_score(cfg, loader, sp)
    runner.aggregate_pose(cfg, sp, None, ap)
    scale = PoseNet(cfg.copy(agent_type="scale")).eval()
    runner.inference_scale(cfg, loader, sp, ap, fp, agent=scale)
    with open(ap, "rb") as f:
        aggs = pickle.load(f)
    with open(sp, "rb") as f:
        _, feats = pickle.load(f)
    with open(fp, "rb") as f:
        finals, lengths = pickle.load(f)
    _, ref = scale.pred_scale_func({"pts_feat": feats[0]["pts_feat"].to(DEV),
                                    "axes": aggs[0][:, :3, :3].to(DEV).contiguous()})
    assert torch.equal(lengths[0], ref.cpu()) and lengths[0].shape == (2, 3)
    assert torch.equal(finals[0][:, :3, 3], aggs[0][:, :3, 3])


def test_sharded_pipeline_single_rank_equals_pipeline():
    """ShardedEvaluationPipeline on a one-rank RCCL group (the 8-GPU path's code: weight broadcast,
    shard, all_gather) returns exactly what EvaluationPipeline returns for the same batch and seeds."""
    import os
    import torch.distributed as dist
    from genpose2_amd import synthetic
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.runner import EvaluationPipeline, ShardedEvaluationPipeline
    pts, center = synthetic.make_batch(8, 6, 1024)
    batch = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    cfg = GenPoseConfig(device=DEV, sampling_steps=20, eval_repeat_num=20, noise_seed=4)
    ref = EvaluationPipeline(cfg, with_scale=True).run(dict(batch))
    port = 29400 + os.getpid() % 500
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(DEV))
    try:
        got = ShardedEvaluationPipeline(cfg, with_scale=True).run(dict(batch))
    finally:
        dist.destroy_process_group()
    for k in ("pred_pose", "pts_feat", "energy", "aggregated", "length"):
        assert torch.equal(getattr(got, k), getattr(ref, k)), k


def test_pred_func_with_precomputed_features():
    """pred_func(extract_feature=False) on data["pts_feat"] from encode_func (encoded on a side
    stream, as bench.py --pipeline does) equals the encode-inside call bit for bit."""
    from genpose2_amd import synthetic
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    pts, center = synthetic.make_batch(3, 4, 1024)
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    cfg = GenPoseConfig(device=DEV, sampling_steps=10, noise_seed=3)
    ref, _ = PoseNet(cfg).eval().pred_func(dict(data), repeat_num=8)
    agent = PoseNet(cfg).eval()
    d2 = dict(data)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        agent.encode_func(d2)
    torch.cuda.current_stream().wait_stream(side)
    got, _ = agent.pred_func(d2, repeat_num=8, extract_feature=False)
    assert torch.equal(got, ref)
    with pytest.raises(Exception):
        agent.pred_func(dict(data), repeat_num=8, extract_feature=False)   # no pts_feat given


def test_global_batch_ode_one_rank_equals_plain_and_exchange_failure(monkeypatch):
    """The global-batch ODE path (GlobalDeviceRk45, gp_ode_auto_attempt_global) on a one-rank gloo group: the
    exchange after every attempt has nothing to gather, so the solve equals the plain device-controlled one bit
    for bit (the same tiling, partials and decisions); an exchange that fails ends the solve with an error."""
    import torch.distributed as dist
    from genpose2_amd import shard, synthetic
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    B, K = 6, 24
    pts, center = synthetic.make_batch(8, B, 1024)
    data = lambda: {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}  # noqa
    cfg = GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None, T0=0.55, seed=3)
    ref_agent = PoseNet(cfg).eval()
    ref, _ = ref_agent.pred_func(data(), K, T0=0.55)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{29100 + os.getpid() % 90}", rank=0, world_size=1)
    try:
        agent = PoseNet(cfg).eval()
        agent.global_batch = shard.GlobalBatch.of(B)
        got, _ = agent.pred_func(data(), K, T0=0.55)
        assert torch.equal(got, ref) and agent.last_nfev == ref_agent.last_nfev

        def failing(self, ctx, attempt, slot_ptr, n, stream):
            if attempt == 2:
                self.error = RuntimeError("injected exchange failure")
                return -1
            return 0
        monkeypatch.setattr(shard.PartialsExchange, "_call", failing)
        with pytest.raises(RuntimeError, match="exchange failed"):
            agent.pred_func(data(), K, T0=0.55)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
