"""Pose hypotheses on the device: gp_rank_aggregate_modes against the reference-made fixture (golden_modes.npz) and
against the NumPy restatement (tests/modes_ref.py) at the shapes where the kernel takes another path, and the way up
to EvaluationPipeline.run and GenPose2.inference_modes / inference_frames_modes.

Every device call made through ``_device`` is also held to the bit identities: aggregated / sorted_pose /
sorted_energy equal gp_rank_aggregate's, slot 0's rotation equals aggregated's, one object run alone equals its rows
of the batched call, and the slots past the filled ones are zero.

Bounds. Integer outputs are exact. Rotation entries: 1e-5, the bar ``aggregated`` has against the reference (fp32
eigh there, fp64 Jacobi here). On the fixture the means are held to max(1e-6, 2 x the float32-float64 gap the generator
stored). At the other shapes, for a cluster of n members of magnitude <= X: an fp32 sum of n terms is off by at most
(n-1) u n X (u = 2^-24), its mean by (n-1) u X, and the device and the restatement each make one, so the mean bound is
max(1e-6, n 2^-23 X); the spread adds 2e-5, since d(1 - dot^2) = 2 dot d(dot) and the rotation bar admits mode
quaternions 1e-5 apart.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden

import modes_inputs as mi
import modes_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_OUTPUTS = ("mode_count", "n_clusters", "noise_count", "nearest")
FIELDS = ("aggregated", "mode_pose", "mode_count", "mode_energy", "mode_spread", "n_clusters", "noise_count",
          "nearest")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(pose, energy, keep, clustering, eps, min_samples, M, prev_rot):
    from genpose2_amd import aggregate
    modes, sp, se = aggregate._rank_aggregate_modes(pose, energy, keep, clustering, eps, min_samples, M, prev_rot, True)
    torch.cuda.synchronize()
    return modes, sp, se


def _device(pose, energy, keep, clustering, eps, min_samples, M, prev_rot=None):
    """One launch of the new entry -> numpy outputs, after the bit identities of this file's header."""
    from genpose2_amd import aggregate
    tp, te = _t(pose), _t(energy)
    tr = _t(prev_rot) if prev_rot is not None else None
    modes, sp, se = _call(tp, te, keep, clustering, eps, min_samples, M, tr)
    agg0, sp0, se0 = aggregate._rank_aggregate(tp, te, keep, clustering, eps, min_samples, True)
    B = pose.shape[0]
    assert torch.equal(modes.aggregated, agg0)
    assert torch.equal(sp, sp0)
    assert torch.equal(se.view(torch.int32), se0.view(torch.int32))               # NaN energies: compare the bits
    assert torch.equal(modes.mode_pose[:, 0, :3, :3], modes.aggregated[:, :3, :3])
    if B:
        j = B - 1 if B < 3 else B // 2
        alone, _, _ = _call(tp[j:j + 1], te[j:j + 1], keep, clustering, eps, min_samples, M,
                            tr[j:j + 1] if tr is not None else None)
        for f in FIELDS:
            assert torch.equal(getattr(alone, f)[0].contiguous().view(torch.int32),
                               getattr(modes, f)[j].contiguous().view(torch.int32)), f
    out = {f: getattr(modes, f).cpu().numpy() for f in FIELDS}
    filled = np.maximum(1, np.minimum(out["n_clusters"], M))
    for j in range(B):
        assert out["mode_count"][j, :filled[j]].min() >= 1
        for f in ("mode_pose", "mode_count", "mode_energy", "mode_spread"):
            assert not out[f][j, filled[j]:].any(), (j, f)                        # +0.0 and 0: no bit set
            assert not out[f][j, filled[j]:].view(np.int32).any(), (j, f)
        assert np.array_equal(out["mode_pose"][j, :filled[j], 3], np.tile([0, 0, 0, 1], (filled[j], 1)))
    out["filled"] = filled
    return out


def _against_ref(out, ref, pose, energy, keep, what=""):
    """Device outputs against the restatement, with the bounds of this file's header for arbitrary shapes."""
    assert ref["margin"].min() > 1e-4 and ref["nearest_gap"].min() > 1e-3, "ambiguous inputs: choose another seed"
    for f in INT_OUTPUTS:
        np.testing.assert_array_equal(out[f], ref[f], err_msg=f"{what} {f}")
    rot = np.abs(out["mode_pose"][:, :, :3, :3] - ref["mode_pose"][:, :, :3, :3]).max()
    tr = np.abs(out["mode_pose"][:, :, :3, 3] - ref["mode_pose"][:, :, :3, 3]).max()
    agg = np.abs(out["aggregated"] - ref["aggregated"]).max()
    finite = np.isfinite(ref["mode_energy"])
    np.testing.assert_array_equal(np.isnan(out["mode_energy"]), np.isnan(ref["mode_energy"]))
    np.testing.assert_array_equal(out["mode_energy"][~finite & ~np.isnan(ref["mode_energy"])],
                                  ref["mode_energy"][~finite & ~np.isnan(ref["mode_energy"])])   # +-inf
    en = np.abs(out["mode_energy"][finite] - ref["mode_energy"][finite]).max() if finite.any() else 0.0
    spr = np.abs(out["mode_spread"] - ref["mode_spread"]).max()
    u2 = keep * 2.0 ** -23
    e_fin = energy[..., 0][np.isfinite(energy[..., 0])]
    tol_t = max(1e-6, u2 * float(np.abs(pose[..., 6:]).max()))
    tol_e = max(1e-6, u2 * float(np.abs(e_fin).max())) if e_fin.size else 1e-6
    tol_s = 2e-5 + max(1e-6, u2)
    print(f"{what}: rot {rot:.2e} agg {agg:.2e} trans {tr:.2e}/{tol_t:.1e} energy {en:.2e}/{tol_e:.1e} "
          f"spread {spr:.2e}/{tol_s:.1e}")
    assert rot < 1e-5 and agg < 1e-5, what
    assert tr <= tol_t and en <= tol_e and spr <= tol_s, what


# ---------------------------------------------------------------------------- the reference-made fixture
@pytest.mark.parametrize("M", [4, 8])
def test_golden(M):
    g = golden("modes")
    tol_mean = max(1e-6, 2 * float(g["mean_gap"]))
    tol_spread = max(1e-6, 2 * float(g["spread_gap"]))
    for p in (0, 1):
        out = _device(g["pred_pose"], g["pred_energy"], mi.KEEP, 1, mi.EPS, mi.MIN_SAMPLES, M, g["prev_rot"][p])
        np.testing.assert_array_equal(out["n_clusters"], g["n_clusters"])
        np.testing.assert_array_equal(out["noise_count"], g["noise_count"])
        np.testing.assert_array_equal(out["mode_count"], g["mode_count"][:, :M])
        if M == 4:   # the fixture's nearest is that of max_modes = 4
            np.testing.assert_array_equal(out["nearest"], g["nearest"][p])
        else:        # more slots filled: the restatement's choice among them
            ref = modes_ref.modes_ref(g["pred_pose"], g["pred_energy"], mi.KEEP, 1, mi.EPS, mi.MIN_SAMPLES, M,
                                      g["prev_rot"][p])
            assert ref["nearest_gap"].min() > 1e-3
            np.testing.assert_array_equal(out["nearest"], ref["nearest"])
        rot = np.abs(out["mode_pose"][:, :, :3, :3] - g["mode_rot"][:, :M]).max()
        agg = np.abs(out["aggregated"] - g["aggregated"]).max()
        tr = np.abs(out["mode_pose"][:, :, :3, 3] - g["mode_trans_f32"][:, :M]).max()
        en = np.abs(out["mode_energy"] - g["mode_energy_f32"][:, :M]).max()
        spr = np.abs(out["mode_spread"] - g["mode_spread_f32"][:, :M]).max()
        print(f"golden M={M} prev {p}: rot {rot:.2e} agg {agg:.2e} trans {tr:.2e} energy {en:.2e} (<= {tol_mean:.2e}) "
              f"spread {spr:.2e} (<= {tol_spread:.2e})")
        assert rot < 1e-5 and agg < 1e-5
        assert tr <= tol_mean and en <= tol_mean
        assert spr <= tol_spread
    no_prev = _device(g["pred_pose"], g["pred_energy"], mi.KEEP, 1, mi.EPS, mi.MIN_SAMPLES, M)
    assert (no_prev["nearest"] == -1).all()
    for f in FIELDS[:-1]:   # prev_rot moves nothing but nearest
        np.testing.assert_array_equal(no_prev[f], out[f], err_msg=f)


# ---------------------------------------------------------------------------- other shapes, against the restatement
def _clustered_candidates(rng, B, K, modes=3, spread=0.02):
    """K candidates per object around `modes` random rotations (6D) + noise, random translations: the recipe of
    tests/test_gpu_parity.py's ranking tests."""
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


def _prev_near_slots(seed, ref):
    """A previous rotation per object, a few degrees off the restatement's slot (object index mod filled)."""
    B, M = ref["mode_count"].shape
    filled = np.maximum(1, np.minimum(ref["n_clusters"], M))
    return np.stack([mi.prev_rotation(seed + j, ref["mode_pose"][j, j % filled[j], :3, :3]) for j in range(B)])


def _case(seed, B, K, keep, clustering, eps, min_samples, M, modes=3, spread=0.02, energy=None, what=""):
    """modes = 0: every candidate a random rotation of its own."""
    rng = np.random.default_rng(seed)
    if modes:
        pose = _clustered_candidates(rng, B, K, modes, spread)
    else:
        pose = np.concatenate([rng.normal(size=(B, K, 6)), rng.normal(scale=0.3, size=(B, K, 3))], -1).astype(np.float32)
    energy = rng.normal(size=(B, K, 2)).astype(np.float32) if energy is None else energy
    prev = _prev_near_slots(seed, modes_ref.modes_ref(pose, energy, keep, clustering, eps, min_samples, M))
    ref = modes_ref.modes_ref(pose, energy, keep, clustering, eps, min_samples, M, prev)
    out = _device(pose, energy, keep, clustering, eps, min_samples, M, prev)
    _against_ref(out, ref, pose, energy, keep, what or f"B{B} K{K} keep{keep} M{M}")
    return out, ref


def test_keep_128_of_320():
    """The LDS limits (keep = 128): clusters at the shipped ratio, and every kept candidate a cluster of its own
    (min_samples 1, a tiny eps), so that the labels outnumber the workgroup's 64 lanes twice over."""
    out, _ = _case(5, 3, 320, 128, 1, 0.05, int(0.1667 * 128), 4)
    assert (out["n_clusters"] >= 1).all()
    out, _ = _case(6, 2, 320, 128, 1, 1e-4, 1, 8, modes=0)
    assert (out["n_clusters"] == 128).all() and (out["mode_count"] == 1).all() and not out["noise_count"].any()
    assert np.abs(out["mode_spread"]).max() < 1e-6          # a single member is its own mode


def test_keep_one_of_three():
    for clustering in (0, 1):
        out, _ = _case(7, 4, 3, 1, clustering, 0.05, 1, 4, modes=1)
        assert (out["mode_count"][:, 0] == 1).all() and (out["n_clusters"] == clustering).all()


def test_one_slot_and_eight_on_the_same_inputs():
    args = dict(B=8, K=50, keep=20, clustering=1, eps=0.05, min_samples=2, modes=6)
    one, _ = _case(8, M=1, **args)
    eight, ref = _case(8, M=8, **args)
    assert ref["n_clusters"].max() > 1                       # the cap at M = 1 is exercised
    for f in ("aggregated", "n_clusters", "noise_count"):
        np.testing.assert_array_equal(one[f], eight[f], err_msg=f)
    for f in ("mode_pose", "mode_count", "mode_energy", "mode_spread"):
        np.testing.assert_array_equal(one[f][:, 0], eight[f][:, 0], err_msg=f)
    assert (one["nearest"] == 0).all()


def test_without_clustering_all_noise_and_one_cluster():
    out, _ = _case(9, 8, 50, 20, 0, 0.05, 3, 4, modes=4, spread=0.2, what="clustering 0")
    assert not out["n_clusters"].any() and not out["noise_count"].any() and (out["mode_count"][:, 0] == 20).all()
    out, _ = _case(9, 8, 50, 20, 1, 1e-6, 2, 4, modes=4, spread=0.2, what="eps 1e-6")
    assert not out["n_clusters"].any() and (out["noise_count"] == 20).all() and (out["mode_count"][:, 0] == 20).all()
    out, _ = _case(9, 8, 50, 20, 1, 10.0, 2, 4, modes=4, spread=0.2, what="eps 10")
    assert (out["n_clusters"] == 1).all() and not out["noise_count"].any() and (out["mode_count"][:, 0] == 20).all()


def test_nan_and_inf_energies():
    """The energies of tests/test_gpu_parity.py::test_rank_with_nan_and_inf_energies: the ranks are still a
    permutation (sorted outputs equal the old entry's, which that test holds to torch.sort), the rotations stay
    finite, and a NaN among a cluster's energies makes that cluster's mean NaN."""
    rng = np.random.default_rng(11)
    B, K = 6, 50
    energy = np.round(rng.normal(size=(B, K, 2)), 1).astype(np.float32)
    for b in range(B):
        idx = rng.choice(K, size=10, replace=False)
        energy[b, idx[:4], 0] = np.nan
        energy[b, idx[4:6], 1] = np.nan
        energy[b, idx[6], 0], energy[b, idx[7], 1] = np.inf, -np.inf
        energy[b, idx[8:], :] = np.nan
    energy[0, :, :] = np.nan
    for clustering in (0, 1):
        out, _ = _case(12, B, K, 20, clustering, 0.05, 3, 4, energy=energy, what=f"nan energies c{clustering}")
        assert np.isfinite(out["mode_pose"]).all() and np.isfinite(out["aggregated"]).all()
        assert np.isfinite(out["mode_spread"]).all()
        assert np.isnan(out["mode_energy"][0, 0])


def test_empty_batch():
    from genpose2_amd import aggregate
    modes = aggregate.aggregate_modes(torch.zeros((0, 50, 9), device=DEV), torch.zeros((0, 50, 2), device=DEV))
    assert modes.aggregated.shape == (0, 4, 4) and modes.mode_pose.shape == (0, 4, 4, 4)
    assert modes.mode_count.shape == (0, 4) and modes.nearest.shape == (0,)
    from genpose2_amd._lib import GenPoseHipError
    tp, te = torch.zeros((2, 50, 9), device=DEV), torch.zeros((2, 50, 2), device=DEV)
    for m in (0, 9):
        with pytest.raises(GenPoseHipError, match="max_modes"):
            aggregate.aggregate_modes(tp, te, max_modes=m)
    with pytest.raises(ValueError, match="prev_rot"):
        aggregate.aggregate_modes(tp, te, prev_rot=torch.zeros((3, 3, 3), device=DEV))


def test_64_objects_of_50():
    out, ref = _case(64 * 50, 64, 50, 20, 1, 0.05, 3, 4)
    assert len(set(ref["n_clusters"].tolist())) > 1


# ---------------------------------------------------------------------------- pipeline and GenPose2
K_PIPE = 50


@functools.lru_cache(maxsize=None)
def _frames_batch():
    import frontend_frames_fixture as fx
    from genpose2_amd.frontend import frames_objects
    out = frames_objects(*fx.frames(), list(fx.CAMERAS), img_size=56, n_pts=1024, max_depth=4.0, seed=list(fx.SEEDS),
                         device=DEV)
    torch.cuda.synchronize()
    return out


def _cfg(**kw):
    from genpose2_amd.infer import default_config
    return default_config(device=DEV, sampling_steps=5, eval_repeat_num=K_PIPE, noise_seed=3, **kw)


def _same_modes(a, b):
    for f in FIELDS:
        x, y = getattr(a, f).contiguous(), getattr(b, f).contiguous()
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), f


def test_pipeline_run_with_and_without_modes():
    from genpose2_amd import aggregate, synthetic
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.runner import EvaluationPipeline
    pts, center = synthetic.make_batch(3, 4, 1024)
    batch = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    cfg = GenPoseConfig(device=DEV, sampling_steps=10, eval_repeat_num=K_PIPE)
    keep = int(K_PIPE * cfg.retain_ratio)

    def old_entry(out):   # the aggregation launch as it stands, on this run's own candidates
        return aggregate.aggregate_pose(out.pred_pose, out.energy, cfg.retain_ratio, cfg.clustering, cfg.clustering_eps,
                                        cfg.clustering_minpts, retain_num=keep)

    pipe = EvaluationPipeline(cfg, with_scale=True)
    out0 = pipe.run(batch)
    assert out0.modes is None and torch.equal(out0.aggregated, old_entry(out0))
    out0b = pipe.run(batch, max_modes=0)
    assert out0b.modes is None and torch.equal(out0b.aggregated, old_entry(out0b))
    out4 = pipe.run(batch, max_modes=4)
    assert out4.modes is not None and out4.modes.mode_pose.shape == (4, 4, 4, 4)
    assert torch.equal(out4.aggregated, old_entry(out4)) and torch.equal(out4.modes.aggregated, out4.aggregated)
    assert (out4.modes.nearest == -1).all() and torch.isfinite(out4.length).all()
    _, length = pipe.scale_agent.pred_scale_func({"pts_feat": out4.pts_feat, "rgb_feat": None,
                                                  "axes": out4.aggregated[:, :3, :3].contiguous()})
    assert torch.equal(out4.length, length)


def test_inference_modes_equals_inference():
    from genpose2_amd.infer import GenPose2
    b = _frames_batch()
    torch.manual_seed(21)
    pose, length = GenPose2(None, cfg=_cfg()).inference(b)
    torch.manual_seed(21)
    pose_m, length_m, modes = GenPose2(None, cfg=_cfg()).inference_modes(b)
    assert torch.equal(pose_m, pose) and torch.equal(length_m, length)
    assert torch.equal(modes.aggregated, pose) and modes.mode_pose.shape == (pose.shape[0], 4, 4, 4)
    assert torch.equal(modes.mode_pose[:, 0, :3, :3], pose[:, :3, :3]) and (modes.nearest == -1).all()


def _two_mode_genpose():
    """A GenPose2 whose sampler and energy stage hand out the fixture's object with two modes of 9 candidates each
    (the encoders still run), so that what follows the candidates can be checked on known hypotheses."""
    from genpose2_amd.infer import GenPose2
    g = golden("modes")
    j = [o[0] for o in mi.OBJECTS].index((9, 9))
    gp = GenPose2(None, cfg=_cfg())
    B = _frames_batch()["pts"].shape[0]
    cand, en = _t(g["pred_pose"][j]).repeat(B, 1, 1), _t(g["pred_energy"][j]).repeat(B, 1, 1)
    score = gp.score_agent

    def pred_func(data, repeat_num, **kw):
        score.encode_func(data)
        if score.after_encode is not None:
            score.after_encode()
        return cand, None

    score.pred_func = pred_func
    gp.energy_agent.get_energy = lambda **kw: en
    prev = [torch.eye(4).repeat(B, 1, 1) for _ in range(2)]
    for p in range(2):
        prev[p][:, :3, :3] = torch.from_numpy(g["prev_rot"][p][j])
        prev[p][:, :3, 3] = _frames_batch()["pts_center"].cpu()
    return gp, prev


def test_follow_prev_takes_the_mode_nearest_to_the_previous_pose():
    from genpose2_amd import device as dev
    gp, prev = _two_mode_genpose()
    b = _frames_batch()
    base, base_len = gp.inference(b)
    plain, plain_len, modes = gp.inference_modes(b, prev_pose=prev[1].to(DEV))
    assert torch.equal(plain, base) and torch.equal(plain_len, base_len)              # follow_prev is off
    assert (modes.mode_count[:, :2] == 9).all() and (modes.nearest == 1).all()
    second, second_len, m2 = gp.inference_modes(b, prev_pose=prev[1].to(DEV), follow_prev=True)
    _same_modes(m2, modes)
    assert torch.equal(second[:, :3, :3], modes.mode_pose[:, 1, :3, :3])
    assert not torch.equal(second[:, :3, :3], base[:, :3, :3])
    assert torch.equal(second[:, :, 3], base[:, :, 3]) and torch.equal(second[:, 3], base[:, 3])
    assert torch.equal(second_len, dev.bbox_length(b["pts"], second))                  # the size in that frame
    first, first_len, m1 = gp.inference_modes(b, prev_pose=prev[0].to(DEV), follow_prev=True)
    assert (m1.nearest == 0).all() and torch.equal(first, base) and torch.equal(first_len, base_len)
    # without a previous pose there is nothing to follow
    cold, cold_len, m0 = gp.inference_modes(b, follow_prev=True)
    assert (m0.nearest == -1).all() and torch.equal(cold, base) and torch.equal(cold_len, base_len)


def test_follow_prev_feeds_the_scale_network_the_followed_axes():
    from genpose2_amd.runner import EvaluationPipeline
    gp, prev = _two_mode_genpose()
    pipe = EvaluationPipeline(gp.cfg, with_scale=True)
    pipe.score_agent, pipe.energy_agent = gp.score_agent, gp.energy_agent      # the agents that hand out the fixture
    b = _frames_batch()
    out = pipe.run(b, energy_T=None, max_modes=4, prev_rot=prev[1][:, :3, :3].contiguous().to(DEV), follow_prev=True)
    assert torch.equal(out.aggregated[:, :3, :3], out.modes.mode_pose[:, 1, :3, :3])
    assert torch.equal(out.aggregated[:, :3, 3], out.modes.aggregated[:, :3, 3])
    _, length = pipe.scale_agent.pred_scale_func({"pts_feat": out.pts_feat, "rgb_feat": None,
                                                  "axes": out.modes.mode_pose[:, 1, :3, :3].contiguous()})
    assert torch.equal(out.length, length)
    _, other = pipe.scale_agent.pred_scale_func({"pts_feat": out.pts_feat, "rgb_feat": None,
                                                 "axes": out.modes.aggregated[:, :3, :3].contiguous()})
    assert not torch.equal(out.length, other)


def test_inference_frames_modes_equals_the_one_call_split():
    """The aggregation stage on identical candidates: the frames call is inference_modes on the same batch, split by
    frame_offsets, and each frame's hypotheses are those of its objects aggregated in a call of their own."""
    import frontend_frames_fixture as fx
    from genpose2_amd import aggregate
    from genpose2_amd.infer import GenPose2
    b = _frames_batch()
    prev = torch.eye(4).repeat(b["pts"].shape[0], 1, 1)
    prev[:, :3, 3] = b["pts_center"].cpu()
    split = [prev[lo:hi] for lo, hi in zip(fx.OFFSETS[:-1], fx.OFFSETS[1:])]
    torch.manual_seed(21)
    out = GenPose2(None, cfg=_cfg()).inference_frames_modes(b, prev_pose=split, tracking=True, follow_prev=True)
    torch.manual_seed(21)
    gp = GenPose2(None, cfg=_cfg())
    captured = {}
    run = gp.pipeline.run

    def recording_run(*a, **kw):
        captured["out"] = run(*a, **kw)
        return captured["out"]

    gp.pipeline.run = recording_run
    pose, length, modes = gp.inference_modes(b, prev_pose=prev.to(DEV), tracking=True, follow_prev=True)
    assert [tuple(o[0].shape) for o in out] == [(3, 4, 4), (0, 4, 4), (2, 4, 4)]
    assert torch.equal(torch.cat([o[0] for o in out]), pose) and torch.equal(torch.cat([o[1] for o in out]), length)
    stage = captured["out"]
    cfg = gp.cfg
    for f, (lo, hi) in enumerate(zip(fx.OFFSETS[:-1], fx.OFFSETS[1:])):
        _same_modes(out[f][2], modes.slice(lo, hi))
        own = aggregate.aggregate_modes(stage.pred_pose[lo:hi], stage.energy[lo:hi], cfg.retain_ratio, cfg.clustering,
                                        cfg.clustering_eps, cfg.clustering_minpts,
                                        retain_num=int(cfg.eval_repeat_num * cfg.retain_ratio), max_modes=4,
                                        prev_rot=prev[lo:hi, :3, :3].contiguous().to(DEV))
        _same_modes(out[f][2], own)
    # every frame empty: F triples of empty tensors, nothing run
    from genpose2_amd.frontend import frames_objects
    none = frames_objects(*fx.frames(objects=((), (), ())), fx.CAM_A, img_size=56, device=DEV)
    empty = gp.inference_frames_modes(none)
    assert [(tuple(p.shape), tuple(n.shape), tuple(m.mode_pose.shape)) for p, n, m in empty] == \
        [((0, 4, 4), (0, 3), (0, 4, 4, 4))] * 3
