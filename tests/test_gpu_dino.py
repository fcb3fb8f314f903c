"""The DINOv3 ViT-S+/16 backbone on the device (genpose2_amd/dino.py, csrc/gp_dino.hip): parity with the float64
fixtures of tests/dino_ref.py, batch / chunk / layer-subset consistency, workspace bounds, and the --dino pointwise
wiring through PoseNet, EvaluationPipeline and GenPose2.inference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dino_inputs as di

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITHS = ("split_f16", "f32")
# The project's calibrated bar (large_noise.check_calibrated's factor, restated): the device's error against the
# float64 reference stays within FACTOR x the error of the float32 torch run of the same model against it, in
# max, 99.9th percentile and mean, per output layer.
FACTOR = 2.0
N_PTS = 512      # the fewest points the point encoder takes (gp_encoder_fps: 512 <= n <= 8192)


@functools.lru_cache(maxsize=None)
def dino_sd():
    from genpose2_amd import weights
    return weights.synthetic_state_dict("dino", di.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def backbone():
    from genpose2_amd.dino import DinoBackbone
    return DinoBackbone(dino_sd(), torch.device(DEV))


@functools.lru_cache(maxsize=None)
def case(name):
    return di.load_case(name)


def run(x, arith, n=di.LAYERS, bb=None):
    bb = backbone() if bb is None else bb
    bb.set_arith(arith)
    out = bb.get_intermediate_layers(torch.as_tensor(x).to(DEV), n=list(n), reshape=False, norm=True,
                                     return_class_token=False)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_backbone_matches_float64_fixture(name, arith):
    """Measured on MI355X, device error over the float32 torch run's error (range over layers and statistics):
    split_f16 0.79-1.00, f32 1.03-1.57 (worst: case (b) layer 6 max, 4.23e-6 against 2.70e-6); the table is in
    DESIGN.md "DINOv3 backbone"."""
    g = case(name)
    out = run(g["x"], arith)
    b, h, w, _ = di.CASES[name]
    failures = []
    for i, l in enumerate(di.LAYERS):
        got = out[i].cpu().numpy()
        assert got.shape == (b, (h // 16) * (w // 16), 384) and np.all(np.isfinite(got))
        st = di.error_stats(got, g["ref64"][i])
        for j, s in enumerate(di.STATS):
            bound = FACTOR * g["stats32"][i][j]
            print(f"dino case {name} {arith} layer {l} {s}: device {st[s]:.3e}  fp32 torch {g['stats32'][i][j]:.3e}  "
                  f"ratio {st[s] / g['stats32'][i][j]:.2f}")
            if not st[s] <= bound:
                failures.append((l, s, st[s], bound))
    assert not failures, failures


# ------------------------------------------------------------------ consistency
@pytest.mark.parametrize("arith", ARITHS)
def test_batch_chunks_and_layer_subsets_are_bit_identical(arith):
    from genpose2_amd import _lib
    x = case("a")["x"]
    bb = backbone()
    full = run(x, arith)
    # a batch of 3 = its three single-image runs
    for i in range(x.shape[0]):
        one = run(x[i:i + 1], arith)
        for a, b in zip(one, full):
            assert torch.equal(a[0], b[i])
    # chunks of one image (a workspace that holds one) = one chunk
    lib = _lib.load()
    bb.max_workspace_bytes = int(lib.gp_dino_workspace_size(1, 64, 96))
    try:
        chunked = run(x, arith)
        assert bb._ws.numel() == bb.max_workspace_bytes < int(lib.gp_dino_workspace_size(3, 64, 96))
    finally:
        bb.max_workspace_bytes = None
    for a, b in zip(chunked, full):
        assert torch.equal(a, b)
    # n = (2,) runs three blocks and gives the first output of n = (2, 6, 11); any order of layers
    only2 = run(x, arith, n=(2,))
    assert len(only2) == 1 and torch.equal(only2[0], full[0])
    rev = run(x, arith, n=(11, 2))
    assert torch.equal(rev[0], full[2]) and torch.equal(rev[1], full[0])


def test_workspace_is_not_touched_beyond_its_size():
    from genpose2_amd import _lib
    from genpose2_amd.dino import ARITH
    lib = _lib.load()
    bb = backbone()
    x = torch.as_tensor(case("a")["x"]).to(DEV)
    B, _, H, W = x.shape
    need, pad = int(lib.gp_dino_workspace_size(B, H, W)), 1 << 16
    for arith in ARITHS:
        want = run(x, arith)
        ws = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        outs = [torch.full((B * 24 * 384 + 2 * 256,), 7.0, dtype=torch.float32, device=DEV) for _ in di.LAYERS]
        wts = bb._weights(bb.rope_table(H // 16, W // 16), H // 16, W // 16)
        lay = (ctypes.c_int * 3)(*di.LAYERS)
        ptrs = (ctypes.c_void_p * 3)(*[o.data_ptr() + 256 * 4 for o in outs])
        rc = lib.gp_dino_forward(ctypes.byref(wts), x.data_ptr(), B, H, W, 3, lay, ptrs, ARITH[arith],
                                 ws.data_ptr() + pad, need, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.gp_last_error()
        assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + need:] == 0xA5).all())
        for o, w in zip(outs, want):
            assert bool((o[:256] == 7.0).all()) and bool((o[-256:] == 7.0).all())
            assert torch.equal(o[256:-256].view_as(w), w)


def test_other_arguments_raise():
    bb = backbone()
    x = torch.zeros((1, 3, 64, 96), device=DEV)
    for kw in (dict(reshape=True), dict(norm=False), dict(return_class_token=True), dict(n=4), dict(n=[12])):
        with pytest.raises(NotImplementedError):
            bb.get_intermediate_layers(x, **kw)
    with pytest.raises(ValueError):
        bb.get_intermediate_layers(torch.zeros((1, 3, 60, 96), device=DEV))
    with pytest.raises(ValueError):
        bb.get_intermediate_layers(torch.zeros((1, 3, 64, 96)))
    with pytest.raises(ValueError):
        bb.set_arith("bf16")


# ------------------------------------------------------------------ PoseNet wiring
def _pointwise_data(B, n_pts, seed):
    from genpose2_amd import synthetic
    pts, center = synthetic.make_batch(seed, B, n_pts)
    rng = np.random.default_rng(seed)
    return {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV),
            "roi_rgb": torch.from_numpy(rng.uniform(-2.1, 2.6, (B, 3, 256, 256)).astype(np.float32)).to(DEV),
            "roi_xs": torch.from_numpy(rng.integers(0, 256, (B, n_pts)).astype(np.int32)).to(DEV),
            "roi_ys": torch.from_numpy(rng.integers(0, 256, (B, n_pts)).astype(np.int32)).to(DEV)}


def test_posenet_runs_the_backbone_on_roi_rgb():
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.dino import DinoBackbone
    cfg = GenPoseConfig(device=DEV, dino="pointwise", sampling_steps=4, sampler_mode=["pc"], noise_seed=5)
    agent = PoseNet(cfg).eval()
    assert agent.dino is None                      # synthetic weights bring no backbone
    data = _pointwise_data(2, N_PTS, 31)
    with pytest.raises(KeyError, match="dino_layers"):
        agent.pred_func(dict(data), repeat_num=2)
    agent.load_dino({"dino." + k: v for k, v in dino_sd().items()})     # the checkpoint's prefix is accepted
    assert isinstance(agent.dino, DinoBackbone) and agent.dino.same_weights(backbone())
    agent.dino.set_arith(backbone().arith)

    def pred(d):
        agent._gen.manual_seed(cfg.noise_seed)
        agent._calls = 0
        pose, q = agent.pred_func(d, repeat_num=2)
        torch.cuda.synchronize()
        return pose, q

    calls = agent.dino.calls
    a = pred(dict(data))
    assert agent.dino.calls == calls + 1
    layers = agent.dino.get_intermediate_layers(data["roi_rgb"], n=[2, 6, 11], reshape=False, norm=True,
                                                return_class_token=False)
    assert [tuple(t.shape) for t in layers] == [(2, 256, 384)] * 3
    b = pred(dict({k: v for k, v in data.items() if k != "roi_rgb"}, dino_layers=layers))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[0]).all())
    other = dict(data, roi_rgb=data["roi_rgb"].flip(-1).contiguous())    # the image matters
    assert not torch.equal(pred(other)[0], a[0])


def test_load_ckpt_builds_the_backbone_from_dino_keys(tmp_path):
    from genpose2_amd import weights
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    sd = {k: torch.from_numpy(v) for k, v in weights.synthetic_state_dict("score_pointwise", seed=1).items()}
    sd.update({"dino." + k: torch.from_numpy(v) for k, v in dino_sd().items()})
    path = str(tmp_path / "score_pointwise.pth")
    torch.save({"model_state_dict": sd}, path)
    agent = PoseNet(GenPoseConfig(device=DEV, dino="pointwise")).eval()
    agent.load_ckpt(model_dir=path, model_path=True, load_model_only=True)
    assert agent.dino is not None and agent.dino.same_weights(backbone())
    assert not any(k.startswith("dino.") for k in agent.state_dict)


# ------------------------------------------------------------------ end to end: a frame through GenPose2
def _frame():
    rng = np.random.default_rng(77)
    H, W = 120, 160
    depth = (0.8 + 0.004 * np.arange(W)[None, :] + 0.002 * np.arange(H)[:, None]).astype(np.float32)
    color = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask = np.full((H, W), 255, np.uint8)
    mask[40:70, 50:80] = 3
    mask[20:40, 100:125] = 7
    intr = dict(fx=411.3, fy=409.7, cx=158.6, cy=121.2, width=320, height=240)
    return {"depth": depth, "color": color, "mask": mask, "meta": intr}


def test_genpose2_inference_pointwise_from_a_frame():
    from genpose2_amd.frontend import InferDataset
    from genpose2_amd.infer import GenPose2, default_config
    cfg = default_config(dino="pointwise", device=DEV, sampling_steps=5, eval_repeat_num=20, noise_seed=3)   # K = 20: the
    # fewest candidates whose retained share still gives DBSCAN a min_samples >= 1 at the default ratios
    gp = GenPose2(None, cfg=cfg)
    with pytest.raises(KeyError, match="dino_layers"):     # no backbone yet
        gp.inference(InferDataset(_frame(), img_size=256, device=DEV, n_pts=N_PTS))
    gp.score_agent.load_dino(dino_sd())
    gp.energy_agent.load_dino(dino_sd())                   # a second, byte-identical backbone
    sb, eb = gp.score_agent.dino, gp.energy_agent.dino
    assert sb is not eb

    def reset():
        torch.manual_seed(21)
        for a in (gp.score_agent, gp.energy_agent):
            a._gen.manual_seed(cfg.noise_seed)
            a._calls = 0

    ds = InferDataset(_frame(), img_size=256, device=DEV, n_pts=N_PTS)
    reset()
    pose, length = gp.inference(ds)
    torch.cuda.synchronize()
    assert tuple(pose.shape) == (2, 4, 4) and tuple(length.shape) == (2, 3) and bool(torch.isfinite(pose).all())
    assert (sb.calls, eb.calls) == (1, 0)                  # once per frame, for both agents
    # the same poses as the pipeline on the same batch with the layers precomputed
    batch = ds.get_objects()
    assert tuple(batch["roi_rgb"].shape) == (2, 3, 256, 256)
    layers = sb.get_intermediate_layers(batch["roi_rgb"], n=[2, 6, 11])
    reset()
    out = gp.pipeline.run(dict(batch, dino_layers=layers), T0=None, energy_T=None)
    torch.cuda.synchronize()
    assert torch.equal(out.aggregated, pose)
    assert (sb.calls, eb.calls) == (2, 0)                  # only the explicit call above
    # different backbones: each agent runs its own
    eb.t["cls"].add_(1.0)
    gp.pipeline._dino_same = None
    reset()
    gp.inference(ds)
    assert (sb.calls, eb.calls) == (3, 1)
    # 224 pixels give 14 x 14 patches: refused before anything is launched
    with pytest.raises(ValueError, match="img_size=256"):
        gp.inference(InferDataset(_frame(), img_size=224, device=DEV, n_pts=N_PTS))
    assert (sb.calls, eb.calls) == (3, 1)
