"""DINOv3 backbone without a device: the key table, the synthetic generator, pack_dino's folding, the torch
restatement (tests/dino_ref.py) against its fixtures and against transformers, C-level argument validation.
No HIP compute calls."""
import ctypes

import numpy as np
import pytest
import torch

import dino_inputs as di
import dino_ref

from genpose2_amd import arch, weights

NEW = ("gp_dino_workspace_size", "gp_dino_rope_table", "gp_dino_forward")


@pytest.fixture(scope="module")
def dino_sd():
    return weights.synthetic_state_dict("dino", di.WEIGHT_SEED)


def _lib():
    from genpose2_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ key table, generator, check_keys
def test_key_table_and_synthetic_state_dict(dino_sd):
    man = weights.manifest("dino")
    keys = [k for k, _, _ in man]
    assert len(keys) == len(set(keys)) == len(weights.DINO_TOP_KEYS) + 12 * len(weights.DINO_BLOCK_KEYS)
    assert set(dino_sd) == set(keys)
    for k, shape, _ in man:
        assert dino_sd[k].shape == tuple(shape) and dino_sd[k].dtype == np.float32, k
    # the issue's original key names
    for k in ("cls_token", "storage_tokens", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias",
              "rope_embed.periods", "norm.weight", "norm.bias", "blocks.0.norm1.weight", "blocks.11.attn.qkv.weight",
              "blocks.3.attn.qkv.bias", "blocks.3.attn.qkv.bias_mask", "blocks.5.attn.proj.bias", "blocks.7.ls1.gamma",
              "blocks.7.norm2.bias", "blocks.9.mlp.w1.weight", "blocks.9.mlp.w2.bias", "blocks.9.mlp.w3.weight",
              "blocks.11.ls2.gamma"):
        assert k in dino_sd, k
    assert weights.dino_key("gate_w", 4) == "blocks.4.mlp.w1.weight" and weights.dino_key("up_w", 4) == "blocks.4.mlp.w2.weight"
    assert weights.dino_key("down_w", 4) == "blocks.4.mlp.w3.weight"
    assert dino_sd["blocks.0.mlp.w3.weight"].shape == (384, 1536)
    # what makes attention position-sensitive
    w = dino_sd["blocks.2.attn.qkv.weight"]
    assert abs(w.std() * np.sqrt(384) - 1) < 0.02
    ls = dino_sd["blocks.2.ls1.gamma"]
    assert ls.min() >= 0.5 and ls.max() <= 1.5
    assert abs(dino_sd["blocks.2.norm1.weight"].mean() - 1) < 0.05
    kb = dino_sd["blocks.2.attn.qkv.bias"][384:768]
    assert np.all(kb != 0) and np.abs(kb).mean() > 0.1
    mask = dino_sd["blocks.2.attn.qkv.bias_mask"]
    assert np.all(mask[:384] == 1) and np.all(mask[384:768] == 0) and np.all(mask[768:] == 1)
    assert np.all(dino_sd["cls_token"] != 0) and np.all(dino_sd["storage_tokens"] != 0)
    per = dino_sd["rope_embed.periods"]
    assert np.array_equal(per, weights.round_bf16(per)) and per[0] == 1 and abs(per[4] - 100 ** 0.25) < 0.02
    # deterministic
    again = weights.synthetic_state_dict("dino", di.WEIGHT_SEED)
    assert all(np.array_equal(again[k], dino_sd[k]) for k in dino_sd)
    assert not np.array_equal(weights.synthetic_state_dict("dino", di.WEIGHT_SEED + 1)["cls_token"], dino_sd["cls_token"])


def test_check_keys(dino_sd):
    weights.check_keys(dino_sd, "dino")
    sd = dict(dino_sd)
    for k in weights.dino_optional_keys():      # the mask, the periods and the unused mask token may be absent
        sd.pop(k)
    weights.check_keys(sd, "dino")
    with pytest.raises(RuntimeError, match="missing"):
        weights.check_keys({k: v for k, v in dino_sd.items() if k != "blocks.4.ls2.gamma"}, "dino")
    with pytest.raises(RuntimeError, match="unexpected"):
        weights.check_keys(dict(dino_sd, extra=np.zeros(1)), "dino")
    with pytest.raises(RuntimeError, match="size mismatch"):
        weights.check_keys(dict(dino_sd, **{"norm.weight": np.zeros(383, np.float32)}), "dino")
    rest, dino = weights.split_dino({"dino." + k: v for k, v in dino_sd.items()} | {"a.b": np.zeros(1)})
    assert set(rest) == {"a.b"} and set(dino) == set(dino_sd)


def test_round_bf16():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, 3.1622777, -100.0], np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(weights.round_bf16(x), want)


# ------------------------------------------------------------------ packing
def test_pack_dino_folding(dino_sd):
    from genpose2_amd import dino
    from genpose2_amd.fus_encoder import pack_split_linear
    p = dino.pack_dino(dino_sd)
    f64 = lambda k: dino_sd[k].astype(np.float64)  # noqa: E731
    i, rng = 5, np.random.default_rng(0)
    x = rng.standard_normal((7, 384))
    # proj and w3 with LayerScale folded = the unfolded formula
    want = f64(f"blocks.{i}.ls1.gamma") * (x @ f64(f"blocks.{i}.attn.proj.weight").T + f64(f"blocks.{i}.attn.proj.bias"))
    got = x @ p[f"b{i}.proj.w"].astype(np.float64).T + p[f"b{i}.proj.b"]
    assert np.abs(got - want).max() < 1e-5
    hx = rng.standard_normal((7, 1536))
    want = f64(f"blocks.{i}.ls2.gamma") * (hx @ f64(f"blocks.{i}.mlp.w3.weight").T + f64(f"blocks.{i}.mlp.w3.bias"))
    got = hx @ p[f"b{i}.w3.w"].astype(np.float64).T + p[f"b{i}.w3.b"]
    assert np.abs(got - want).max() < 2e-5
    # folding happens in float64 and rounds once
    ls1 = f64(f"blocks.{i}.ls1.gamma")
    assert np.array_equal(p[f"b{i}.proj.w"], (ls1[:, None] * f64(f"blocks.{i}.attn.proj.weight")).astype(np.float32))
    # the masked bias: q and v kept, k zero
    qb = p[f"b{i}.qkv.b"]
    assert np.array_equal(qb[:384], dino_sd[f"blocks.{i}.attn.qkv.bias"][:384]) and np.all(qb[384:768] == 0)
    assert np.array_equal(qb[768:], dino_sd[f"blocks.{i}.attn.qkv.bias"][768:])
    # gate | up interleaved in 16-row tiles: the SwiGLU of the interleaved product = the plain formula
    z = x @ p[f"b{i}.w12.w"].astype(np.float64).T + p[f"b{i}.w12.b"]
    z = z.reshape(7, 96, 2, 16)
    gate, up = z[:, :, 0].reshape(7, 1536), z[:, :, 1].reshape(7, 1536)
    wg = x @ f64(f"blocks.{i}.mlp.w1.weight").T + f64(f"blocks.{i}.mlp.w1.bias")
    wu = x @ f64(f"blocks.{i}.mlp.w2.weight").T + f64(f"blocks.{i}.mlp.w2.bias")
    assert np.array_equal(gate, wg) and np.array_equal(up, wu)
    # split planes are pack_split_linear of the folded fp32 matrix
    assert np.array_equal(p[f"b{i}.w3.wh"], pack_split_linear(p[f"b{i}.w3.w"]))
    assert p[f"b{i}.w12.wh"].size == 4 + 3072 * 384
    assert np.array_equal(p["rope_periods"], dino_sd["rope_embed.periods"])
    # without a mask the bias is used as stored; without periods none are packed
    sd = {k: v for k, v in dino_sd.items() if not k.endswith("bias_mask") and k != "rope_embed.periods"}
    p2 = dino.pack_dino(sd)
    assert np.array_equal(p2[f"b{i}.qkv.b"], dino_sd[f"blocks.{i}.attn.qkv.bias"]) and "rope_periods" not in p2
    bad = dict(dino_sd)
    bad["blocks.1.attn.qkv.bias_mask"] = np.full(1152, np.nan, np.float32)
    with pytest.raises(ValueError, match="not finite"):
        dino.pack_dino(bad)


# ------------------------------------------------------------------ the restatement and its fixtures
@pytest.mark.parametrize("name", ["a", "b"])
def test_dino_ref_fp32_reproduces_fixture(dino_sd, name):
    g = di.load_case(name)
    b, h, w, _ = di.CASES[name]
    torch.manual_seed(0)
    with torch.no_grad():
        out = [o.numpy() for o in dino_ref.forward(dino_sd, g["x"], di.LAYERS, torch.float32)]
    for o, r32, r64 in zip(out, g["ref32"], g["ref64"]):
        assert o.shape == (b, (h // 16) * (w // 16), 384) == r64.shape
        # the same float32 program up to the BLAS's summation order: well inside the float32 run's own error
        assert np.abs(o - r32).max() <= 2 * np.abs(r32 - r64).max()
        assert np.abs(o - r64).max() <= 2 * np.abs(r32 - r64).max()


def test_fixture_c_layout():
    g = di.load_case("c")
    assert [r.shape for r in g["ref64"]] == [(1, 256, 384)] * 3 and g["ref64"][0].dtype == np.float64
    assert g["stats32"].shape == (3, 3) and np.all(g["stats32"] > 0) and np.all(g["stats32"][:, 0] < 1e-5)
    f = np.load(di.fixture_paths("c")[0])
    recorded = sorted(k[len("ratio_"):] for k in f.files if k.startswith("ratio_"))
    assert recorded == ["no_mask", "no_rope", "rope_prefix", "swap_hw"]   # the variants dino_ref had at that time
    for v in recorded:                # every switched-off variant was visible when the fixture was made
        assert v in dino_ref.VARIANTS and float(f[f"ratio_{v}"]) >= 100.0


def test_variants_move_the_output(dino_sd):
    g = di.load_case("a")
    emax = max(np.abs(a - b).max() for a, b in zip(g["ref32"], g["ref64"]))
    with torch.no_grad():
        for v in dino_ref.VARIANTS:
            out = dino_ref.forward(dino_sd, g["x"], (2,), torch.float64, variant=v)[0].numpy()
            assert np.abs(out - g["ref64"][0]).max() >= 100 * emax, v


def test_transformers_cross_check(dino_sd):
    pytest.importorskip("transformers")
    out_diff, tab_diff = dino_ref.hf_cross_check(dino_sd, di.case_input("a"), di.LAYERS)
    assert out_diff <= 1e-10 and tab_diff <= 2e-6


# ------------------------------------------------------------------ C argument validation (nothing is launched)
def test_abi_and_argument_validation():
    from genpose2_amd import _lib as L
    lib = _lib()
    assert lib.gp_abi_version() == 7
    assert all(n in L.EXPORTED for n in NEW)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)

    def wts(hp=4, wp=6, **null):
        w = L.DinoWeights()
        for name, _ in L.DinoWeights._fields_[:7]:
            setattr(w, name, None if name in null else p.value)
        w.rope_hp, w.rope_wp = hp, wp
        for blk in w.blocks:
            for name, _ in L.DinoBlock._fields_:
                setattr(blk, name, p.value)
        return w

    size = lib.gp_dino_workspace_size
    n29 = 29
    per_row = 384 * 4 + 1152 + 1536 + 3072          # h, y, att, r | qkv | g | u
    assert size(1, 64, 96) >= 4 * n29 * per_row and size(1, 64, 96) % 256 == 0
    assert size(3, 64, 96) > size(1, 64, 96)
    assert size(256, 256, 256) == size(83, 256, 256) < 1 << 30      # chunked: bounded in b (21760 // 261 images)
    assert size(82, 256, 256) < size(83, 256, 256)
    assert size(0, 64, 96) == 0 and size(1, 60, 96) == 0 and size(1, 16 * 33, 16 * 32) == 0

    lay = (ctypes.c_int * 3)(2, 6, 11)
    outs = (ctypes.c_void_p * 3)(p.value, p.value, p.value)

    def fwd(w=None, rgb=p, b=3, h=64, wd=96, n_out=3, layers=lay, o=outs, arith=0, ws=p, wsb=1 << 40):
        w = wts() if w is None else w
        return lib.gp_dino_forward(ctypes.byref(w), rgb, b, h, wd, n_out, layers, o, arith, ws, wsb, None)

    assert fwd(h=60) == -1 and b"multiples of the patch size 16" in lib.gp_last_error()
    assert fwd(wd=100) == -1
    assert fwd(w=wts(33, 32), h=16 * 33, wd=16 * 32) == -1 and b"exceed 1024" in lib.gp_last_error()
    assert fwd(b=0) == -1 and b"b=0" in lib.gp_last_error()
    assert fwd(wsb=size(1, 64, 96) - 1) == -1 and b"workspace" in lib.gp_last_error()
    assert fwd(rgb=None) == -1 and b"null pointer" in lib.gp_last_error()
    assert fwd(ws=None) == -1 and b"null pointer" in lib.gp_last_error()
    assert fwd(w=wts(norm_w=1)) == -1 and b"null weight" in lib.gp_last_error()
    assert fwd(o=(ctypes.c_void_p * 3)(p.value, None, p.value)) == -1 and b"output 1" in lib.gp_last_error()
    assert fwd(w=wts(4, 4)) == -1 and b"RoPE table" in lib.gp_last_error()
    assert fwd(arith=2) == -1 and fwd(n_out=0) == -1 and fwd(n_out=13) == -1
    assert fwd(layers=(ctypes.c_int * 3)(2, 6, 12)) == -1 and b"layer 12" in lib.gp_last_error()
    assert lib.gp_dino_rope_table(None, 4, 6, None, None) == -1
    assert lib.gp_dino_rope_table(None, 33, 32, p, None) == -1
    bad = np.ones(16, np.float32)
    bad[3] = np.inf
    assert lib.gp_dino_rope_table(bad.ctypes.data_as(ctypes.c_void_p), 4, 6, p, None) == -1
    assert b"period 3" in lib.gp_last_error()
    # the split linear's new epilogues keep its argument rules
    i32 = np.zeros(8, np.int32).ctypes.data_as(ctypes.c_void_p)
    assert lib.gp_linear_split(p, 32, 1, 32, i32, p, 48, 5, p, 48, p, 0, None, None) == -1
    assert b"multiple of 32" in lib.gp_last_error()
    assert lib.gp_linear_split(p, 32, 1, 32, i32, p, 64, 5, p, 16, p, 0, None, None) == -1     # ldy < n / 2
    assert lib.gp_linear_split(p, 32, 1, 32, i32, p, 64, 6, p, 64, p, 0, None, None) == -1
    assert buf.sum() == 0


# ------------------------------------------------------------------ Python rules that need no device
def test_frame_size_rule():
    from genpose2_amd import frontend
    for s in (14, 56, 224, 16, 64, 256, 112):
        assert frontend.check_img_size(s) == s
    for s in (0, 8, 13, 15, 100, 250, -16):
        with pytest.raises(ValueError, match="multiple of 14 or of 16"):
            frontend.check_img_size(s)
    z = np.zeros((120, 160), np.uint8)
    K = dict(fx=100.0, fy=100.0, cx=80.0, cy=60.0, width=160, height=120)
    with pytest.raises(ValueError, match="HIP device"):       # the device check still comes first
        frontend.frame_objects(z.astype(np.float32), np.zeros((120, 160, 3), np.uint8), z, K, img_size=256, device="cpu")


def test_pointwise_size_check_and_default_config():
    from genpose2_amd import infer
    assert infer.default_config().dino == "none"
    assert infer.default_config(dino="pointwise").dino == "pointwise"
    infer.GenPose2.check_pointwise_size(256, 256)
    for hw in ((224, 224), (256, 240), (128, 128)):
        with pytest.raises(ValueError, match="img_size=256"):
            infer.GenPose2.check_pointwise_size(*hw)
    assert arch.DINO_BLOCKS == 12 and arch.DINO_HEADS * arch.DINO_HEAD_DIM == arch.DINO_DIM
