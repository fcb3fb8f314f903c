"""Cases, seeds and inputs of the DINOv3 backbone's edge tests (test_cpu_dino_edge.py, test_gpu_dino_edge.py): shapes
at the tile boundaries of dino_attention_kernel (64-query tiles, 64-key chunks padded to 16-key tiles) and of
dino_patch_embed_kernel (64-row blocks), grids with Hp > Wp, and inputs that stress the softmax. Nothing is stored:
inputs come from seeds, and the float64 / float32 references are computed by tests/dino_ref.py when a test asks."""
from __future__ import annotations

import functools

import numpy as np

import dino_inputs as di

WEIGHT_SEED = di.WEIGHT_SEED
STATS = di.STATS
# 27,648: the values of one output of fixture (a), the smallest sample the 2 x bar was measured on
MIN_VALUES = 3 * 24 * 384
LAYERS = (0, 2, 11)
# name -> (B, H, W, input seed, output layers, input kind, weights kind)
#   input kind: "uniform" (-2.1 .. 2.6) | "const" (every pixel 0.7) | "big" (the uniform input x 100)
#   weights kind: "plain" | "sharp" (rows 0..383 of every attn.qkv.weight / .bias x 6: a peaked softmax)
CASES = {
    "one_patch":  (72, 16, 16, 201, LAYERS, "uniform", "plain"),   # 1 x 1 patches, 6 tokens; RoPE coordinate 0
    "strip_w":    (2, 16, 944, 202, LAYERS, "uniform", "plain"),   # 1 x 59, 64 tokens: one full query tile / chunk
    "strip_h":    (2, 960, 16, 203, LAYERS, "uniform", "plain"),   # 60 x 1, 65 tokens: second chunk / query tile hold 1
    "n128":       (2, 48, 656, 204, LAYERS, "uniform", "plain"),   # 3 x 41, 128 tokens: two full chunks
    "n129":       (2, 64, 496, 205, LAYERS, "uniform", "plain"),   # 4 x 31, 129 tokens: third chunk of 1 key
    "tall":       (3, 96, 64, 206, LAYERS, "uniform", "plain"),    # 6 x 4, 29 tokens: fixture (a) transposed
    "m64":        (5, 64, 64, 207, LAYERS, "uniform", "plain"),    # 4 x 4, 21 tokens: patch-embed m = 80 (B = 4: 64)
    "m129":       (3, 16, 688, 208, LAYERS, "uniform", "plain"),   # 1 x 43, 48 tokens: patch-embed m = 129
    "max":        (1, 512, 512, 209, (0, 2), "uniform", "plain"),  # 32 x 32, 1029 tokens: DN_MAX_PATCHES
    "n129_const": (2, 64, 496, 205, LAYERS, "const", "plain"),
    "n129_big":   (2, 64, 496, 205, LAYERS, "big", "plain"),
    "n129_sharp": (2, 64, 496, 205, LAYERS, "uniform", "sharp"),
}
# what each case is there for: tokens n = 5 + patches, n % 64, patch-embed rows m = B * patches, m % 64, Hp > Wp
PROPERTIES = {
    "one_patch":  dict(n=6, n_mod64=6, m=72, m_mod64=8, tall=False),
    "strip_w":    dict(n=64, n_mod64=0, m=118, m_mod64=54, tall=False),
    "strip_h":    dict(n=65, n_mod64=1, m=120, m_mod64=56, tall=True),
    "n128":       dict(n=128, n_mod64=0, m=246, m_mod64=54, tall=False),
    "n129":       dict(n=129, n_mod64=1, m=248, m_mod64=56, tall=False),
    "tall":       dict(n=29, n_mod64=29, m=72, m_mod64=8, tall=True),
    "m64":        dict(n=21, n_mod64=21, m=80, m_mod64=16, tall=False),
    "m129":       dict(n=48, n_mod64=48, m=129, m_mod64=1, tall=False),
    "max":        dict(n=1029, n_mod64=5, m=1024, m_mod64=0, tall=False),
    "n129_const": dict(n=129, n_mod64=1, m=248, m_mod64=56, tall=False),
    "n129_big":   dict(n=129, n_mod64=1, m=248, m_mod64=56, tall=False),
    "n129_sharp": dict(n=129, n_mod64=1, m=248, m_mod64=56, tall=False),
}
SHARP = 6.0
# part 2: one image more than a natural chunk (DN_CHUNK_ROWS = 85 * 256 = 21760 token rows) of 16 x 32 images
CHUNK_H, CHUNK_W, CHUNK_N, CHUNK_SEED = 16, 32, 7, 210
CHUNK_CAP = 21760 // CHUNK_N         # 3108
CHUNK_B = CHUNK_CAP + 1
CHUNK_PROBES = (0, CHUNK_CAP - 1, CHUNK_CAP)


def uniform_input(b: int, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-2.1, 2.6, size=(b, 3, h, w)).astype(np.float32)


def case_input(name: str) -> np.ndarray:
    b, h, w, seed, _, kind, _ = CASES[name]
    if kind == "const":
        return np.full((b, 3, h, w), 0.7, np.float32)
    x = uniform_input(b, h, w, seed)
    return x * np.float32(100.0) if kind == "big" else x


def sharp_state_dict(sd: dict) -> dict:
    """A copy of the state dict with the query rows (0..383) of every attn.qkv.weight and attn.qkv.bias x SHARP."""
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            a = np.array(v, np.float32, copy=True)
            a[:384] *= np.float32(SHARP)
            out[k] = a
    return out


@functools.lru_cache(maxsize=None)
def state_dict(kind: str = "plain") -> dict:
    from genpose2_amd import weights
    sd = weights.synthetic_state_dict("dino", WEIGHT_SEED)
    return sharp_state_dict(sd) if kind == "sharp" else sd


def yardstick(sd: dict, x: np.ndarray, layers) -> dict:
    """The float64 run of dino_ref on the CPU and the float32 run's error against it:
    {"ref64": [arrays], "stats32": (layers, 3) array [layer][STATS]}."""
    import torch

    import dino_ref
    with torch.no_grad():
        ref64 = [o.numpy() for o in dino_ref.forward(sd, x, layers, torch.float64)]
        ref32 = [o.numpy() for o in dino_ref.forward(sd, x, layers, torch.float32)]
    stats = np.array([[di.error_stats(a, b)[s] for s in STATS] for a, b in zip(ref32, ref64)])
    for r in ref64:
        r.setflags(write=False)
    stats.setflags(write=False)
    return {"ref64": ref64, "stats32": stats}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """yardstick() of a case, computed once per process (both arithmetics and the CPU tests share it)."""
    return yardstick(state_dict(CASES[name][6]), case_input(name), CASES[name][4])


@functools.lru_cache(maxsize=None)
def chunk_input() -> np.ndarray:
    x = uniform_input(CHUNK_B, CHUNK_H, CHUNK_W, CHUNK_SEED)
    x.setflags(write=False)
    return x
