"""Cases, seeds and inputs of the DINOv3 backbone fixtures (golden_dino_*.npz), regenerated from seeds wherever they
are needed: the generator (make_golden_dino.py), the CPU tests and the GPU tests all call these."""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHT_SEED = 3          # weights.synthetic_state_dict("dino", WEIGHT_SEED)
LAYERS = (2, 6, 11)
# name -> (B, H, W, input seed): (a) non-square, 29 tokens, below one 64-query tile; (b) 41 tokens;
# (c) the shipped shape, 261 tokens (a ragged fifth query tile and key chunk)
CASES = {"a": (3, 64, 96, 101), "b": (2, 96, 96, 102), "c": (1, 256, 256, 103)}
STATS = ("max", "p999", "mean")


def case_input(name: str) -> np.ndarray:
    """roi_rgb-like input (B, 3, H, W) float32: ImageNet-normalised pixels span about [-2.1, 2.6]."""
    b, h, w, seed = CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-2.1, 2.6, size=(b, 3, h, w)).astype(np.float32)


def fixture_paths(name: str):
    """(a), (b): one file; (c): one file per layer (every committed file stays below 1 MiB)."""
    if name == "c":
        return [os.path.join(HERE, f"golden_dino_c_l{l}.npz") for l in LAYERS]
    return [os.path.join(HERE, f"golden_dino_{name}.npz")]


def error_stats(got: np.ndarray, ref64: np.ndarray) -> dict:
    """max, 99.9th percentile and mean of |got - ref| (float64)."""
    e = np.abs(np.asarray(got, np.float64) - ref64).reshape(-1)
    return {"max": float(e.max()), "p999": float(np.quantile(e, 0.999)), "mean": float(e.mean())}


def load_case(name: str) -> dict:
    """-> {"x", "ref64": [3 arrays], "ref32": [3 arrays] or None, "stats32": (3, 3) array [layer][STATS]}."""
    files = [np.load(p) for p in fixture_paths(name)]
    if name == "c":
        ref64 = [f["ref64"] for f in files]
        stats = np.stack([f["stats32"] for f in files])
        ref32 = None
    else:
        f = files[0]
        ref64 = [f[f"ref64_l{l}"] for l in LAYERS]
        ref32 = [f[f"ref32_l{l}"] for l in LAYERS]
        stats = np.array([[error_stats(a, b)[s] for s in STATS] for a, b in zip(ref32, ref64)])
    return {"x": case_input(name), "ref64": ref64, "ref32": ref32, "stats32": stats}
