#!/usr/bin/env python
"""Times the DINOv3 ViT-S+/16 backbone (genpose2_amd/dino.py) at the shipped shape and, beside it, the same model
run by torch in float32 on the same GPU (tests/dino_ref.py moved to the device): the baseline to beat.

    python scripts/bench_dino.py [--b 256] [--size 256] [--steps 10] [--warmup 3] [--arith split_f16 f32] [--no-torch]

Device-event timings after warm-up, one JSON line per configuration. FLOPs are counted from the shapes (linears,
patch embedding, QK^T and PV; 2 per multiply-add). Per-kernel shares come from a separate profiler run of this
script with --no-torch and one --arith (rocprofv3 --kernel-trace --stats)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

LAYERS = (2, 6, 11)
SPLIT_PEAK_TFLOPS = 839.0     # three f16 MFMA products per fp32 product: a third of the f16 dense peak


def flops(b: int, size: int) -> dict:
    npatch = (size // 16) ** 2
    n = npatch + 5
    lin = 12 * 2 * n * (384 * 1152 + 384 * 384 + 384 * 3072 + 1536 * 384)
    attn = 12 * 2 * 2 * 6 * n * n * 64
    patch = 2 * npatch * 768 * 384
    return {"linears": b * lin, "attention": b * attn, "patch_embed": b * patch, "total": b * (lin + attn + patch)}


def timed(fn, steps: int, warmup: int) -> list:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arith", nargs="+", default=["split_f16", "f32"])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino.py needs a HIP device: there is no CPU timing")
    from genpose2_amd import weights
    from genpose2_amd.dino import DinoBackbone
    dev = torch.device("cuda:0")
    sd = weights.synthetic_state_dict("dino", a.seed)
    rng = np.random.Generator(np.random.PCG64(a.seed))
    x = torch.from_numpy(rng.uniform(-2.1, 2.6, (a.b, 3, a.size, a.size)).astype(np.float32)).to(dev)
    fl = flops(a.b, a.size)
    bb = DinoBackbone(sd, dev)
    outs = {}
    for arith in a.arith:
        bb.set_arith(arith)
        ms = timed(lambda: bb.get_intermediate_layers(x, n=list(LAYERS)), a.steps, a.warmup)
        outs[arith] = bb.get_intermediate_layers(x, n=list(LAYERS))
        med = float(np.median(ms))
        res = {"what": "dino_backbone", "arith": arith, "b": a.b, "size": a.size, "ms_median": med, "ms_min": min(ms),
               "ms_max": max(ms), "tflops": fl["total"] / med * 1e-9, "flop": fl}
        if arith == "split_f16":
            res["fraction_of_three_product_peak"] = fl["total"] / med * 1e-9 / SPLIT_PEAK_TFLOPS
        print(json.dumps(res), flush=True)
    if not a.no_torch:
        import dino_ref
        torch.backends.cuda.matmul.allow_tf32 = False
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}   # the weights stay on the device
        with torch.no_grad():
            ms = timed(lambda: dino_ref.forward(sd_dev, x, LAYERS, torch.float32, device=dev), a.steps, a.warmup)
            ref = dino_ref.forward(sd_dev, x, LAYERS, torch.float32, device=dev)
        med = float(np.median(ms))
        res = {"what": "torch_fp32_dino_ref", "b": a.b, "size": a.size, "ms_median": med, "ms_min": min(ms),
               "ms_max": max(ms), "tflops": fl["total"] / med * 1e-9}
        for arith, o in outs.items():
            res[f"max_abs_diff_{arith}"] = max(float((p - q).abs().max()) for p, q in zip(o, ref))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
