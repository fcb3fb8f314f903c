"""Time of the PC sampler driven by the energy model's score (gp_pc_sample_energy: exact-fp32 trunk + reverse pass per
step) beside the exact-fp32 score sampler (gp_pc_sample with set_arith("f32"): the same trunk, forward only) and
the default f16x3 score sampler, at B objects x K candidates over T steps, Philox draws. Each is timed with device
events over whole sampler calls, alternating the variants within every repeat. Prints one JSON line.

    python scripts/bench_energy_pc.py [--b 256] [--k 50] [--steps 500] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose2_amd import arch, device, sde, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    heads = device.HeadModel(weights.synthetic_state_dict("energy", seed=0), dev)
    B, K, T = a.b, a.k, a.steps
    R = B * K
    rng = np.random.default_rng(0)
    feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pobj = heads.object_proj(torch.from_numpy(feat).to(dev))
    x0 = torch.from_numpy(rng.standard_normal((R, 9)).astype(np.float32)).to(dev) * sde.prior_sigma(arch.SDE_T)
    center = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    tab = sde.pc_step_table(T)
    tproj = heads.time_proj(torch.from_numpy(tab[:, 0]).to(dev))
    variants = (("energy_grad_f32", "f32", True), ("score_f32", "f32", False), ("score_f16x3", "f16x3", False))

    finite = {}

    def run(name, arith, grad):
        heads.set_arith(arith)
        x = x0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res, _, _ = heads.pc_sample(pobj, tproj, tab, x, K, center, seed=7, energy_grad=grad)
        e1.record()
        torch.cuda.synchronize()
        finite[name] = bool(torch.isfinite(res).all())
        return e0.elapsed_time(e1)

    for name, arith, grad in variants:     # warm-up: code objects, the transposed-weight upload, the workspace
        run(name, arith, grad)
    ms = {name: [] for name, _, _ in variants}
    for _ in range(a.repeats):
        for name, arith, grad in variants:
            ms[name].append(run(name, arith, grad))
    out = {"b": B, "k": K, "rows": R, "steps": T, "repeats": a.repeats}
    for name in ms:
        out[name + "_ms"] = round(float(np.median(ms[name])), 3)
        out[name + "_ms_min_max"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
        out[name + "_us_per_step"] = round(float(np.median(ms[name])) * 1000.0 / T, 2)
    out["finite"] = finite
    out["ratio_energy_grad_over_score_f32"] = round(out["energy_grad_f32_ms"] / out["score_f32_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
