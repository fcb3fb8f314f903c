"""Cost of per-object coupling in the PC sampler: whole HeadModel.pc_sample calls at config 4's shape (B = 256
objects x K = 50 candidates, T = 500 steps, device Philox draws) on one GPU, coupling "batch" and "object"
alternating within each repeat, HIP events around each call. Prints the median and range per mode, their ratio,
and one JSON line. Under the default head arithmetic (f16x3 planes) "batch" runs the hybrid (FP8) form of the
64-candidate tile as it does by default, "object" the six-product f16x3 form: --pc-small f16 puts "batch" on the
six f16 products too (the same arithmetic on both sides, so the ratio is the coupling's cost alone), --arith f32
both on exact fp32.
usage: python scripts/bench_pc_object.py [--repeats 5] [--arith f16x3|f32] [--pc-small auto|f16] [-B 256] [-K 50]
       [-T 500]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose2_amd import arch, sde, synthetic  # noqa: E402
from genpose2_amd.agent import PoseNet  # noqa: E402
from genpose2_amd.config import GenPoseConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--arith", default="f16x3", choices=("f16x3", "f32"))
    ap.add_argument("--pc-small", default="auto", choices=("auto", "f16"))
    ap.add_argument("-B", type=int, default=256)
    ap.add_argument("-K", type=int, default=50)
    ap.add_argument("-T", type=int, default=500)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    agent = PoseNet(GenPoseConfig(device="cuda:0", sampling_steps=a.T)).eval()
    agent.heads.set_pc_small(a.pc_small)
    agent.heads.set_arith(a.arith)
    B, K, T = a.B, a.K, a.T
    pts, center = synthetic.make_batch(4, B, 1024)
    pobj = agent.heads.object_proj(agent.encoder.forward(torch.from_numpy(pts).to(dev)))
    center = torch.from_numpy(center).to(dev)
    tab, tproj = agent._pc_table(T)
    x0 = torch.randn(B * K, 9, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * sde.prior_sigma(arch.SDE_T)
    modes = ("batch", "object")

    def call(mode, seed):
        x = x0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        agent.heads.pc_sample(pobj, tproj, tab, x, K, center, seed=seed, coupling=mode)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for m in modes:                                   # warm-up: workspace, code objects, clocks
        call(m, 0)
    ms = {m: [] for m in modes}
    for r in range(a.repeats):
        for m in modes:
            ms[m].append(call(m, 1 + r))
    out = {"shape": {"B": B, "K": K, "T": T}, "arith": a.arith, "pc_small": a.pc_small, "repeats": a.repeats}
    for m in modes:
        v = ms[m]
        out[m] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        print(f"{m:>6}: median {out[m]['median_ms']:.2f} ms, range {min(v):.2f} .. {max(v):.2f} ms "
              f"({out[m]['median_ms'] * 1e3 / T:.1f} us / step)")
    out["object_over_batch"] = out["object"]["median_ms"] / out["batch"]["median_ms"]
    print(f"object / batch (medians): {out['object_over_batch']:.4f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
