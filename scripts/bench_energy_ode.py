"""Time of the ODE sampler driven by the energy model's score (the energy backend of ode.DeviceRk45 under the device
controller: gp_ode_auto_attempt_energy, exact-fp32 trunk + reverse pass per stage) beside the exact-fp32 score ODE
(set_arith("f32"): the same trunk, forward only) on the same inputs, at B objects x K candidates from T0 with
t_eval of `steps` points. Each is timed with device events over whole calls (initial step, attempts, dense output,
denoise), alternating the two within every repeat, after a warm-up. The two solves take different numbers of
attempts (the energy's gradient is discontinuous at ReLU kinks), so the per-attempt time is reported too, and with
--split the share of the attempts' stage launches in it (ode.STAGE_EVENTS). Prints one JSON line.

    python scripts/bench_energy_ode.py [--b 256] [--k 50] [--t0 0.55] [--steps 20] [--repeats 5] [--split]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose2_amd import arch, device, ode, sde, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=256)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--t0", type=float, default=0.55)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--split", action="store_true", help="also time the attempts' stage launches alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    heads = device.HeadModel(weights.synthetic_state_dict("energy", seed=0), dev)
    heads.set_arith("f32")
    B, K, T0, steps = a.b, a.k, a.t0, a.steps
    R = B * K
    eps = arch.SAMPLING_EPS
    rng = np.random.default_rng(0)
    feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pobj = heads.object_proj(torch.from_numpy(feat).to(dev))
    x0 = torch.from_numpy(rng.standard_normal((R, 9)).astype(np.float32)).to(dev) * sde.prior_sigma(T0)
    center = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    t_eval = np.linspace(T0, eps, steps)
    t32, sig, _ = ode.time_scalars(eps)
    g2 = float(sde.diffusion(torch.full((1,), eps, dtype=torch.float32)).to(torch.float32) ** 2)
    step = float(np.float32((1 - eps) / steps))
    variants = (("energy_grad_f32", True), ("score_f32", False))
    info = {}

    def run(name, grad):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        be = ode.DeviceRk45(heads, pobj, x0, K, energy_grad=grad)
        x, nfev, status = ode.rk45_device(be, T0, eps, t_eval=t_eval)
        pose, _ = heads.ode_denoise(pobj, t32, sig, g2, step, x, K, center, be.ws, energy_grad=grad)
        e1.record()
        torch.cuda.synchronize()
        info[name] = {"nfev": nfev, "attempts": (nfev - 2) // 6, "status": status,
                      "finite": bool(torch.isfinite(pose).all())}
        return e0.elapsed_time(e1)

    for name, grad in variants:     # warm-up: code objects, the transposed weights, pinned buffers
        run(name, grad)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, grad in variants:
            ms[name].append(run(name, grad))
    out = {"b": B, "k": K, "rows": R, "t0": T0, "steps": steps, "repeats": a.repeats}
    for name in ms:
        med = float(np.median(ms[name]))
        out[name + "_ms"] = round(med, 3)
        out[name + "_ms_min_max"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
        out[name + "_us_per_attempt"] = round(med * 1000.0 / info[name]["attempts"], 2)
        out[name] = info[name]
    out["ratio_call"] = round(out["energy_grad_f32_ms"] / out["score_f32_ms"], 3)
    out["ratio_per_attempt"] = round(out["energy_grad_f32_us_per_attempt"] / out["score_f32_us_per_attempt"], 3)
    if a.split:   # the stage launches of every attempt between their own events (the control kernels are outside)
        for name, grad in variants:
            ode.STAGE_EVENTS = []
            try:
                run(name, grad)
                st = [s0.elapsed_time(s1) for s0, s1, _ in ode.STAGE_EVENTS]
            finally:
                ode.STAGE_EVENTS = None
            out[name + "_stage_us_per_attempt"] = round(1000.0 * float(np.mean(st)), 2)
        out["ratio_stages_per_attempt"] = round(out["energy_grad_f32_stage_us_per_attempt"]
                                                / out["score_f32_stage_us_per_attempt"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
