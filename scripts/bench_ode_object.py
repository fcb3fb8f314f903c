"""Cost of per-object coupling in the ODE sampler: whole solves at config 4's shape (B = 256 objects x K = 50
candidates, T0 = 0.55, t_eval of 20 steps) on one GPU, coupling "batch" (gp_ode_sample: one RK45 solve on every row)
and "object" (gp_ode_sample_object: one solve per object) alternating within each repeat, HIP events around each
call. Prints the median and range per mode, their ratio, the batch's attempt count against the per-object counts
(the object mode runs as many attempts as its slowest object), and the share of a per-object attempt spent in the
control kernel (decision, stage scalars and the folded time rows) from a short run of attempts timed kernel by
kernel. One JSON line at the end.
usage: python scripts/bench_ode_object.py [--repeats 5] [--arith f16x3|f32|both] [-B 256] [-K 50] [--t0 0.55]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose2_amd import _lib, arch, sde, synthetic  # noqa: E402
from genpose2_amd.agent import PoseNet  # noqa: E402
from genpose2_amd.config import GenPoseConfig  # noqa: E402

STEPS = 20


def batch_call(h, pobj, x0, K, center, T0, ws, pose, q):
    nfev, status = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(h.lib.gp_ode_sample(ctypes.byref(h.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(x0.data_ptr()),
                                   x0.shape[0], K, T0, arch.SAMPLING_EPS, STEPS, 1e-5, 1e-5,
                                   ctypes.c_void_p(center.data_ptr()), ctypes.c_void_p(pose.data_ptr()),
                                   ctypes.c_void_p(q.data_ptr()), ctypes.byref(nfev), ctypes.byref(status),
                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), h._s()), "ode_sample")
    return np.asarray([nfev.value])


def run(arith, a):
    dev = torch.device("cuda:0")
    agent = PoseNet(GenPoseConfig(device="cuda:0", sampler_mode=["ode"], sampling_steps=STEPS)).eval()
    agent.heads.set_arith(arith)
    h = agent.heads
    B, K = a.B, a.K
    R = B * K
    pts, center = synthetic.make_batch(4, B, 1024)
    pobj = h.object_proj(agent.encoder.forward(torch.from_numpy(pts).to(dev)))
    center = torch.from_numpy(center).to(dev)
    x0 = (torch.randn(R, 9, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
          * sde.prior_sigma(a.t0)).contiguous()
    ws = torch.empty(int(h.lib.gp_ode_sample_workspace_size(R)), dtype=torch.uint8, device=dev)
    pose = torch.empty((R, 9), dtype=torch.float64, device=dev)
    q = torch.empty((R, 7), dtype=torch.float64, device=dev)
    modes = ("batch", "object")
    nfev = {}

    def call(mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if mode == "batch":
            nfev[mode] = batch_call(h, pobj, x0, K, center, a.t0, ws, pose, q)
        else:
            nfev[mode] = h.ode_sample_object(pobj, x0, K, center, a.t0, arch.SAMPLING_EPS, STEPS)[2]
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for m in modes:                                   # warm-up: workspace, code objects, clocks
        call(m)
    ms = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m in modes:
            ms[m].append(call(m))
    out = {"shape": {"B": B, "K": K, "T0": a.t0, "steps": STEPS}, "arith": arith, "repeats": a.repeats}
    att = {m: (nfev[m] - 2) // 6 for m in modes}
    for m in modes:
        v = ms[m]
        n_att = int(att[m].max())
        out[m] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "attempts": n_att,
                  "us_per_attempt": statistics.median(v) * 1e3 / n_att}
        print(f"{arith} {m:>6}: median {out[m]['median_ms']:.2f} ms, range {min(v):.2f} .. {max(v):.2f} ms, "
              f"{n_att} attempts ({out[m]['us_per_attempt']:.0f} us / attempt, launches and status reads included)")
    ao = att["object"]
    out["object"]["attempts_per_object"] = {"min": int(ao.min()), "median": float(np.median(ao)), "max": int(ao.max())}
    out["object_over_batch"] = out["object"]["median_ms"] / out["batch"]["median_ms"]
    print(f"{arith} attempts per object: min {ao.min()} median {np.median(ao):.0f} max {ao.max()} "
          f"(whole batch: {int(att['batch'][0])})")
    print(f"{arith} object / batch (medians): {out['object_over_batch']:.4f}")
    # device time by kernel of one more object-coupled solve (the profiler's kernel records): the control kernel
    # (decision, stage scalars, the six folded time rows per object) against the six-stage attempt kernel
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call("object")
        torch.cuda.synchronize()
    us = {"control": 0.0, "attempt": 0.0}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        t = ev.cuda_time_total if t is None else t
        if "ode_obj_control_kernel" in ev.key:
            us["control"] += t
        elif "ode_obj_attempt_kernel" in ev.key:
            us["attempt"] += t
    if us["attempt"] <= 0.0:
        raise RuntimeError("the profiler recorded no ode_obj_attempt_kernel")
    n_att = int(ao.max()) + 3                          # launches: + the run-ahead attempt and select_initial_step's two
    out["object"]["control_us_per_attempt"] = us["control"] / n_att
    out["object"]["stages_us_per_attempt"] = us["attempt"] / n_att
    out["object"]["control_share"] = us["control"] / (us["control"] + us["attempt"])
    print(f"{arith} object, kernels per attempt: control + time rows {us['control'] / n_att:.1f} us, stages "
          f"{us['attempt'] / n_att:.1f} us: control share {out['object']['control_share']:.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--arith", default="both", choices=("f16x3", "f32", "both"))
    ap.add_argument("-B", type=int, default=256)
    ap.add_argument("-K", type=int, default=50)
    ap.add_argument("--t0", type=float, default=0.55)
    a = ap.parse_args()
    res = [run(ar, a) for ar in (("f16x3", "f32") if a.arith == "both" else (a.arith,))]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
