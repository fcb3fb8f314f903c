"""Time per host-controlled RK45 attempt at R rows: the likelihood attempt (gp_like_attempt: six stages of score +
forward-mode divergence over [x | logp]) beside the sampling attempt (gp_ode_attempt: six score stages), both as
six stage launches + the norm kernel, timed with device events over back-to-back attempts (no host read
between them). Prints one JSON line.

    python scripts/bench_like_attempt.py [--rows 12800] [--k 50] [--iters 200] [--arith f16x3|f32]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose2_amd import _lib, device, ode, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12800)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--arith", default="f16x3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    heads = device.HeadModel(weights.synthetic_state_dict("score", seed=0), dev)
    heads.set_arith(a.arith)
    R, K = a.rows, a.k
    rng = np.random.default_rng(0)
    feat = np.maximum(rng.normal(size=((R + K - 1) // K, 1024)), 0).astype(np.float32)
    pobj = heads.object_proj(torch.from_numpy(feat).to(dev))
    x = rng.normal(size=(R, 9))
    x[:, 6:] *= 0.3
    eps = torch.from_numpy((rng.standard_normal((R, 9)) * 50.0).astype(np.float32)).to(dev)
    t, h = 0.3, 1e-3
    t32, sig, coef = ode.stage_scalars([t + c * h for c in ode.C[1:]] + [t + h])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {"rows": R, "k": K, "arith": a.arith, "iters": a.iters}
    for name, n in (("ode_attempt", 9 * R), ("like_attempt", 10 * R)):
        y = torch.zeros(n, dtype=torch.float64, device=dev)
        y[: 9 * R] = torch.from_numpy(x.reshape(-1)).to(dev)
        Ks = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(7)]
        ynew = torch.empty(n, dtype=torch.float64, device=dev)
        err = torch.zeros(1, dtype=torch.float64, device=dev)
        size = lib.gp_like_workspace_size if name == "like_attempt" else lib.gp_ode_workspace_size
        ws = torch.empty(int(size(R)), dtype=torch.uint8, device=dev)
        head = (ctypes.byref(heads.w), ctypes.c_void_p(pobj.data_ptr()), t32.ctypes.data_as(ctypes.c_void_p),
                sig.ctypes.data_as(ctypes.c_void_p), coef.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(y.data_ptr()))
        tail = (ode._ptr_array(Ks), ode._A6.ctypes.data_as(ctypes.c_void_p), ode._B6.ctypes.data_as(ctypes.c_void_p),
                ode._E7.ctypes.data_as(ctypes.c_void_p), h, 1e-5, 1e-5, R, K, ctypes.c_void_p(ynew.data_ptr()),
                ctypes.c_void_p(err.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream)

        def attempt():
            if name == "like_attempt":
                _lib.check(lib.gp_like_attempt(*head, ctypes.c_void_p(eps.data_ptr()), *tail), name)
            else:
                _lib.check(lib.gp_ode_attempt(*head, *tail), name)
        for _ in range(a.warmup):
            attempt()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            attempt()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(e0.elapsed_time(e1) * 1000.0 / a.iters, 2)
    out["ratio"] = round(out["like_attempt_us"] / out["ode_attempt_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
