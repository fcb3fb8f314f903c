"""The object-coupled likelihood beside the batch-coupled one (PoseNet.get_likelihood, like_coupling "object" |
"batch") on one GPU: (1) on tests/golden/golden_like_object.npz (B = 3 x K = 7) in both arithmetics: |ll - ll64| in
max and mean over the 21 rows beside the spread of the reference's own three float32 runs, nfev per object beside the
reference's per-object calls, and the time of one call of either coupling; (2) at B x K (default 256 x 50, f16x3, the
encoder's features of config-4 clouds, seeded poses): the time of one call of either coupling, the attempts of the
batch's one solve and of the objects' solves. Times are wall clock around a synchronised call, the median of
--repeats after a warm-up; the batch-coupled call at B x K is timed once (it reads an error norm per attempt). One JSON
line at the end.
usage: python scripts/bench_like_object.py [--repeats 3] [-B 256] [-K 50] [--skip-large]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
from genpose2_amd import synthetic  # noqa: E402
from genpose2_amd.agent import NoiseFeed, PoseNet  # noqa: E402
from genpose2_amd.config import GenPoseConfig  # noqa: E402
from like_inputs import _gs6  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def fixture(agents, repeats):
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_like_object.npz"))
    refs = [np.abs(g[k] - g["ll64"]) for k in ("ll32", "ll32_p1", "ll32_p2")]
    spread = {"max": max(float(e.max()) for e in refs), "mean": max(float(e.mean()) for e in refs)}
    print(f"fixture: reference fp32 spread about ll64: {spread}; reference nfev per object fp32 "
          f"{g['nfev_ll32'].tolist()}, float64 {g['nfev_ll64'].tolist()}, whole batch {int(g['nfev_ll32_batch'])}")
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    poses = torch.from_numpy(g["pose_samples"]).to(DEV)
    out = {"spread": spread}
    for arith in ("f16x3", "f32"):
        for mode, a in agents.items():
            a.heads.set_arith(arith)
            a.noise_feed = NoiseFeed(torch.from_numpy(g["eps_unit"]))
            res = {}

            def call():
                res["ll"] = a.get_likelihood(dict(data), poses)
            med, lo, hi = timed(call, repeats)
            a.noise_feed = None
            a.heads.set_arith("f16x3")
            e = np.abs(res["ll"].cpu().numpy() - g["ll64"])
            nfev = a.last_nfev_objects.tolist() if mode == "object" else [int(a.last_nfev)]
            out[f"{arith}_{mode}"] = {"max": float(e.max()), "mean": float(e.mean()), "nfev": nfev, "median_ms": med}
            print(f"fixture {arith} {mode:>6}: |ll - ll64| max {e.max():.3f} mean {e.mean():.3f}; nfev {nfev}; "
                  f"call median {med:.0f} ms (range {lo:.0f} .. {hi:.0f}, encoder included)")
    return out


def large(agents, B, K, repeats):
    pts, center = synthetic.make_batch(4, B, 1024)
    rng = np.random.default_rng(5)
    local = np.concatenate([_gs6(rng.normal(size=(B * K, 6))), 0.05 * rng.normal(size=(B * K, 3))], 1)
    cam = local.astype(np.float32)
    cam[:, 6:] += np.repeat(center, K, 0)
    poses = torch.from_numpy(cam.reshape(B, K, 9)).to(DEV)
    prior = torch.from_numpy(rng.standard_normal((B * K, 9)).astype(np.float32))
    a = agents["object"]
    feat = a.encoder.forward(torch.from_numpy(pts).to(DEV))
    data = {"pts": torch.zeros((B, 1, 3), device=DEV), "pts_feat": feat, "pts_center": torch.from_numpy(center).to(DEV)}
    out = {"B": B, "K": K}
    for mode, a in agents.items():
        a.heads.set_arith("f16x3")
        a.noise_feed = NoiseFeed(prior)

        def call():
            a.get_likelihood(dict(data), poses, extract_feature=False)
        if mode == "object":
            med, lo, hi = timed(call, repeats)
            att = (a.last_nfev_objects - 2) // 6
            out[mode] = {"median_ms": med, "attempts": {"min": int(att.min()), "median": float(np.median(att)),
                                                        "max": int(att.max())},
                         "status": sorted(set(a.last_status_objects.tolist()))}
        else:   # one host-controlled solve: timed once, after no warm-up of its own
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            med = lo = hi = (time.perf_counter() - t0) * 1e3
            out[mode] = {"median_ms": med, "attempts": (int(a.last_nfev) - 2) // 6}
        a.noise_feed = None
        print(f"B = {B} x K = {K} f16x3 {mode:>6}: call {med:.0f} ms (range {lo:.0f} .. {hi:.0f}); {out[mode]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("-B", type=int, default=256)
    ap.add_argument("-K", type=int, default=50)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    agents = {m: PoseNet(GenPoseConfig(device=DEV, like_coupling=m)).eval() for m in ("object", "batch")}
    print("device:", torch.cuda.get_device_name(0))
    res = {"fixture": fixture(agents, a.repeats)}
    if not a.skip_large:
        res["large"] = large(agents, a.B, a.K, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
