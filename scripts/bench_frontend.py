"""Time of the RGB-D front end (genpose2_amd.frontend.frame_objects) on a 480 x 640 frame with --objects objects,
S = 224, n_pts = 1024, beside the numpy restatement of the same rules (tests/frontend_ref.py, the stand-in for the
host-side front end callers bring today) and GenPose2.inference's total on the same frame. The device times are
device events around whole calls (a call holds its two host reads), the host times a host clock; medians over
--repeats after a warm-up, the device variants alternated within every repeat. Prints one JSON line per object count.

    python scripts/bench_frontend.py [--objects 8 32] [--repeats 20] [--no-inference]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import frontend_ref as ref  # noqa: E402
from genpose2_amd import frontend  # noqa: E402
from genpose2_amd.infer import GenPose2, default_config  # noqa: E402

H, W, S, N_PTS = 480, 640, 224, 1024
INTR = dict(fx=600.0, fy=600.0, cx=319.5, cy=239.5, width=W, height=H)


def make_frame(n_obj, seed=0):
    """n_obj rectangles of 30..70 pixels on a grid of cells, a tilted depth plane with 10 % holes, random colour."""
    rng = np.random.default_rng(seed)
    depth = (0.6 + 0.002 * np.arange(W)[None, :] + 0.001 * np.arange(H)[:, None]).astype(np.float32)
    depth[rng.random((H, W)) < 0.1] = 0
    color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.full((H, W), 255, np.uint8)
    cols = 8
    rows = (n_obj + cols - 1) // cols
    ch, cw = H // rows, W // cols
    for k in range(n_obj):
        r0, c0 = (k // cols) * ch, (k % cols) * cw
        hh, ww = int(rng.integers(30, min(71, ch))), int(rng.integers(30, min(71, cw)))
        mask[r0 + 2:r0 + 2 + hh, c0 + 2:c0 + 2 + ww] = k
    return depth, color, mask


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-inference", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gp = None if a.no_inference else GenPose2(None, cfg=default_config(device="cuda:0"))
    for n_obj in a.objects:
        depth, color, mask = make_frame(n_obj)
        on_dev = tuple(torch.from_numpy(x).to(dev) for x in (depth, color, mask))
        variants = {
            "frontend_device_inputs": lambda: frontend.frame_objects(*on_dev, INTR, S, N_PTS, device=dev),
            "frontend_host_inputs": lambda: frontend.frame_objects(depth, color, mask, INTR, S, N_PTS, device=dev),
        }
        if gp is not None:
            variants["inference_total"] = lambda: gp.inference(
                frontend.frame_objects(*on_dev, INTR, S, N_PTS, device=dev))
        ev = {k: [] for k in variants}
        host = {k: [] for k in variants}
        for rep in range(a.repeats + 1):       # the first pass warms up: code objects, workspaces
            for k, fn in variants.items():
                if k == "inference_total" and rep > max(3, a.repeats // 4):
                    continue
                d, h, out = timed(fn)
                if rep:
                    ev[k].append(d)
                    host[k].append(h)
        batch = variants["frontend_device_inputs"]()
        t_ref = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = ref.frame_objects(depth, color, mask, INTR, S, N_PTS, 4.0, 0)
            for box in want["boxes"]:
                ref.roi_rgb(color, box, S)
            t_ref.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(batch["pts"].cpu().numpy(), want["pts"])
                    and np.array_equal(batch["roi_xs"].cpu().numpy(), want["roi_xs"]))
        out = {"frame": [H, W], "objects": int(batch["pts"].shape[0]), "img_size": S, "n_pts": N_PTS,
               "repeats": a.repeats, "equals_restatement": same,
               "count_min_max": [int(batch["count"].min()), int(batch["count"].max())],
               "numpy_restatement_host_ms": round(float(np.median(t_ref)), 2),
               "host_threads": torch.get_num_threads()}
        for k in variants:
            out[k + "_event_ms"] = round(float(np.median(ev[k])), 3)
            out[k + "_event_ms_min_max"] = [round(min(ev[k]), 3), round(max(ev[k]), 3)]
            out[k + "_host_clock_ms"] = round(float(np.median(host[k])), 3)
            out[k + "_timed_calls"] = len(ev[k])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
