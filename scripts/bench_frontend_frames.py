"""Several frames per call against one frame per call: F seeded 480 x 640 frames of bench_frontend.py with 8 objects
each, S = 224, n_pts = 1024, inputs on the device.

  front end   F calls of frontend.frame_objects          against one frontend.frames_objects
  inference   F calls of GenPose2.inference (one frame)  against one GenPose2.inference_frames,
              in the default configuration and with ode_coupling="object"

Device events around whole calls that end synchronised, every shape warmed up, the two variants alternated within
each repeat, median and range over --repeats. In the same run the batched front-end outputs are compared with the
per-frame ones bit for bit. Prints one JSON line per F.

    python scripts/bench_frontend_frames.py [--frames 1 4 16 32] [--repeats 10] [--no-inference]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
from bench_frontend import H, INTR, N_PTS, S, W, make_frame  # noqa: E402
from genpose2_amd import frontend  # noqa: E402
from genpose2_amd.infer import GenPose2, default_config  # noqa: E402

OBJECTS = 8
KEYS = ("pts", "roi_xs", "roi_ys", "roi_rgb", "count", "ids", "pts_center", "zero_mean_pts")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(variants, repeats):
    """Every variant once per repeat, in turn; the first pass warms up (code objects, workspaces) and is dropped."""
    ms = {k: [] for k in variants}
    for rep in range(repeats + 1):
        for k, fn in variants.items():
            t, _ = timed(fn)
            if rep:
                ms[k].append(t)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-inference", action="store_true")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    dev = torch.device("cuda:0")
    configs = {} if a.no_inference else {
        "default": GenPose2(None, cfg=default_config(device="cuda:0")),
        "ode_object": GenPose2(None, cfg=default_config(device="cuda:0", ode_coupling="object"))}
    for F in a.frames:
        frames = [make_frame(OBJECTS, seed=f) for f in range(F)]
        per = [tuple(torch.from_numpy(x).to(dev) for x in fr) for fr in frames]
        stacked = tuple(torch.stack([p[k] for p in per]) for k in range(3))
        seeds = list(range(F))

        def loop():
            return [frontend.frame_objects(*per[f], INTR, S, N_PTS, seed=seeds[f], device=dev) for f in range(F)]

        def once():
            return frontend.frames_objects(*stacked, INTR, S, N_PTS, seed=seeds, device=dev)

        ms = alternate({"frontend_loop": loop, "frontend_frames": once}, a.repeats)
        singles, batch = loop(), once()
        same = batch["frame_offsets"] == [OBJECTS * f for f in range(F + 1)] and all(
            torch.equal(batch[k], torch.cat([s[k] for s in singles])) for k in KEYS)
        for name, gp in configs.items():
            ms.update({f"inference_{name}_{k}": v for k, v in alternate({
                "loop": lambda: [gp.inference(frontend.frame_objects(*per[f], INTR, S, N_PTS, seed=seeds[f], device=dev))
                                 for f in range(F)],
                "frames": lambda: gp.inference_frames(
                    frontend.frames_objects(*stacked, INTR, S, N_PTS, seed=seeds, device=dev))}, a.repeats).items()})
        B = int(batch["pts"].shape[0])
        out = {"frames": F, "frame": [H, W], "objects": B, "img_size": S, "n_pts": N_PTS, "repeats": a.repeats,
               "batched_equals_per_frame_bitwise": bool(same)}
        for k, v in ms.items():
            out[k + "_ms"] = round(float(np.median(v)), 3)
            out[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            out[k + "_objects_per_ms"] = round(B / float(np.median(v)), 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
