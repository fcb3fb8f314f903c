"""Fixtures of the DINOv3 ViT-S+/16 backbone: golden_dino_a.npz, golden_dino_b.npz, golden_dino_c_l{2,6,11}.npz.

    python tests/golden/make_golden_dino.py

The weights are weights.synthetic_state_dict("dino", WEIGHT_SEED) and the inputs dino_inputs.case_input(name): both
are regenerated from their seeds and never stored. The files hold outputs only, computed by tests/dino_ref.py on
the CPU: cases (a) and (b) the float64 and the float32 outputs of layers [2, 6, 11]; case (c) the float64 outputs
(one file per layer) with the float32 run's error statistics [max, 99.9th percentile, mean] and, in the first
file, the sensitivity ratios.

Before writing anything the generator asserts
  * where ``transformers`` imports: dino_ref (float64) equals DINOv3ViTModel with the mapped weights to <= 1e-10
    when given that model's RoPE table (transformers evaluates the table in float32 whatever the dtype), and the
    two tables agree to float32 rounding (<= 2e-6) -- a second, independent reading of the architecture;
  * every switched-off variant of dino_ref (no RoPE, h / w swapped, bias mask ignored, prefix tokens rotated)
    moves the float64 output of case (a) by at least 100 x the float32 run's max error: a fixture that cannot
    see a mistake is no fixture.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import dino_inputs as di  # noqa: E402
import dino_ref  # noqa: E402
from genpose2_amd import weights  # noqa: E402

MIN_RATIO = 100.0


def run(sd, x, dtype, variant=None):
    with torch.no_grad():
        return [o.numpy() for o in dino_ref.forward(sd, x, di.LAYERS, dtype, variant=variant)]


def main() -> None:
    torch.manual_seed(0)
    sd = weights.synthetic_state_dict("dino", di.WEIGHT_SEED)
    try:
        import transformers  # noqa: F401
        out_diff, tab_diff = dino_ref.hf_cross_check(sd, di.case_input("a"), di.LAYERS)
        print(f"transformers cross-check: outputs {out_diff:.2e}, RoPE table {tab_diff:.2e}")
        assert out_diff <= 1e-10 and tab_diff <= 2e-6, (out_diff, tab_diff)
    except ImportError:
        print("transformers is not installed: cross-check skipped")
    ratios = None
    for name in di.CASES:
        x = di.case_input(name)
        ref64, ref32 = run(sd, x, torch.float64), run(sd, x, torch.float32)
        stats = np.array([[di.error_stats(a, b)[s] for s in di.STATS] for a, b in zip(ref32, ref64)])
        print(f"case {name}: x {x.shape}, |out| <= {max(np.abs(r).max() for r in ref64):.2f}, fp32 run error "
              f"[max p99.9 mean] per layer {stats.tolist()}")
        if name == "a":
            emax = stats[:, 0].max()
            ratios = {}
            for v in dino_ref.VARIANTS:
                moved = max(np.abs(a - b).max() for a, b in zip(run(sd, x, torch.float64, v), ref64))
                ratios[v] = float(moved / emax)
                print(f"  variant {v}: moves the output by {moved:.3e} = {ratios[v]:.0f} x the fp32 run's max error")
                assert ratios[v] >= MIN_RATIO, (v, ratios[v])
        paths = di.fixture_paths(name)
        if name == "c":
            for i, (p, l) in enumerate(zip(paths, di.LAYERS)):
                extra = {f"ratio_{k}": np.float64(v) for k, v in ratios.items()} if i == 0 else {}
                np.savez(p, ref64=ref64[i], stats32=stats[i], layer=np.int64(l), **extra)
        else:
            np.savez(paths[0], **{f"ref64_l{l}": r for l, r in zip(di.LAYERS, ref64)},
                     **{f"ref32_l{l}": r for l, r in zip(di.LAYERS, ref32)})
        for p in paths:
            size = os.path.getsize(p)
            print(f"  {os.path.basename(p)}: {size} bytes")
            assert size < (1 << 20), p


if __name__ == "__main__":
    main()
