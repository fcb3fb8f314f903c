"""bench.py's plain run: the headline line alone, --steps timed steps, and --dump-outputs' arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_and_dump(tmp_path):
    """A plain run (no --full) of the smallest config reports the headline keys and none of the legs that
    --full adds, counts --steps, and writes the last timed step's outputs as finite float32 arrays of the
    caller's shapes (config 2: B=64 objects x K=50 candidates; ScoreNet only, so no energy / aggregate)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "2", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    # value = B*K*T candidate-steps per step / the step's time
    assert d["value"] == pytest.approx(64 * 50 * 500 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "f32_exact", "ode", "pointwise", "cpu_baseline"):
        assert k not in d
    assert sorted(os.listdir(out)) == ["pred_pose.npy", "pred_q.npy"]
    for name, width in (("pred_pose", 9), ("pred_q", 7)):
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (64, 50, width) and np.isfinite(a).all()
