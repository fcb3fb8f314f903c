"""Fixture of the object-coupled likelihood (GenPoseConfig.like_coupling = "object"), made by running the
REFERENCE itself once per object: GFObjectPose.forward(data, mode="likelihood") on that object's K poses alone, so
every object has its own solve_ivp over [x_b (9K) | logp_b (K)].

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/like_object_inputs.py (seeded).

golden_like_object.npz -- B = 3 objects (config-21 clouds, each scaled differently, through the reference's
  encoder) x K = 7 poses. Per object: ll32 (the reference as is), ll32_p1 / ll32_p2 (the reference in float32 with
  pts_feat scaled by 1 + 2e-7 / 1 - 3e-7: independently rounded samples of the reference itself), ll64 and z64
  (cond_ode_likelihood restated in float64), and every run's nfev and status. ll32_batch: the reference on all 21
  rows in one call (one solve over the whole batch), for the record.

Usage:  python tests/golden/make_golden_like_object.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import like_object_inputs as lo  # noqa: E402
from make_golden_likelihood import _features, run_ll32, run_ll64, save_npz  # noqa: E402
import torch  # noqa: E402

MAX_NFEV = 30000   # per object and run: keeps the device tests short (pick another seed otherwise)


def main():
    get_config, PoseNet = mg.import_reference("ode", None)
    B, K = lo.B, lo.K
    d = mg.batch(lo.CONFIG_ID, B, lo.N_POINTS)
    pts = torch.from_numpy(lo.scale_clouds(d["pts"].numpy()))
    d = {"pts": pts, "pts_center": torch.mean(pts, dim=1)}
    inp = lo.pose_inputs(d["pts_center"].numpy())
    # the pose rows the model sees: pts_center subtracted from the camera-frame samples in float32
    rows = torch.from_numpy(inp["pose_samples"].reshape(B * K, 9).copy())
    rows[:, -3:] -= d["pts_center"].unsqueeze(1).repeat(1, K, 1).view(B * K, -1)
    rows = rows.numpy()
    eps = inp["eps_unit"]
    a32 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    net32, feat32 = _features(a32, d, False)
    out = dict(pts=d["pts"].numpy(), pts_center=d["pts_center"].numpy(), pts_feat=feat32.numpy(), **inp)
    runs = {"ll32": 1.0, "ll32_p1": 1 + 2e-7, "ll32_p2": 1 - 3e-7}
    for tag in runs:
        out[tag] = np.zeros((B, K))
        out["nfev_" + tag] = np.zeros(B, np.int64)
        out["status_" + tag] = np.zeros(B, np.int64)
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        fr = feat32[b:b + 1].repeat(K, 1)
        for tag, s in runs.items():
            t0 = time.time()
            f = fr if s == 1.0 else (fr * np.float32(s)).contiguous()
            ll, nfev, res = run_ll32(net32, f, rows[sl], eps[sl])
            out[tag][b] = ll
            out["nfev_" + tag][b] = nfev
            out["status_" + tag][b] = res.status
            print(f"object {b}: {tag} nfev {nfev} status {res.status} ({time.time() - t0:.0f} s)", flush=True)
            assert res.status == 0 and nfev <= MAX_NFEV, (b, tag, res.status, nfev)
    ll, nfev, res = run_ll32(net32, feat32.unsqueeze(1).repeat(1, K, 1).view(B * K, -1), rows, eps)
    out.update(ll32_batch=ll.reshape(B, K), nfev_ll32_batch=np.int64(nfev), status_ll32_batch=np.int64(res.status))
    print("whole batch: ll32_batch nfev", nfev, "status", res.status, flush=True)
    a64 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    net64, feat64 = _features(a64, d, True)
    out.update(ll64=np.zeros((B, K)), z64=np.zeros((B, K, 9)), nfev_ll64=np.zeros(B, np.int64),
               status_ll64=np.zeros(B, np.int64))
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        ll64, nfev64, res64 = run_ll64(net64, feat64[b:b + 1].repeat(K, 1), rows[sl], eps[sl])
        out["ll64"][b] = ll64
        out["z64"][b] = res64.y[:-K, -1].reshape(K, 9)
        out["nfev_ll64"][b] = nfev64
        out["status_ll64"][b] = res64.status
        print(f"object {b}: ll64 nfev {nfev64} status {res64.status}", flush=True)
        assert res64.status == 0 and nfev64 <= MAX_NFEV, (b, res64.status, nfev64)
    for b in range(B):
        for tag in runs:
            e = np.abs(out[tag][b] - out["ll64"][b])
            print(f"object {b}: |{tag} - ll64| max {e.max():.3f} mean {e.mean():.3f}")
    for tag in list(runs) + ["ll32_batch"]:
        e = np.abs(out[tag] - out["ll64"])
        print(f"all rows: |{tag} - ll64| max {e.max():.3f} mean {e.mean():.3f}")
    print("|ll64| range", np.abs(out["ll64"]).min(), np.abs(out["ll64"]).max())
    save_npz(os.path.join(HERE, "golden_like_object.npz"), out)


if __name__ == "__main__":
    main()
