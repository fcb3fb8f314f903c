"""Fixture of the per-object PC sampler, made by running the REFERENCE itself: cond_pc_sampler (samplers.py:113-177,
GFObjectPose.forward(mode='pc_sample'), posenet.py:338-340) called once per object, on that object's K candidates
alone, so that the Langevin grad_norm (samplers.py:143-144) is the mean over that object's rows only.

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/pc_object_inputs.py (seeded). Weights are
weights.synthetic_state_dict("score", seed=0).

golden_pc_object.npz -- B = 3 objects x K = 10, T = 20 steps, prior and z1 / z2 injected. pred_pose32 / pred_q32 /
  xs32: the B per-object calls in float32, as the reference runs, stacked in row order; pred_pose64 / pred_q64 /
  xs64: the same with net.double() and state, noise and the sampler's scalars in float64; pred_pose32_batch: one
  float32 call on all 30 rows (the whole-batch grad_norm), which a test holds against pred_pose32 to show that the
  fixture tells the two semantics apart. If it cannot, the seed in pc_object_inputs.py changes.

Usage:  python tests/golden/make_golden_pc_object.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import pc_object_inputs as pi  # noqa: E402
from make_golden_likelihood import save_npz  # noqa: E402
import torch  # noqa: E402


def _pc_run(net, inp, rows, dtype):
    """One mode='pc_sample' call on rows [rows.start, rows.stop) (whole objects) with their prior and z1 / z2 rows,
    then the quaternion of res (posenet_agent.py:554-556), all in `dtype`."""
    from utils.misc import get_rot_matrix
    from utils.transforms.rotation_conversions import matrix_to_quaternion
    K, T = pi.K, pi.T
    np_t = np.float64 if dtype == torch.float64 else np.float32
    R = rows.stop - rows.start
    zs = np.empty((2 * T, R, 9), np_t)
    zs[0::2], zs[1::2] = inp["z1"][:, rows], inp["z2"][:, rows]
    data = {"pts": torch.zeros(R, 1, 3, dtype=dtype),
            "pts_feat": torch.from_numpy(np.repeat(inp["pts_feat"], K, 0)[rows]).to(dtype), "rgb_feat": None,
            "pts_center": torch.from_numpy(np.repeat(inp["pts_center"], K, 0)[rows]).to(dtype)}
    with mg.NoiseFeed(inp["prior"][rows].astype(np_t), zs) as nf, torch.no_grad():
        xs, res = net(data, mode="pc_sample")
        assert nf.i == 2 * T
    q = torch.cat((matrix_to_quaternion(get_rot_matrix(res[:, :-3], "rot_matrix")), res[:, -3:]), dim=-1)
    assert res.dtype == dtype and xs.dtype == dtype
    return res.numpy(), q.numpy(), xs.numpy()


def _per_object(net, inp, dtype):
    parts = [_pc_run(net, inp, slice(b * pi.K, (b + 1) * pi.K), dtype) for b in range(pi.B)]
    return tuple(np.concatenate([p[j] for p in parts], 0) for j in range(3))


def main():
    get_config, PoseNet = mg.import_reference("pc", None)
    inp = pi.inputs()
    out = dict(inp)
    a32 = mg.make_agent(get_config, PoseNet, "score", "pc", pi.T)
    assert a32.cfg.pose_mode == "rot_matrix"
    out["pred_pose32"], out["pred_q32"], out["xs32"] = _per_object(a32.net, inp, torch.float32)
    out["pred_pose32_batch"] = _pc_run(a32.net, inp, slice(0, pi.B * pi.K), torch.float32)[0]
    net64 = mg.make_agent(get_config, PoseNet, "score", "pc", pi.T).net.double()
    torch.set_default_dtype(torch.float64)     # the sampler's time grid, ones(...) and scalars in float64 too
    try:
        out["pred_pose64"], out["pred_q64"], out["xs64"] = _per_object(net64, inp, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    e = np.abs(out["pred_pose32"].astype(np.float64) - out["pred_pose64"]).max(1)
    d = np.abs(out["pred_pose32_batch"] - out["pred_pose32"]).reshape(pi.B, -1).max(1)
    print(f"per object: reference fp32 pred_pose error vs float64: max {e.max():.2e} mean {e.mean():.2e}")
    print("whole-batch call vs per-object calls, max |difference| per object:", " ".join(f"{v:.2e}" for v in d))
    save_npz(os.path.join(HERE, "golden_pc_object.npz"), out)


if __name__ == "__main__":
    main()
