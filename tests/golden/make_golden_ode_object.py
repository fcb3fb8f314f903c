"""Fixture of the per-object ODE sampler, made by running the REFERENCE itself: cond_ode_sampler (samplers.py:180-258,
GFObjectPose.forward(mode='ode_sample'), posenet.py:341-343) called once per object, on that object's K candidates
alone, so that every object has its own solve_ivp(RK45): its own steps, accept / reject and error norms.

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/ode_object_inputs.py (seeded). Weights are
weights.synthetic_state_dict("score", seed=0).

golden_ode_object.npz -- B = 3 objects x K = 10, T0 = 0.55, steps = 20, prior injected. pred_pose32 / pred_q32 /
  nfev32[B]: the B per-object calls with the float32 net, as the reference runs, stacked in row order; pred_pose64 /
  nfev64[B]: the same with net.double() (the state, x0 and the solver's scalars are the reference's own: only the
  network's arithmetic changes); pred_pose_batch / nfev_batch: one float32 call on all 30 rows (one solve on the
  whole batch).

Two conditions are asserted; if one fails, raise SEED in ode_object_inputs.py and rerun:
  - nfev32 == nfev64 for every object: no accept / reject decision sits within float32 distance of its threshold,
    so equal nfev can be asked of an implementation with other float32 summation orders;
  - the whole-batch call is outside rotation 1e-4 or translation 1e-5 (relative) of the per-object calls on every
    object, and nfev_batch differs from at least one object's nfev: the fixture tells the two semantics apart.

Usage:  python tests/golden/make_golden_ode_object.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ode_object_inputs as oi  # noqa: E402
from make_golden_likelihood import save_npz  # noqa: E402
import torch  # noqa: E402


def _ode_run(net, inp, rows):
    """One mode='ode_sample' call on rows [rows.start, rows.stop) (whole objects) with their prior rows, then the
    quaternion of res (posenet_agent.py:554-556) -> (res, q, solve_ivp's nfev)."""
    import networks.gf_algorithms.samplers as smp
    from utils.misc import get_rot_matrix
    from utils.transforms.rotation_conversions import matrix_to_quaternion
    K = oi.K
    R = rows.stop - rows.start
    data = {"pts": torch.zeros(R, 1, 3), "pts_feat": torch.from_numpy(np.repeat(inp["pts_feat"], K, 0)[rows]),
            "rgb_feat": None, "pts_center": torch.from_numpy(np.repeat(inp["pts_center"], K, 0)[rows])}
    orig = smp.integrate.solve_ivp
    seen = {}

    def recording(*a, **k):
        res = orig(*a, **k)
        seen["nfev"], seen["status"] = int(res.nfev), int(res.status)
        return res

    smp.integrate.solve_ivp = recording
    try:
        with mg.NoiseFeed(inp["prior"][rows], np.zeros((0,), np.float32)), torch.no_grad():
            _, res = net(data, mode="ode_sample", T0=oi.T0)
    finally:
        smp.integrate.solve_ivp = orig
    assert seen["status"] == 0 and res.dtype == torch.float64
    q = torch.cat((matrix_to_quaternion(get_rot_matrix(res[:, :-3], "rot_matrix")), res[:, -3:]), dim=-1)
    return res.numpy(), q.numpy(), seen["nfev"]


def _per_object(net, inp):
    parts = [_ode_run(net, inp, slice(b * oi.K, (b + 1) * oi.K)) for b in range(oi.B)]
    return (np.concatenate([p[0] for p in parts], 0), np.concatenate([p[1] for p in parts], 0),
            np.asarray([p[2] for p in parts], np.int64))


def _to_double(module, args):
    """Forward pre-hook of the float64 net: ode_func hands the pose as float32 (samplers.py:212); the double net
    takes the same values as float64."""
    data = args[0]
    for k in ("sampled_pose", "t", "pts_feat"):
        if isinstance(data.get(k), torch.Tensor):
            data[k] = data[k].double()


def apart(batch, per, B, K):
    """Per object: is the whole-batch result outside rotation 1e-4 / translation 1e-5 (of max |t|) of the
    per-object one."""
    a, b = batch.reshape(B, K, 9), per.reshape(B, K, 9)
    tsc = np.abs(b[..., 6:]).max()
    return [bool(np.abs(a[o, :, :6] - b[o, :, :6]).max() > 1e-4 or np.abs(a[o, :, 6:] - b[o, :, 6:]).max() / tsc > 1e-5)
            for o in range(B)]


def main():
    get_config, PoseNet = mg.import_reference("ode", oi.STEPS)
    inp = oi.inputs()
    out = dict(inp)
    a32 = mg.make_agent(get_config, PoseNet, "score", "ode", oi.STEPS)
    assert a32.cfg.pose_mode == "rot_matrix"
    out["pred_pose32"], out["pred_q32"], out["nfev32"] = _per_object(a32.net, inp)
    pb, _, nb = _ode_run(a32.net, inp, slice(0, oi.B * oi.K))
    out["pred_pose_batch"], out["nfev_batch"] = pb, np.int64(nb)
    net64 = mg.make_agent(get_config, PoseNet, "score", "ode", oi.STEPS).net.double()
    net64.register_forward_pre_hook(_to_double)
    out["pred_pose64"], _, out["nfev64"] = _per_object(net64, inp)
    e = np.abs(out["pred_pose32"] - out["pred_pose64"]).max(1)
    d = np.abs(out["pred_pose_batch"] - out["pred_pose32"]).reshape(oi.B, -1).max(1)
    print(f"seed {oi.SEED}: nfev32 {out['nfev32']} nfev64 {out['nfev64']} nfev_batch {nb}")
    print(f"per object: float32 net vs float64 net, pred_pose: max {e.max():.2e} mean {e.mean():.2e}")
    print("whole-batch call vs per-object calls, max |difference| per object:", " ".join(f"{v:.2e}" for v in d))
    assert np.array_equal(out["nfev32"], out["nfev64"]), "an accept / reject decision flips with the net's precision"
    assert all(apart(out["pred_pose_batch"], out["pred_pose32"], oi.B, oi.K)), "whole batch too close to per object"
    assert np.any(out["nfev32"] != nb), "nfev_batch equals every object's nfev"
    save_npz(os.path.join(HERE, "golden_ode_object.npz"), out)


if __name__ == "__main__":
    main()
