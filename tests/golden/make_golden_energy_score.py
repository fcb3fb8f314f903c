"""Fixtures of the energy model used as a score model, made by running the REFERENCE itself:
PoseEnergyNet.forward(data, return_item='score' | 'score_and_energy') (networks/gf_algorithms/energynet.py:211-233,
the autograd gradient of the IP / score / identical energy) and cond_pc_sampler driven by it (samplers.py:113-177,
GFObjectPose.forward(mode='pc_sample'), posenet.py:338-340).

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/energy_score_inputs.py (seeded). Weights are
weights.synthetic_state_dict("energy", seed=0): the reference zero-initialises the last head layers, so its own
initialisation would give zero heads.

golden_energy_score.npz -- one evaluation, R = 50 rows at t in {1e-5, 0.01, 0.3, 1.0}: score32 / energy32, the
  reference's float32 return_item='score_and_energy'; score64 / energy64, the same with net.double() and float64
  inputs; margin: per row and time, the min over the 1,280 ReLU units that depend on the pose of
  |pre-activation| / that layer's max |pre-activation| in the float64 run (like_ref.py's definition). A unit that
  close to 0 can take the other side under any other rounding, and its mask then moves the gradient: rows under
  energy_score_inputs.KINK_MARGIN may be excluded from a comparison, at most MAX_EXCLUDED_EVAL of all rows.

golden_energy_pc.npz -- cond_pc_sampler with the energy agent on B = 4 x K = 10 rows, T = 2 steps, prior and
  z1 / z2 injected: pred_pose32 / pred_q32 / xs32 (float32, as the reference runs) and pred_pose64 / pred_q64 /
  xs64 (network, state and noise in float64), and margin: per row, the min of the margin above over both score
  evaluations of the float64 run (at most MAX_EXCLUDED_PC of the rows under KINK_MARGIN).

If a count printed here exceeds its cap, the seed in energy_score_inputs.py changes, not the cap.

Usage:  python tests/golden/make_golden_energy_score.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import energy_score_inputs as ei  # noqa: E402
from make_golden_likelihood import POSE_UNITS, save_npz  # noqa: E402
import torch  # noqa: E402


def _hooked(net, store):
    """Appends every forward's pre-activations of the pose-dependent ReLU layers to store[name]."""
    mods = dict(net.pose_score_net.named_modules())
    return [mods[n].register_forward_hook(lambda m, i, o, n=n: store.setdefault(n, []).append(o.detach().clone()))
            for n in POSE_UNITS]


def _margin(pre, call):
    return torch.stack([(pre[n][call].abs() / pre[n][call].abs().max()).min(dim=1).values
                        for n in POSE_UNITS]).min(dim=0).values


def gen_eval(get_config, PoseNet):
    inp = ei.eval_inputs()
    R = ei.EVAL_B * ei.EVAL_K
    feat_rows = np.repeat(inp["pts_feat"], ei.EVAL_K, 0)
    n32 = mg.make_agent(get_config, PoseNet, "energy", "pc", None).net
    n64 = mg.make_agent(get_config, PoseNet, "energy", "pc", None).net.double()
    out = dict(inp)
    s32, e32, s64, e64, mar, flips = [], [], [], [], [], []
    for t in inp["t"]:
        pre32, pre64 = {}, {}
        hooks = _hooked(n32, pre32) + _hooked(n64, pre64)
        data = {"pts_feat": torch.from_numpy(feat_rows), "rgb_feat": None,
                "sampled_pose": torch.from_numpy(inp["pose"].copy()), "t": torch.ones(R).unsqueeze(-1) * float(t)}
        s, e = n32.pose_score_net(data, return_item="score_and_energy")
        data = {"pts_feat": torch.from_numpy(feat_rows).double(), "rgb_feat": None,
                "sampled_pose": torch.from_numpy(inp["pose"]).double(),
                "t": torch.ones(R, dtype=torch.float64).unsqueeze(-1) * float(t)}
        sd_, ed_ = n64.pose_score_net(data, return_item="score_and_energy")
        for h in hooks:
            h.remove()
        flip = torch.stack([((pre32[n][0] > 0) != (pre64[n][0] > 0)).any(dim=1) for n in POSE_UNITS]).any(dim=0)
        s32.append(s.detach().numpy()), e32.append(e.detach().numpy())
        s64.append(sd_.detach().numpy()), e64.append(ed_.detach().numpy())
        mar.append(_margin(pre64, 0).numpy()), flips.append(flip.numpy())
    out.update(score32=np.stack(s32), energy32=np.stack(e32), score64=np.stack(s64), energy64=np.stack(e64),
               margin=np.stack(mar))
    excl = out["margin"] < ei.KINK_MARGIN
    flips = np.stack(flips)
    print("eval: rows under the kink margin", int(excl.sum()), "of", excl.size, "| rows whose float32 masks differ from "
          "float64's", int(flips.sum()), "| of those outside the margin", int((flips & ~excl).sum()))
    assert excl.sum() <= ei.MAX_EXCLUDED_EVAL * excl.size, "too many rows near a ReLU kink: change the seed"
    for j, t in enumerate(inp["t"]):
        sc = np.abs(out["score64"][j]).max()
        e = np.abs(out["score32"][j].astype(np.float64) - out["score64"][j]).max(1) / sc
        k = ~excl[j]
        print(f"  t={t:g}: reference fp32 score error / max|score64| max {e[k].max():.2e} mean {e[k].mean():.2e} "
              f"(all rows: max {e.max():.2e}); max|score64| {sc:.3e}; max|energy32| {np.abs(out['energy32'][j]).max():.3e}")
    save_npz(os.path.join(HERE, "golden_energy_score.npz"), out)


def _pc_run(net, inp, dtype):
    """The reference's repeated-data call of pred_func (posenet_agent.py:510-559) on given features: mode
    'pc_sample', then the quaternion of res, all in `dtype`."""
    from utils.misc import get_rot_matrix
    from utils.transforms.rotation_conversions import matrix_to_quaternion
    B, K, T = ei.PC_B, ei.PC_K, ei.PC_T
    R = B * K
    np_t = np.float64 if dtype == torch.float64 else np.float32
    zs = np.empty((2 * T, R, 9), np_t)
    zs[0::2], zs[1::2] = inp["z1"], inp["z2"]
    data = {"pts": torch.zeros(R, 1, 3, dtype=dtype),
            "pts_feat": torch.from_numpy(np.repeat(inp["pts_feat"], K, 0)).to(dtype), "rgb_feat": None,
            "pts_center": torch.from_numpy(np.repeat(inp["pts_center"], K, 0)).to(dtype)}
    with mg.NoiseFeed(inp["prior"].astype(np_t), zs) as nf, torch.no_grad():
        xs, res = net(data, mode="pc_sample")
        assert nf.i == 2 * T
    q = torch.cat((matrix_to_quaternion(get_rot_matrix(res[:, :-3], "rot_matrix")), res[:, -3:]), dim=-1)
    assert res.dtype == dtype and xs.dtype == dtype
    return res.numpy(), q.numpy(), xs.numpy()


def gen_pc(get_config, PoseNet):
    inp = ei.pc_inputs()
    T = ei.PC_T
    out = dict(inp)
    a32 = mg.make_agent(get_config, PoseNet, "energy", "pc", T)
    assert a32.cfg.pose_mode == "rot_matrix"
    out["pred_pose32"], out["pred_q32"], out["xs32"] = _pc_run(a32.net, inp, torch.float32)
    a64 = mg.make_agent(get_config, PoseNet, "energy", "pc", T)
    net64 = a64.net.double()
    pre64 = {}
    hooks = _hooked(net64, pre64)
    torch.set_default_dtype(torch.float64)     # the sampler's time grid, ones(...) and scalars in float64 too
    try:
        out["pred_pose64"], out["pred_q64"], out["xs64"] = _pc_run(net64, inp, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
        for h in hooks:
            h.remove()
    assert all(len(pre64[n]) == T for n in POSE_UNITS)
    out["margin"] = torch.stack([_margin(pre64, c) for c in range(T)]).min(dim=0).values.numpy()
    excl = out["margin"] < ei.KINK_MARGIN
    print("pc: rows under the kink margin", int(excl.sum()), "of", excl.size)
    assert excl.sum() <= ei.MAX_EXCLUDED_PC * excl.size, "too many rows near a ReLU kink: change the seed"
    e = np.abs(out["pred_pose32"].astype(np.float64) - out["pred_pose64"]).max(1)
    print(f"pc: reference fp32 pred_pose error vs float64: max {e[~excl].max():.2e} mean {e[~excl].mean():.2e} "
          f"(all rows max {e.max():.2e}); max|pred_pose64| {np.abs(out['pred_pose64']).max():.3e}")
    save_npz(os.path.join(HERE, "golden_energy_pc.npz"), out)


def main():
    get_config, PoseNet = mg.import_reference("pc", None)
    gen_eval(get_config, PoseNet)
    gen_pc(get_config, PoseNet)


if __name__ == "__main__":
    main()
