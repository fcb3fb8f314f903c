"""Fixture of the energy agent on the ODE sampler, made by running the REFERENCE itself: cond_ode_sampler
(samplers.py:180-258, GFObjectPose.forward(mode='ode_sample')) with the EnergyNet, whose score is the autograd
gradient of its energy (energynet.py:211-233).

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/energy_ode_inputs.py (seeded). Weights are
weights.synthetic_state_dict("energy", seed=0).

The energy's gradient is discontinuous at ReLU kinks: a unit that takes the other side in one row moves the
error norm, with it the step size, and with that every row. The reference's float32 net therefore lands only
about 1e-3 from its own net.double() run, and no whole-solve parity to float32 rounding exists. The fixture
holds what can be checked instead.

golden_energy_ode.npz -- B = 3 x K = 10 rows, T0 = 0.55, steps = 20, prior injected:
  free runs: pred_pose32 / pred_q32 / nfev32 (the float32 net, as the reference runs); pred_pose64 / nfev64 and the
    pre-denoise state y64 = res.y[:, -1] (net.double(); state, x0 and the solver's scalars are the reference's
    own); trace64 = [t, h, error norm] of every attempt of the float64 solve;
  forced runs: the float32 net stepped through trace64's (t, h) sequence, accepting where norm64 < 1 (a plain
    loop over genpose2_amd.ode.NumpyRk45: rhs0, attempt, accept): norm32_forced per attempt and the final state
    y32_forced. The float64 net through the same loop must reproduce trace64's norms to 1e-12 (asserted here);
  spread: over SPREAD_SEEDS consecutive seeds from the fixture's, the largest row error of the float32 free run
    against the float64 one -- spread_rot (rotation entries, absolute), spread_trans (translation over
    max |t64|) -- and nfev_lo / nfev_hi, the range of nfev over those runs, float32 and float64.

A seed is taken if: nfev32 == nfev64; no trace64 norm within NEAR_ONE of 1; the forced float32 run takes the
float64 run's accept / reject decisions; the median row error (rotation) of its float32 free run is at least
MIN_MEDIAN_ROW (the typical regime: a lucky seed must not become the yardstick). Otherwise the next seed is tried,
from FIRST_SEED; the seed taken must be energy_ode_inputs.SEED (update it there if the search ends elsewhere).
Seed 521 is taken: its norm nearest 1 is 0.973, 2.7 % away.

Usage:  python tests/golden/make_golden_energy_ode.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import energy_ode_inputs as ei  # noqa: E402
import ode_object_inputs as oi  # noqa: E402
from make_golden_likelihood import save_npz  # noqa: E402
from make_golden_ode_object import _ode_run, _to_double  # noqa: E402
from make_ode_trace import _trace_patch  # noqa: E402
import torch  # noqa: E402

from genpose2_amd import ode  # noqa: E402

assert (oi.B, oi.K, oi.T0, oi.STEPS) == (ei.B, ei.K, ei.T0, ei.STEPS)   # _ode_run reads K and T0 there
R = ei.B * ei.K
EPS = 1e-5


def free_run(net, inp):
    """One mode='ode_sample' call on all rows -> dict(pose, q, nfev, y = res.y[:, -1], trace)."""
    import networks.gf_algorithms.samplers as smp
    orig = smp.integrate.solve_ivp
    seen, log = {}, []

    def keeping(*a, **k):
        res = orig(*a, **k)
        seen["y"] = np.array(res.y[:, -1], dtype=np.float64)
        return res

    smp.integrate.solve_ivp = keeping
    undo = _trace_patch(log)
    try:
        pose, q, nfev = _ode_run(net, inp, slice(0, R))
    finally:
        undo()
        smp.integrate.solve_ivp = orig
    return dict(pose=pose, q=q, nfev=nfev, y=seen["y"], trace=np.asarray(log, np.float64))


def ode_fun(net, inp):
    """cond_ode_sampler's ode_func (samplers.py:210-219) over `net`, as a fun(t, y) for NumpyRk45."""
    data = {"pts": torch.zeros(R, 1, 3), "pts_feat": torch.from_numpy(np.repeat(inp["pts_feat"], ei.K, 0)),
            "rgb_feat": None}
    feat = data["pts_feat"]
    sde_coeff = net.sde_fn

    def fun(t, x):
        xt = torch.tensor(x.reshape(-1, 9), dtype=torch.float32)
        drift, diffusion = sde_coeff(torch.tensor(t))
        data["pts_feat"] = feat                      # the float64 net's pre-hook converts what it is handed
        data["sampled_pose"] = xt
        data["t"] = torch.ones(R).unsqueeze(-1) * t
        with torch.no_grad():
            s = net(data, mode="score")
        return drift.numpy() - 0.5 * (diffusion.numpy() ** 2) * s.detach().numpy().reshape((-1,))
    return fun


def forced_run(net, inp, trace):
    """`net` stepped through trace's (t, h), accepting where trace's norm < 1 -> (norms, final state)."""
    sig = 0.01 * (50 / 0.01) ** ei.T0
    x0 = (torch.from_numpy(inp["prior"]) * sig).reshape(-1).numpy()   # prior((R,9), T) in float32 (sde.py:30-34)
    be = ode.NumpyRk45(ode_fun(net, inp), x0)
    be.rhs0(ei.T0)                                   # t0 is a Python float (ivp.py), later times NumPy float64
    norms = []
    for t, h, n64 in trace:
        t, h = np.float64(t), np.float64(h)
        norms.append(float(be.attempt(t, h)))
        if n64 < 1:
            be.accept(t, t + h)
    return np.asarray(norms, np.float64), np.array(be.y, dtype=np.float64)


def main():
    get_config, PoseNet = mg.import_reference("ode", ei.STEPS)
    a32 = mg.make_agent(get_config, PoseNet, "energy", "ode", ei.STEPS)
    assert a32.cfg.pose_mode == "rot_matrix"
    net32 = a32.net
    net64 = mg.make_agent(get_config, PoseNet, "energy", "ode", ei.STEPS).net.double()
    net64.register_forward_pre_hook(_to_double)
    runs = {}

    def both(seed):
        if seed not in runs:
            inp = ei.inputs(seed)
            runs[seed] = (inp, free_run(net32, inp), free_run(net64, inp))
        return runs[seed]

    for seed in range(ei.FIRST_SEED, ei.FIRST_SEED + 32):
        inp, f32, f64 = both(seed)
        tr = f64["trace"]
        rot, _ = ei.row_errors(f32["pose"], f64["pose"])
        near = np.abs(tr[:, 2] - 1).min()
        print(f"seed {seed}: nfev32 {f32['nfev']} nfev64 {f64['nfev']} | norm nearest 1: {near:.3f} off | float32 "
              f"free run rotation row error max {rot.max():.2e} median {np.median(rot):.2e}", flush=True)
        if f32["nfev"] != f64["nfev"] or near < ei.NEAR_ONE or np.median(rot) < ei.MIN_MEDIAN_ROW:
            continue
        n32, y32 = forced_run(net32, inp, tr)
        if not np.array_equal(n32 < 1, tr[:, 2] < 1):
            print("  the forced float32 run decides an attempt otherwise")
            continue
        break
    else:
        raise AssertionError("no seed meets the fixture's conditions")
    assert seed == ei.SEED, f"set energy_ode_inputs.SEED = {seed}"
    n64, y64f = forced_run(net64, inp, tr)
    self_rel = np.abs(n64 - tr[:, 2]).max() / tr[:, 2].min()
    print(f"forced float64 run vs the free one: norms differ by {np.abs(n64 / tr[:, 2] - 1).max():.2e} relative")
    assert np.abs(n64 / tr[:, 2] - 1).max() <= 1e-12, self_rel
    assert 2 + 6 * len(tr) == f64["nfev"]
    rel32 = np.abs(n32 / tr[:, 2] - 1)
    er = np.abs(y32 - f64["y"]).reshape(R, 9).max(1)
    print(f"forced float32 run: |norm / norm64 - 1| max {rel32.max():.2e}; final state row error vs y64: median "
          f"{np.median(er):.2e} p90 {np.percentile(er, 90):.2e} max {er.max():.2e}")
    rots, trs, nfevs = [], [], []
    for s in range(seed, seed + ei.SPREAD_SEEDS):
        _, a, b = both(s)
        r, t = ei.row_errors(a["pose"], b["pose"])
        rots.append(r.max()), trs.append(t.max()), nfevs.extend([a["nfev"], b["nfev"]])
        print(f"spread seed {s}: rotation {r.max():.2e} translation {t.max():.2e} nfev {a['nfev']} / {b['nfev']}")
    out = dict(inp)
    out.update(seed=np.int64(seed), pred_pose32=f32["pose"], pred_q32=f32["q"], nfev32=np.int64(f32["nfev"]),
               pred_pose64=f64["pose"], nfev64=np.int64(f64["nfev"]), y64=f64["y"], trace64=tr,
               norm32_forced=n32, y32_forced=y32, norm64_forced=n64, spread_rot=np.float64(max(rots)),
               spread_trans=np.float64(max(trs)), nfev_lo=np.int64(min(nfevs)), nfev_hi=np.int64(max(nfevs)))
    print(f"spread: rotation {max(rots):.2e} translation {max(trs):.2e} nfev {min(nfevs)} .. {max(nfevs)}")
    save_npz(os.path.join(HERE, "golden_energy_ode.npz"), out)


if __name__ == "__main__":
    main()
