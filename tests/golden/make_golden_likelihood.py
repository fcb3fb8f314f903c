"""Fixtures of the likelihood mode, GFObjectPose.forward(data, mode="likelihood") (networks/posenet.py:278-292,
cond_ode_likelihood in networks/gf_algorithms/samplers.py:14-110), made by running the REFERENCE itself.

Runs only where the reference is present (it imports it read-only through make_golden.import_reference); only
data is written. Inputs come from tests/golden/like_inputs.py (seeded).

golden_like_eval.npz -- one right-hand-side evaluation, R = 50 rows at t in {1e-5, 0.01, 0.3, 1.0}:
  score32 / div32: the reference's score and divergence_eval (samplers.py:54-68: reverse-mode
  eps . grad_x(sum(score * eps))) in float32, as it runs them; score64 / div64: the same with net.double() and
  float64 inputs (make_ode_trace.run_ref64's convention: the float32 casts removed); margin: per row and time, the
  min over the 1,280 ReLU units that depend on the pose (pose_encoder.0 / .2, fusion_tail_*.0) of
  |pre-activation| / that layer's max |pre-activation| in the float64 run. A unit that close to 0 can take the
  other side under any other rounding, and its mask moves div by ~1/256 of a term: rows under
  like_inputs.KINK_MARGIN may be excluded from a comparison, at most like_inputs.MAX_EXCLUDED of all rows
  (asserted here; the rows where the reference's own float32 masks differ from its float64 masks are printed).

golden_like_ode.npz -- the whole mode on B = 2 objects (config-21 clouds through the reference's encoder) x K = 5
  poses: ll32 (the reference as is), ll64 (cond_ode_likelihood restated in float64), their nfev, and ll32_p1 / ll32_p2:
  the reference in float32 with pts_feat scaled by 1 + 2e-7 / 1 - 3e-7 -- independently rounded samples of the
  reference itself (the solve is chaotic at solver-tolerance scale).

Usage:  python tests/golden/make_golden_likelihood.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import like_inputs as li  # noqa: E402
import torch  # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order: a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def divergence_eval(net, data, epsilon):
    """samplers.py:54-68, statement by statement (it is a closure of cond_ode_likelihood there)."""
    with torch.enable_grad():
        data["sampled_pose"].requires_grad_(True)
        score = net(data)
        score_energy = torch.sum(score * epsilon)
        grad_score_energy = torch.autograd.grad(score_energy, data["sampled_pose"])[0]
    return score.detach(), torch.sum(grad_score_energy * epsilon, dim=-1).detach()


POSE_UNITS = ("pose_encoder.0", "pose_encoder.2", "fusion_tail_rot_x.0", "fusion_tail_rot_y.0", "fusion_tail_trans.0")


def _hooked(net, store):
    mods = dict(net.pose_score_net.named_modules())
    return [mods[n].register_forward_hook(lambda m, i, o, n=n: store.__setitem__(n, o.detach().clone()))
            for n in POSE_UNITS]


def gen_eval(get_config, PoseNet):
    inp = li.eval_inputs()
    R = li.EVAL_B * li.EVAL_K
    feat_rows = np.repeat(inp["pts_feat"], li.EVAL_K, 0)
    a32 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    a64 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    n32, n64 = a32.net, a64.net.double()
    out = dict(inp)
    s32, d32, s64, d64, mar, flips = [], [], [], [], [], []
    for t in inp["t"]:
        pre32, pre64 = {}, {}
        h32, h64 = _hooked(n32, pre32), _hooked(n64, pre64)
        # float32 as ode_func feeds the model (samplers.py:83-89): float32 poses, t = ones(R, 1) * t
        data = {"pts_feat": torch.from_numpy(feat_rows), "rgb_feat": None,
                "sampled_pose": torch.from_numpy(inp["pose"].copy()), "t": torch.ones(R).unsqueeze(-1) * float(t)}
        s, d = divergence_eval(n32, data, torch.from_numpy(inp["eps"]))
        data = {"pts_feat": torch.from_numpy(feat_rows).double(), "rgb_feat": None,
                "sampled_pose": torch.from_numpy(inp["pose"]).double(),
                "t": torch.ones(R, dtype=torch.float64).unsqueeze(-1) * float(t)}
        sd_, dd_ = divergence_eval(n64, data, torch.from_numpy(inp["eps"]).double())
        for h in h32 + h64:
            h.remove()
        m = torch.stack([(pre64[n].abs() / pre64[n].abs().max()).min(dim=1).values for n in POSE_UNITS]).min(dim=0).values
        flip = torch.stack([((pre32[n] > 0) != (pre64[n] > 0)).any(dim=1) for n in POSE_UNITS]).any(dim=0)
        s32.append(s.numpy()), d32.append(d.numpy()), s64.append(sd_.numpy()), d64.append(dd_.numpy())
        mar.append(m.numpy()), flips.append(flip.numpy())
    out.update(score32=np.stack(s32), div32=np.stack(d32), score64=np.stack(s64), div64=np.stack(d64),
               margin=np.stack(mar))
    excl = out["margin"] < li.KINK_MARGIN
    flips = np.stack(flips)
    print("eval: rows under the kink margin", int(excl.sum()), "of", excl.size, "| rows whose float32 masks differ from "
          "float64's", int(flips.sum()), "| of those outside the margin", int((flips & ~excl).sum()))
    assert excl.sum() <= li.MAX_EXCLUDED * excl.size, "too many rows near a ReLU kink for the comparison"
    for j, t in enumerate(inp["t"]):
        sc = np.abs(out["div64"][j]).max()
        e = np.abs(out["div32"][j].astype(np.float64) - out["div64"][j]) / sc
        k = ~excl[j]
        print(f"  t={t:g}: reference fp32 div error / max|div64| max {e[k].max():.2e} mean {e[k].mean():.2e} "
              f"(all rows: max {e.max():.2e}); max|div64| {sc:.3e}")
    save_npz(os.path.join(HERE, "golden_like_eval.npz"), out)


def _features(agent, d, double):
    import networks.pts_encoder.pointnet2_utils.pointnet2.pointnet2_utils as pu
    net = agent.net.double() if double else agent.net
    if not double:
        with torch.no_grad():
            return net, net(dict(d), mode="pts_feature")
    saved = (pu.furthest_point_sample, pu.gather_operation, pu.ball_query, pu.grouping_operation)
    fps0, bq0 = pu.furthest_point_sample, pu.ball_query
    pu.furthest_point_sample = lambda xyz, n: fps0(xyz.float(), n)
    pu.ball_query = lambda r, ns, xyz, nxyz: bq0(r, ns, xyz.float(), nxyz.float())
    pu.gather_operation = lambda f, i: torch.gather(f, 2, i.long().unsqueeze(1).expand(-1, f.shape[1], -1))
    pu.grouping_operation = lambda f, i: torch.gather(
        f, 2, i.long().reshape(i.shape[0], 1, -1).expand(-1, f.shape[1], -1)).reshape(f.shape[0], f.shape[1], *i.shape[1:])
    try:
        with torch.no_grad():
            return net, net({"pts": d["pts"].double()}, mode="pts_feature")
    finally:
        pu.furthest_point_sample, pu.gather_operation, pu.ball_query, pu.grouping_operation = saved


def _counted(fn):
    """Runs fn() with solve_ivp's right-hand side counted and its result kept: (fn(), nfev, res)."""
    import networks.gf_algorithms.samplers as smp
    calls, keep = {"n": 0}, {}
    orig = smp.integrate.solve_ivp

    def counting(fun, *a, **k):
        def f(t, y):
            calls["n"] += 1
            return fun(t, y)
        keep["res"] = orig(f, *a, **k)
        return keep["res"]
    smp.integrate.solve_ivp = counting
    try:
        r = fn()
    finally:
        smp.integrate.solve_ivp = orig
    return r, calls["n"], keep["res"]


def run_ll32(net, feat_rows, pose_rows, eps_unit):
    """The reference as is: forward(data, mode="likelihood") with prior((R,9)) fed the recorded normals."""
    R = pose_rows.shape[0]
    data = {"pts": torch.zeros(R, 1, 3), "pts_feat": feat_rows, "rgb_feat": None,
            "sampled_pose": torch.from_numpy(pose_rows.copy())}
    with mg.NoiseFeed(eps_unit, np.zeros((0,), np.float32)):
        ll, nfev, res = _counted(lambda: net(data, mode="likelihood"))
    return ll.numpy().astype(np.float64), nfev, res


def run_ll64(net, feat_rows, pose_rows, eps_unit):
    """cond_ode_likelihood (samplers.py:25-110) with the network in float64 and the float32 casts removed."""
    import scipy.integrate as si
    from networks.gf_algorithms.samplers import global_prior_likelihood
    R = pose_rows.shape[0]
    epsilon = (torch.from_numpy(eps_unit) * li.SIGMA_T1).double()     # the reference's float32 draw, exactly
    dd = {"pts_feat": feat_rows, "rgb_feat": None}
    calls = {"n": 0}

    def ode_func(t, inp):
        calls["n"] += 1
        x = torch.tensor(inp[:-R].reshape(-1, 9), dtype=torch.float64)
        drift, diffusion = net.sde_fn(torch.tensor(t))
        dd["sampled_pose"] = x
        dd["t"] = torch.ones(R, dtype=torch.float64).unsqueeze(-1) * t
        score, div = divergence_eval(net, dd, epsilon)
        c = drift.numpy() - 0.5 * (diffusion.numpy() ** 2)
        return np.concatenate([c * score.numpy().reshape(-1), c * div.numpy().reshape(-1)], axis=0)
    init = np.concatenate([pose_rows.astype(np.float64).reshape(-1), np.zeros((R,))], axis=0)
    res = si.solve_ivp(ode_func, (1e-5, 1.0), init, rtol=1e-5, atol=1e-5, method="RK45")
    zp = torch.tensor(res.y[:, -1])
    z, delta = zp[:-R].reshape(R, 9), zp[-R:]
    _, sigma_max = net.marginal_prob_fn(None, torch.tensor(1.0, dtype=torch.float64))
    ll = (global_prior_likelihood(z, sigma_max) + delta) / np.log(2)
    return ll.numpy(), calls["n"], res


def gen_ode(get_config, PoseNet):
    B, K = li.ODE_B, li.ODE_K
    d = mg.batch(21, B, 1024)
    inp = li.ode_inputs(d["pts_center"].numpy())
    # the pose rows the model sees: pts_center subtracted from the camera-frame samples in float32, as
    # get_energy does (posenet_agent.py:664-668)
    rows = torch.from_numpy(inp["pose_samples"].reshape(B * K, 9).copy())
    rows[:, -3:] -= d["pts_center"].unsqueeze(1).repeat(1, K, 1).view(B * K, -1)
    rows = rows.numpy()
    a32 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    net32, feat32 = _features(a32, d, False)
    f32_rows = feat32.unsqueeze(1).repeat(1, K, 1).view(B * K, -1)
    out = dict(pts=d["pts"].numpy(), pts_center=d["pts_center"].numpy(), pts_feat=feat32.numpy(), **inp)
    ll, nfev, res = run_ll32(net32, f32_rows, rows, inp["eps_unit"])
    out.update(ll32=ll.reshape(B, K), nfev32=np.int64(nfev), status32=np.int64(res.status))
    print("ode: ll32", ll, "nfev", nfev, "status", res.status, flush=True)
    for tag, s in (("p1", 1 + 2e-7), ("p2", 1 - 3e-7)):
        llp, nf, rs = run_ll32(net32, (f32_rows * np.float32(s)).contiguous(), rows, inp["eps_unit"])
        out[f"ll32_{tag}"] = llp.reshape(B, K)
        out[f"nfev32_{tag}"] = np.int64(nf)
        print(f"ode: ll32_{tag} nfev", nf, "status", rs.status, flush=True)
    a64 = mg.make_agent(get_config, PoseNet, "score", "ode", None)
    net64, feat64 = _features(a64, d, True)
    ll64, nfev64, res64 = run_ll64(net64, feat64.unsqueeze(1).repeat(1, K, 1).view(B * K, -1), rows, inp["eps_unit"])
    out.update(ll64=ll64.reshape(B, K), nfev64=np.int64(nfev64), status64=np.int64(res64.status),
               z64=res64.y[:-B * K, -1].reshape(B, K, 9))
    for k in ("ll32", "ll32_p1", "ll32_p2"):
        e = np.abs(out[k] - out["ll64"])
        print(f"ode: |{k} - ll64| max {e.max():.3f} mean {e.mean():.3f}")
    print("ode: nfev64", nfev64, "status", res64.status, "| |ll64| range", np.abs(ll64).min(), np.abs(ll64).max())
    save_npz(os.path.join(HERE, "golden_like_ode.npz"), out)


def main():
    get_config, PoseNet = mg.import_reference("ode", None)
    gen_eval(get_config, PoseNet)
    gen_ode(get_config, PoseNet)


if __name__ == "__main__":
    main()
