"""Float64 restatement of the likelihood right-hand side for the tests (not a product path, not the oracle).

cond_ode_likelihood's divergence_eval (networks/gf_algorithms/samplers.py:54-68) takes
div = eps . grad_x(sum(score * eps)) by reverse mode; rows are independent, so per row this is
eps^T J^T eps = eps^T J eps with J = d score / d x. ``score_div64`` forms J eps in FORWARD mode, as the HIP
kernels do: a tangent pushed through PoseScoreNet.forward (scorenet.py:215-275) next to the primal, with the
primal's ReLU masks (torch's relu' is 0 at 0) and without the bias / pts / t terms. The CPU test holds it to the
reference's autograd result in golden_like_eval (1e-10 relative), so it can stand in for the reference at
other shapes.
"""
import numpy as np
import torch


def _p64(sd):
    from genpose2_amd import weights
    return {k: torch.from_numpy(v.astype(np.float64)) for k, v in weights.head_params(sd).items()}


def score_div64(sd, pts_feat, x, t, eps):
    """pts_feat (R,1024), x (R,9), eps (R,9), one time value t -> (score (R,9), div (R,), margin (R,)) float64.
    margin: min over the 1,280 pose-dependent ReLU units of |pre-activation| / the layer's max |pre-activation|."""
    from genpose2_amd import arch
    p = _p64(sd)
    f = torch.as_tensor(np.asarray(pts_feat, dtype=np.float64))
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    e = torch.as_tensor(np.asarray(eps, dtype=np.float64))
    t = float(t)
    xp = t * p["gfp_w"] * 2.0 * np.pi
    tf = torch.relu(p["te_w"] @ torch.cat([torch.sin(xp), torch.cos(xp)]) + p["te_b"])
    margins = []

    def layer(pre, dpre):
        margins.append((pre.abs() / pre.abs().max()).min(dim=1).values)
        return torch.relu(pre), dpre * (pre > 0)

    a0, da0 = layer(x @ p["pe0_w"].T + p["pe0_b"], e @ p["pe0_w"].T)
    a2, da2 = layer(a0 @ p["pe2_w"].T + p["pe2_b"], da0 @ p["pe2_w"].T)
    out, dout = [], []
    for k in range(3):
        z = f @ p["h1_pts"][k].T + p["h1_t"][k] @ tf + a2 @ p["h1_pose"][k].T + p["h1_b"][k]
        u, du = layer(z, da2 @ p["h1_pose"][k].T)
        out.append(u @ p["h2_w"][k].T + p["h2_b"][k])
        dout.append(du @ p["h2_w"][k].T)
    sig = arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** t
    score = torch.cat(out, 1) / (sig + 1e-7)
    jeps = torch.cat(dout, 1) / (sig + 1e-7)
    div = (e * jeps).sum(1)
    margin = torch.stack(margins, 0).min(dim=0).values
    return score.numpy(), div.numpy(), margin.numpy()
