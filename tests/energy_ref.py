"""Float64 autograd restatement of the energy model's score for the tests (not a product path, not the oracle).

PoseEnergyNet.forward(return_item='score_and_energy') (networks/gf_algorithms/energynet.py:151-233) with the IP /
score / identical energy and decoupled_rt=False: E = sum_o x_o f_o(x) / sigma(t), score = grad_x E by torch autograd.
The CPU test holds it to the reference's float64 run in golden_energy_score (1e-10 relative), so it can stand in
for the reference at other shapes.
"""
import numpy as np
import torch


def energy_score64(sd, pts_feat, x, t):
    """pts_feat (R,1024), x (R,9), one time value t -> (score (R,9), energy (R,), margin (R,)) float64.
    margin: min over the 1,280 pose-dependent ReLU units of |pre-activation| / the layer's max |pre-activation|
    (like_ref.py's definition)."""
    from genpose2_amd import arch, weights
    p = {k: torch.from_numpy(v.astype(np.float64)) for k, v in weights.head_params(sd).items()}
    f = torch.as_tensor(np.asarray(pts_feat, dtype=np.float64))
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
    t = float(t)
    xp = t * p["gfp_w"] * 2.0 * np.pi
    tf = torch.relu(p["te_w"] @ torch.cat([torch.sin(xp), torch.cos(xp)]) + p["te_b"])
    margins = []

    def relu(pre):
        margins.append((pre.detach().abs() / pre.detach().abs().max()).min(dim=1).values)
        return torch.relu(pre)

    a0 = relu(x @ p["pe0_w"].T + p["pe0_b"])
    a2 = relu(a0 @ p["pe2_w"].T + p["pe2_b"])
    out = []
    for k in range(3):
        u = relu(f @ p["h1_pts"][k].T + p["h1_t"][k] @ tf + a2 @ p["h1_pose"][k].T + p["h1_b"][k])
        out.append(u @ p["h2_w"][k].T + p["h2_b"][k])
    sig = arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** t
    energy = torch.sum(x * (torch.cat(out, 1) / sig), dim=-1)
    score, = torch.autograd.grad(energy, x, grad_outputs=torch.ones_like(energy))
    margin = torch.stack(margins, 0).min(dim=0).values
    return score.numpy(), energy.detach().numpy(), margin.numpy()


def pc_step(x, s, z1, z2, sigma_g, dt, sqrt_dt, snr=0.16):
    """One corrector + predictor update of cond_pc_sampler (samplers.py:143-169) in the dtype of its tensors (the
    GPU test: float32) from a given score s of the entering state x (both (R,9); grad_norm over all R rows):
    -> (x_next, mean_x), before pts_center is added. sigma_g = g(t) of the step, dt / sqrt_dt the step table's."""
    grad_norm = torch.norm(s.reshape(s.shape[0], -1), dim=-1).mean()
    ls = 2 * (snr * float(np.sqrt(9)) / grad_norm) ** 2
    x = x + ls * s + torch.sqrt(2 * ls) * z1
    x[:, :3] /= torch.norm(x[:, :3], dim=-1, keepdim=True)
    x[:, 3:6] /= torch.norm(x[:, 3:6], dim=-1, keepdim=True)
    drift = 0 - sigma_g ** 2 * s
    mean_x = x + drift * dt
    x = mean_x + sigma_g * sqrt_dt * z2
    return gs6(x), mean_x


def gs6(x):
    """normalize_rotation(., 'rot_matrix') (utils/misc.py:327-333, rotation_6d_to_matrix's Gram-Schmidt of the two
    rot6 columns), translation untouched."""
    import torch.nn.functional as F
    a, b = x[:, :3], x[:, 3:6]
    a = F.normalize(a, dim=-1)
    b = F.normalize(b - (a * b).sum(-1, keepdim=True) * a, dim=-1)
    return torch.cat([a, b, x[:, 6:]], dim=-1)
