"""Seeded inputs of the likelihood fixtures (golden_like_eval / golden_like_ode), shared by their generator
(make_golden_likelihood.py) and the tests: the fixtures also hold them, and the CPU suite checks that they
regenerate bit for bit."""
import numpy as np

SIGMA_T1 = 0.01 * (50 / 0.01) ** 1.0     # ve_prior's scale at T = 1 (sde.py:30-34)
EVAL_TIMES = (1e-5, 0.01, 0.3, 1.0)
EVAL_B, EVAL_K = 10, 5
ODE_B, ODE_K = 2, 5
KINK_MARGIN = 1e-5                       # rows with a pose-dependent ReLU unit this close to 0 may be excluded
MAX_EXCLUDED = 0.10                      # ... at most this share of all rows


def eval_inputs():
    """B=10 objects with relu(normal) features (as make_golden.gen_heads builds them), K=5 poses each: R=50 rows,
    three full 16-row tiles and a 2-row tail, several objects per tile. eps = prior((R,9)) = randn * sigma(T=1)
    in float32, as cond_ode_likelihood draws it (samplers.py:42)."""
    rng = np.random.Generator(np.random.PCG64(311))
    B, K = EVAL_B, EVAL_K
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pose = rng.normal(size=(B * K, 9)).astype(np.float32)
    pose[:, 6:] *= np.float32(0.3)
    eps_unit = rng.standard_normal((B * K, 9)).astype(np.float32)
    eps = (eps_unit * np.float32(SIGMA_T1)).astype(np.float32)
    return dict(pts_feat=pts_feat, pose=pose, eps=eps, t=np.asarray(EVAL_TIMES, np.float64))


def _gs6(v):
    a, b = v[:, :3], v[:, 3:6]
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b - (a * b).sum(1, keepdims=True) * a
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.concatenate([a, b], 1)


def ode_inputs(pts_center):
    """Poses for B=2 objects x K=5: random Gram-Schmidt-normalised rot6 and 0.05 * normal translations about
    each object's pts_center (camera frame, float32, as pred_func returns them), and the unit normals behind
    eps (the test injects them as NoiseFeed.prior; eps = unit * sigma(T=1))."""
    rng = np.random.Generator(np.random.PCG64(312))
    B, K = ODE_B, ODE_K
    rot = _gs6(rng.normal(size=(B * K, 6)))
    tr = 0.05 * rng.normal(size=(B * K, 3))
    local = np.concatenate([rot, tr], 1).astype(np.float32)
    cam = local.copy()
    cam[:, 6:] = cam[:, 6:] + np.repeat(np.asarray(pts_center, np.float32), K, 0)
    eps_unit = rng.standard_normal((B * K, 9)).astype(np.float32)
    return dict(pose_samples=cam.reshape(B, K, 9), eps_unit=eps_unit)
