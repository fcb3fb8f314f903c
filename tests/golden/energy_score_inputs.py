"""Seeded inputs of the energy-gradient fixtures (golden_energy_score / golden_energy_pc), shared by their generator
(make_golden_energy_score.py) and the tests: the fixtures also hold them, and the CPU suite checks that they
regenerate bit for bit."""
import numpy as np

EVAL_TIMES = (1e-5, 0.01, 0.3, 1.0)
EVAL_B, EVAL_K = 10, 5
PC_B, PC_K, PC_T = 4, 10, 2
KINK_MARGIN = 1e-5                       # rows with a pose-dependent ReLU unit this close to 0 may be excluded
MAX_EXCLUDED_EVAL = 0.10                 # ... at most this share of the eval fixture's (time, row) pairs
MAX_EXCLUDED_PC = 0.25                   # ... and of the PC fixture's rows (two score evaluations each)


def eval_inputs():
    """B=10 objects with relu(normal) features (as make_golden.gen_heads builds them), K=5 poses each: R=50 rows,
    three full 16-row tiles and a 2-row tail, several objects per tile."""
    rng = np.random.Generator(np.random.PCG64(411))
    B, K = EVAL_B, EVAL_K
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pose = rng.normal(size=(B * K, 9)).astype(np.float32)
    pose[:, 6:] *= np.float32(0.3)
    return dict(pts_feat=pts_feat, pose=pose, t=np.asarray(EVAL_TIMES, np.float64))


def pc_inputs():
    """B=4 objects x K=10 candidates (tiles of 16, 16 and 8 rows), T=2 PC steps: relu(normal) features, the unit
    normals behind the prior (x0 = prior * sigma(T=1)), the corrector / predictor draws z1 / z2 (T,R,9) of every
    step, and a small pts_center per object."""
    rng = np.random.Generator(np.random.PCG64(425))
    B, K, T = PC_B, PC_K, PC_T
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    prior = rng.standard_normal((B * K, 9)).astype(np.float32)
    z1 = rng.standard_normal((T, B * K, 9)).astype(np.float32)
    z2 = rng.standard_normal((T, B * K, 9)).astype(np.float32)
    pts_center = (0.1 * rng.standard_normal((B, 3))).astype(np.float32)
    return dict(pts_feat=pts_feat, prior=prior, z1=z1, z2=z2, pts_center=pts_center)
