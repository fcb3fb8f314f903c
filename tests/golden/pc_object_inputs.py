"""Seeded inputs of the per-object PC fixture (golden_pc_object), shared by its generator (make_golden_pc_object.py)
and the tests: the fixture also holds them, and the CPU suite checks that they regenerate bit for bit."""
import numpy as np

B, K, T = 3, 10, 20
SEED = 521


def inputs():
    """B=3 objects x K=10 candidates, T=20 PC steps: 30 rows, so objects straddle the 16-row tiles and the last tile
    is partial. relu(normal) features (as make_golden.gen_heads builds them), scaled per object so that the objects'
    score norms -- and with them the per-object and the whole-batch step sizes -- differ; the unit normals behind
    the prior (x0 = prior * sigma(T=1)); the corrector / predictor draws z1 / z2 (T,R,9) of every step; a small
    pts_center per object."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pts_feat *= np.asarray([0.5, 1.0, 2.0], np.float32)[:, None]
    prior = rng.standard_normal((B * K, 9)).astype(np.float32)
    z1 = rng.standard_normal((T, B * K, 9)).astype(np.float32)
    z2 = rng.standard_normal((T, B * K, 9)).astype(np.float32)
    pts_center = (0.1 * rng.standard_normal((B, 3))).astype(np.float32)
    return dict(pts_feat=pts_feat, prior=prior, z1=z1, z2=z2, pts_center=pts_center)
