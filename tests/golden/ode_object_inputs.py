"""Seeded inputs of the per-object ODE fixture (golden_ode_object), shared by its generator
(make_golden_ode_object.py) and the tests: the fixture also holds them, and the CPU suite checks that they
regenerate bit for bit."""
import numpy as np

B, K = 3, 10
T0, STEPS = 0.55, 20
# the generator starts from this seed and raises it until both of its conditions hold (every object's nfev equal
# in float32 and float64; the whole-batch call outside the tolerances of the per-object calls on every object)
SEED = 521


def inputs():
    """B=3 objects x K=10 candidates: 30 rows, so objects straddle the 16-row tiles and the last tile is partial.
    relu(normal) features (as make_golden.gen_heads builds them), scaled per object so that the objects' scores --
    and with them their RK45 error norms and step sequences -- differ; the unit normals behind the prior
    (x0 = prior * sigma(T0)); a small pts_center per object."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pts_feat *= np.asarray([0.5, 1.0, 2.0], np.float32)[:, None]
    prior = rng.standard_normal((B * K, 9)).astype(np.float32)
    pts_center = (0.1 * rng.standard_normal((B, 3))).astype(np.float32)
    return dict(pts_feat=pts_feat, prior=prior, pts_center=pts_center)
