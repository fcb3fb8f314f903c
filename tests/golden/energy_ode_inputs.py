"""Seeded inputs of the energy agent's ODE fixture (golden_energy_ode), shared by its generator
(make_golden_energy_ode.py) and the tests: the fixture also holds them, and the CPU suite checks that they
regenerate bit for bit. The construction is ode_object_inputs.py's."""
import numpy as np

B, K = 3, 10
T0, STEPS = 0.55, 20
# the generator starts at FIRST_SEED and takes the first seed at which all of its conditions hold: SEED
FIRST_SEED = 521
SEED = 521
SPREAD_SEEDS = 6      # consecutive seeds from SEED over which the reference's own float32 / float64 spread is taken
NEAR_ONE = 0.02       # no error norm of the float64 solve within this of the accept / reject threshold 1
MIN_MEDIAN_ROW = 1e-4  # the fixture seed's float32 free run is in the typical regime (median row error at least this)


def row_errors(pose, pose64):
    """Per row of (R,9) poses: the largest absolute error of the six rotation entries, and the largest error of
    the three translation entries over max |translation64|."""
    a, b = np.asarray(pose, np.float64).reshape(-1, 9), np.asarray(pose64, np.float64).reshape(-1, 9)
    return np.abs(a[:, :6] - b[:, :6]).max(1), np.abs(a[:, 6:] - b[:, 6:]).max(1) / np.abs(b[:, 6:]).max()


def inputs(seed=SEED):
    """B=3 objects x K=10 candidates: 30 rows, two 16-row tiles, the second with 14 rows, tile 0 spanning two
    objects. relu(normal) features scaled per object, the unit normals behind the prior (x0 = prior * sigma(T0)),
    a small pts_center per object."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts_feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pts_feat *= np.asarray([0.5, 1.0, 2.0], np.float32)[:, None]
    prior = rng.standard_normal((B * K, 9)).astype(np.float32)
    pts_center = (0.1 * rng.standard_normal((B, 3))).astype(np.float32)
    return dict(pts_feat=pts_feat, prior=prior, pts_center=pts_center)
