"""Seeded inputs of the object-coupled likelihood fixture (golden_like_object), shared by its generator
(make_golden_like_object.py) and the tests: the fixture also holds them, and the CPU suite checks that they
regenerate bit for bit."""
import numpy as np

from like_inputs import _gs6

B, K = 3, 7                              # 21 rows: object 2 straddles the 16-row tile boundary, the last tile is partial
CONFIG_ID, N_POINTS = 21, 1024
CLOUD_SCALE = (1.0, 0.7, 1.4)            # each object's cloud is scaled about the origin: solves of different lengths
SEED = 313


def scale_clouds(pts):
    """(B,N,3) float32 clouds -> each times its CLOUD_SCALE, in float32."""
    s = np.asarray(CLOUD_SCALE, np.float32).reshape(B, 1, 1)
    return (np.asarray(pts, np.float32) * s).astype(np.float32)


def pose_inputs(pts_center):
    """like_inputs.ode_inputs at B=3 x K=7: random Gram-Schmidt-normalised rot6 and 0.05 * normal translations
    about each object's pts_center (camera frame, float32, as pred_func returns them), and the unit normals behind
    eps (the tests inject them as NoiseFeed.prior; eps = unit * sigma(T=1))."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    rot = _gs6(rng.normal(size=(B * K, 6)))
    tr = 0.05 * rng.normal(size=(B * K, 3))
    local = np.concatenate([rot, tr], 1).astype(np.float32)
    cam = local.copy()
    cam[:, 6:] = cam[:, 6:] + np.repeat(np.asarray(pts_center, np.float32), K, 0)
    eps_unit = rng.standard_normal((B * K, 9)).astype(np.float32)
    return dict(pose_samples=cam.reshape(B, K, 9), eps_unit=eps_unit)
