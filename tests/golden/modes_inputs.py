"""Inputs of the pose-hypotheses fixture (golden_modes.npz): candidates as a symmetric object's fall.

NumPy only. ``make_golden_modes.py`` calls ``build_inputs`` with the seeds and the noise it searches, runs the
reference's statements on the result and stores both; the tests read the stored arrays.

Per object the kept set (the ``KEEP`` candidates of highest rotation energy) is built from a random base rotation
composed with elements of ``SYMMETRY`` (180-degree flips about the base's axes and a 90-degree turn about z), each
member with a small random rotation on top, plus outliers at random rotations. The other candidates are random
and every one of their rotation energies lies below every kept one. The translation energies are independent of
the rotation energies, so the set kept by translation energy is a different one.
"""
from __future__ import annotations

import numpy as np

B, K, KEEP = 8, 50, 20
EPS, MIN_SAMPLES = 0.05, 3          # clustering_eps, int(0.1667 * 20): the shipped configuration
MAX_SLOTS = 8

# (cluster sizes, outliers, quantised energies)
OBJECTS = (
    ((20,), 0, False),
    ((11, 7), 2, False),
    ((8, 6, 4), 2, False),
    ((6, 5, 4, 3), 2, False),
    ((9, 9), 2, False),               # a count tie between the two largest
    ((4, 4, 4, 4, 4), 0, False),      # more clusters than M = 4
    ((2, 2, 2, 2), 12, False),        # every point noise at min_samples 3
    ((10, 6), 4, True),               # quantised energies: rank ties go by candidate index
)


def _rotvec(v: np.ndarray) -> np.ndarray:
    """Rodrigues: rotation vector (3,) -> matrix (3,3), float64."""
    th = float(np.linalg.norm(v))
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def random_rotation(rng: np.random.Generator) -> np.ndarray:
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


SYMMETRY = (np.eye(3), _rotvec(np.array([np.pi, 0, 0])), _rotvec(np.array([0, np.pi, 0])),
            _rotvec(np.array([0, 0, np.pi])), _rotvec(np.array([0, 0, np.pi / 2])))


def small_rotation(rng: np.random.Generator, noise_deg: float) -> np.ndarray:
    return _rotvec(rng.normal(scale=np.deg2rad(noise_deg), size=3))


def build_object(seed: int, sizes, outliers: int, quantised: bool, noise_deg: float):
    """-> pose (K,9) float32, energy (K,2) float32, base (3,3) float64."""
    assert sum(sizes) + outliers == KEEP and len(sizes) <= len(SYMMETRY)
    rng = np.random.default_rng(seed)
    base = random_rotation(rng)
    kept = [base @ SYMMETRY[m] @ small_rotation(rng, noise_deg) for m, n in enumerate(sizes) for _ in range(n)]
    kept += [random_rotation(rng) for _ in range(outliers)]
    rot = np.stack(kept + [random_rotation(rng) for _ in range(K - KEEP)])
    where = rng.permutation(K)                      # candidate index of each of the K rotations above
    pose = np.zeros((K, 9), np.float32)
    pose[where, :3] = rot[:, :, 0]
    pose[where, 3:6] = rot[:, :, 1]
    pose[:, 6:] = rng.normal(scale=0.3, size=(K, 3))
    energy = np.zeros((K, 2), np.float32)
    if quantised:
        energy[where[:KEEP], 0] = rng.integers(2, 5, size=KEEP) * 0.25       # 0.5, 0.75, 1.0
        energy[where[KEEP:], 0] = rng.integers(-4, 2, size=K - KEEP) * 0.25  # -1.0 .. 0.25
        energy[:, 1] = rng.integers(-4, 5, size=K) * 0.25
    else:
        energy[where[:KEEP], 0] = rng.uniform(0.5, 1.0, size=KEEP)
        energy[where[KEEP:], 0] = rng.uniform(-1.0, 0.25, size=K - KEEP)
        energy[:, 1] = rng.normal(size=K)
    return pose, energy, base


def build_inputs(seeds, noise_deg):
    """seeds, noise_deg: one per object -> pred_pose (B,K,9), pred_energy (B,K,2), bases (B,3,3)."""
    out = [build_object(int(s), *OBJECTS[b], float(noise_deg[b])) for b, s in enumerate(seeds)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


def prev_rotation(seed: int, mode_rot: np.ndarray, off_deg: float = 3.0) -> np.ndarray:
    """A previous-frame rotation ``off_deg``-ish degrees off a mode's rotation, float32 (3,3)."""
    return (mode_rot.astype(np.float64) @ small_rotation(np.random.default_rng(seed), off_deg)).astype(np.float32)
