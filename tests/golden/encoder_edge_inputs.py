"""Seeded edge-case point clouds for the point encoders (tests/test_cpu_encoder_edge.py keeps them adversarial with
the oracle alone; tests/test_gpu_encoder_edge.py runs the device encoders on them). Nothing binary is committed:
every cloud is regenerated from (kind, N, seed) wherever it is needed.

The encoder's ball radii are 0.01/0.02, 0.02/0.04, 0.04/0.08, 0.08/0.16 m with 16/32 samples (arch.RADII,
arch.NSAMPLES), over 512 / 256 / 128 / 64 FPS centroids. Each kind drives the ball query into one of its corners:

lattice   integer grid of 12^3 cells, 1 cm pitch: FPS ties and duplicate points at every level, point-centroid
          distances exactly ON a radius at levels 1-3, balls of exactly nsample hits.
sparse    an object cloud blown up 6x: nearly every level-0 ball holds its centroid alone (all padding).
dense     an object cloud shrunk to 4 %: every ball of every level is full within the first 64-point block,
          so the scan leaves early everywhere.
mixed     up to 256 points blown up 5x, the rest shrunk to 3 % about the mean, permuted: half the level-0 balls
          are full and most others hold one point, and both kinds meet among the 32 centroids of one workgroup
          (FPS visits the spread points first, so they meet where its order crosses into the blob).
dup       the last two thirds of the cloud repeat the first two thirds (exact duplicates).
clusters  groups of 20 points within +-2 mm of centres in a 0.6 m box: the 16-sample radius fills while the
          32-sample radius stays short; plus six planted points that put, for each level-0 radius, one neighbour
          exactly on the radius (excluded: the test is d2 < r2) and one a single ulp inside it.
"""
from __future__ import annotations

import numpy as np

KINDS = ("lattice", "sparse", "dense", "mixed", "dup", "clusters")
F32 = np.float32


def _object(seed: int, n: int) -> np.ndarray:
    from genpose2_amd import synthetic
    return synthetic.object_cloud(seed, n)


def planted() -> np.ndarray:
    """Six points: two centroids-to-be at x = 0 and, for radius r in (0.01, 0.02), a neighbour at x = fl(r)
    (d2 = fl(r) * fl(r) = r2 exactly: outside) and one at x = -pred(fl(r)) (one ulp inside)."""
    out = []
    for r, y in ((0.01, 0.5), (0.02, -0.5)):
        rf = F32(r)
        out += [(F32(0), y, 0.5), (rf, y, 0.5), (-np.nextafter(rf, F32(0)), y, 0.5)]
    return np.asarray(out, F32)


def cloud(kind: str, n: int, seed: int) -> np.ndarray:
    """(n, 3) float32 cloud of `kind` (KINDS)."""
    rng = np.random.Generator(np.random.PCG64([seed, KINDS.index(kind)]))
    if kind == "lattice":
        p = rng.integers(0, 12, size=(n, 3)).astype(F32) * F32(0.01) + np.asarray([0.1, -0.2, 0.7], F32)
    elif kind == "sparse":
        p = _object(seed, n) * F32(6)
    elif kind == "dense":
        p = _object(seed, n) * F32(0.04) + np.asarray([0, 0, 0.5], F32)
    elif kind == "mixed":
        o = _object(seed, n)
        h = n - min(n // 2, 256)   # at most 256 spread points, so FPS keeps 256 centroids inside the blob at any n
        mean = o.mean(axis=0, dtype=np.float64).astype(F32)
        p = np.concatenate([(o[:h] - mean) * F32(0.03) + mean, o[h:] * F32(5)])[rng.permutation(n)]
    elif kind == "dup":
        p = _object(seed, n).copy()
        t = n // 3
        p[t:] = p[: n - t]
    elif kind == "clusters":
        pl = planted()
        k = n - len(pl)
        centres = rng.uniform(-0.3, 0.3, size=(-(-k // 20), 3)) + np.asarray([0, 0, 0.8])
        body = np.repeat(centres, 20, axis=0)[:k] + rng.uniform(-0.002, 0.002, size=(k, 3))
        p = np.concatenate([body.astype(F32), pl])[rng.permutation(n)]
    else:
        raise ValueError(f"unknown cloud kind {kind!r}")
    p = np.ascontiguousarray(p, F32)
    assert p.shape == (n, 3)
    return p


def batch(spec, n: int) -> np.ndarray:
    """(B, n, 3): one object per (kind, seed) of `spec`."""
    return np.stack([cloud(k, n, s) for k, s in spec])


def dist2(centroids: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """(M, N) float32 squared distances as oracle/pointops.c forms them: every operation rounded to fp32, in the
    order (dx*dx + dy*dy) + dz*dz with d = centroid - point."""
    d = centroids.astype(F32)[:, None, :] - pts.astype(F32)[None, :, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def expected_ball(d2: np.ndarray, r2: np.float32, nsample: int) -> np.ndarray:
    """(M, nsample) int32: the first `nsample` points with d2 < r2 in index order, padded with the first hit
    (ball_query_gpu.cu:9-45); a ball with no hit stays zero."""
    out = np.zeros((d2.shape[0], nsample), np.int32)
    for i, row in enumerate(d2 < r2):
        hits = np.flatnonzero(row)[:nsample]
        if hits.size:
            out[i] = hits[0]
            out[i, : hits.size] = hits
    return out


def ball_counts(pts: np.ndarray):
    """Per level 0..3 of one (N, 3) cloud, from the oracle's FPS chain and dist2(): dict(fps_idx (M,), new_xyz
    (M, 3), d2 (M, N_prev), and per branch r2, hits (M,) = the TRUE number of points inside the ball (not capped
    at nsample) and ties = the number of point-centroid pairs with d2 == r2 exactly)."""
    from genpose2_amd import arch
    from oracle import oracle
    cur = np.ascontiguousarray(pts, F32)
    out = []
    for lv in range(4):
        fidx = oracle.furthest_point_sample(cur[None], arch.NPOINTS[lv])[0]
        cen = cur[fidx]
        d2 = dist2(cen, cur)
        r2 = [F32(r) * F32(r) for r in arch.RADII[lv]]
        out.append(dict(fps_idx=fidx, new_xyz=cen, d2=d2, r2=r2, hits=[(d2 < r).sum(1) for r in r2],
                        ties=[int((d2 == r).sum()) for r in r2]))
        cur = cen
    return out


# ---------------------------------------------------------------- the cases the tests run
SEED = dict(lattice=1, sparse=1, dense=1, mixed=1, dup=4, clusters=1)
SIZES = (512, 513, 600, 1025, 1500, 2049, 4097, 8191, 8192)   # 513 ... 4097: one above an FPS-chain size class
ALL_A, ALL_B = ("lattice", "sparse", "dense"), ("mixed", "dup", "clusters")

# name -> (N, kinds): one object per kind
GEOMETRY_CASES = {f"n{n}": (n, ("lattice", "mixed")) for n in SIZES}
GEOMETRY_CASES.update(n600_a=(600, ALL_A), n600_b=(600, ALL_B))
ENCODER_CASES = dict(n600_a=(600, ALL_A), n600_b=(600, ALL_B), n512_b3=(512, ("lattice", "mixed", "dup")),
                     n513_lattice=(513, ("lattice",)), n513_mixed=(513, ("mixed",)),
                     n1500_b3=(1500, ("lattice", "mixed", "clusters")), n8192_lattice=(8192, ("lattice",)),
                     n8192_mixed=(8192, ("mixed",)))
LEVEL0_CASES = dict(b1_n513=(513, ("mixed",)), b1_n600=(600, ("clusters",)),
                    b3_n600=(600, ("mixed", "clusters", "lattice")), b2_n8191=(8191, ("lattice", "mixed")))
FUS_CASES = dict(b3_n600=(600, ("mixed", "clusters", "lattice")), b1_n513=(513, ("dup",)),
                 b2_n512=(512, ("sparse", "dense")))


def case_points(case) -> np.ndarray:
    """(B, N, 3) of a (N, kinds) case."""
    n, kinds = case
    return batch([(k, SEED[k]) for k in kinds], n)


def case_objects():
    """Every distinct (kind, N) the GPU tests run."""
    seen = []
    for cases in (GEOMETRY_CASES, ENCODER_CASES, LEVEL0_CASES, FUS_CASES):
        for n, kinds in cases.values():
            seen += [(k, n) for k in kinds if (k, n) not in seen]
    return seen
