"""Keeps the encoder edge-case clouds (tests/golden/encoder_edge_inputs.py) adversarial, with the oracle alone: over the
cases the GPU tests run (tests/test_gpu_encoder_edge.py), every ball-query situation the device kernel treats
differently must occur at every level, each kind must keep the property it is named for, and the ball list rebuilt
from the fp32 distances must be the oracle's."""
import functools

import numpy as np
import pytest

import encoder_edge_inputs as ei
from genpose2_amd import arch
from oracle import oracle

NS_A, NS_B = arch.NSAMPLES[0]


@functools.lru_cache(maxsize=None)
def counts(kind, n):
    return ei.ball_counts(ei.cloud(kind, n, ei.SEED[kind]))


def situations(level):
    """Which ball-query situations one level of one cloud holds."""
    ha, hb = level["hits"]
    both, ns = np.concatenate([ha, hb]), np.concatenate([np.full_like(ha, NS_A), np.full_like(hb, NS_B)])
    return dict(one_hit=(both == 1).any(), short=((both > 1) & (both < ns)).any(), exactly_full=(both == ns).any(),
                overfull=(both > ns).any(), b_full_a_short=((hb >= NS_B) & (ha < NS_A)).any(),
                a_full_b_short=((ha >= NS_A) & (hb < NS_B)).any(), tie=sum(level["ties"]) > 0)


def test_cases_cover_every_ball_situation_at_every_level():
    seen = [{} for _ in range(4)]
    for kind, n in ei.case_objects():
        for lv, level in enumerate(counts(kind, n)):
            for k, v in situations(level).items():
                seen[lv][k] = seen[lv].get(k, False) or bool(v)
    for lv in range(4):
        for k, v in seen[lv].items():
            if k == "a_full_b_short" and lv > 0:
                continue   # required at level 0 only
            assert v, f"no case has '{k}' at level {lv}"


def test_each_kind_keeps_its_property():
    n = 600
    lat, sparse, dense, mixed, clusters = (counts(k, n) for k in ("lattice", "sparse", "dense", "mixed", "clusters"))
    # lattice: duplicates, exact ties at levels 1-3, balls of exactly nsample hits
    assert len(np.unique(ei.cloud("lattice", n, ei.SEED["lattice"]), axis=0)) < n
    assert all(sum(lat[lv]["ties"]) > 0 for lv in (1, 2, 3))
    assert any(situations(lat[lv])["exactly_full"] for lv in range(4))
    # sparse: over 90 % of the level-0 balls of radius a hold the centroid alone
    assert (sparse[0]["hits"][0] == 1).mean() > 0.9
    # dense: every ball of every level is full within the first 64 points
    for level in dense:
        for r2, ns in zip(level["r2"], (NS_A, NS_B)):
            assert ((level["d2"][:, :64] < r2).sum(1) >= ns).all()
    # mixed: a quarter of the level-0 balls full in both radii, a quarter one-hit in both, both inside one workgroup
    ha, hb = mixed[0]["hits"]
    full, one = (ha > NS_A) & (hb > NS_B), (ha == 1) & (hb == 1)
    assert full.mean() >= 0.25 and one.mean() >= 0.25
    assert any(full[g:g + 32].any() and one[g:g + 32].any() for g in range(0, 512, 32))
    # dup: the last two thirds repeat the first two thirds
    d = ei.cloud("dup", n, ei.SEED["dup"])
    assert np.array_equal(d[n // 3: 2 * (n // 3)], d[: n // 3]) and len(np.unique(d, axis=0)) == n - n // 3
    # clusters: radius a fills while b stays short for most level-0 balls; the planted points tie both radii
    ha, hb = clusters[0]["hits"]
    assert ((ha >= NS_A) & (hb < NS_B)).mean() > 0.5
    assert all(t > 0 for t in clusters[0]["ties"])
    c = ei.cloud("clusters", n, ei.SEED["clusters"])
    assert all((c == p).all(1).any() for p in ei.planted())


def test_planted_points_sit_on_and_one_ulp_inside_the_radius():
    p = ei.planted()
    for j, r in enumerate(arch.RADII[0]):
        c, on, inside = p[3 * j: 3 * j + 3]
        r2 = np.float32(r) * np.float32(r)
        d_on, d_in = ei.dist2(c[None], on[None])[0, 0], ei.dist2(c[None], inside[None])[0, 0]
        assert d_on == r2 and d_in < r2
        assert abs(inside[0]) == np.nextafter(np.float32(r), np.float32(0))


@pytest.mark.parametrize("kind,n", [(k, 600) for k in ei.KINDS] + [("lattice", 8192), ("mixed", 513)])
def test_ball_list_from_distances_is_the_oracles(kind, n):
    """First nsample hits in index order, padded with the first hit, from ball_counts' fp32 distances: equal to
    oracle.ball_query on the oracle's FPS chain, every level and radius."""
    cur = ei.cloud(kind, n, ei.SEED[kind])
    for lv, level in enumerate(counts(kind, n)):
        np.testing.assert_array_equal(level["fps_idx"], oracle.furthest_point_sample(cur[None], arch.NPOINTS[lv])[0])
        for r, r2, ns in zip(arch.RADII[lv], level["r2"], arch.NSAMPLES[lv]):
            ref = oracle.ball_query(r, ns, cur[None], level["new_xyz"][None])[0]
            np.testing.assert_array_equal(ei.expected_ball(level["d2"], r2, ns), ref, err_msg=f"level {lv} r {r}")
        cur = level["new_xyz"]


def test_clouds_regenerate_bit_for_bit():
    for kind in ei.KINDS:
        a, b = ei.cloud(kind, 600, 3), ei.cloud(kind, 600, 3)
        assert a.dtype == np.float32 and a.shape == (600, 3) and np.array_equal(a, b) and np.isfinite(a).all()
        assert not np.array_equal(a, ei.cloud(kind, 600, 4))
