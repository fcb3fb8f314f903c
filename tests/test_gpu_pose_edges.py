"""GPU checks of the pose tails and of the aggregation's rotation algebra at their branch edges.

a. gp_pose_epilogue_f64 against the float64 restatement (tests/pose_ref.py), bit for bit;
b. gp_debug_pose_tail_f32 -- the PC step's float32 tail, four lanes per row -- against the float32 restatement,
   bit for bit;
c. the float32 tail against the reference's float64 run (golden_pose_edges.npz) and the generator's rotation;
d. the tails inside the real samplers: q is the restatement of the returned pose, bit for bit;
e. aggregation (rot6_to_quat, the Jacobi eigenvector, quaternion_to_matrix) and bbox_length on cube rotations,
   clusters around half turns and a previous rotation that is a half turn.
The inputs are tests/golden/pose_edge_inputs.py; tests/test_cpu_pose_edges.py anchors the restatement.
Every case runs in well under a second on the device (the sampler cases: 4 steps on 21 / 250 rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import modes_ref
import pose_edge_inputs as pe
import pose_ref as P
from conftest import golden
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                    # sentinel rows after the rows of a call
SENTINEL = -12345.5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@functools.lru_cache(maxsize=None)
def inputs():
    return pe.build()


def _center_rows(n, k):
    nobj = (n + k - 1) // k
    return pe.centers(nobj), np.repeat(pe.centers(nobj), k, 0)[:n]


def _same(a, b):
    return a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


def _first_diff(a, b):
    bad = np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).all(-1))[0]
    return f"{len(bad)} rows differ, first {bad[:5].tolist()}: {a[bad[:2]]} vs {b[bad[:2]]}"


def _run_tail(rows, k, f64):
    """rows (n,9) float32 through gp_pose_epilogue_f64 (widened) or gp_debug_pose_tail_f32 -> (res, q) of the n rows
    as NumPy; the GUARD sentinel rows after them must come back untouched (and the probe must not write its input)."""
    from genpose2_amd import _lib
    lib = _lib.load()
    n = len(rows)
    cen, _ = _center_rows(n, k)
    dt = np.float64 if f64 else np.float32
    pose = np.full((n + GUARD, 9), SENTINEL, dt)
    pose[:n] = rows.astype(dt)
    d_pose, d_cen = _t(pose), _t(cen)
    d_q = torch.full((n + GUARD, 7), SENTINEL, dtype=d_pose.dtype, device=DEV)
    if f64:
        _lib.check(lib.gp_pose_epilogue_f64(_vp(d_pose), n, k, _vp(d_cen), _vp(d_q), _stream()), "pose_epilogue_f64")
        d_res = d_pose
    else:
        d_res = torch.full((n + GUARD, 9), SENTINEL, dtype=torch.float32, device=DEV)
        _lib.check(lib.gp_debug_pose_tail_f32(_vp(d_pose), n, k, _vp(d_cen), _vp(d_res), _vp(d_q), _stream()),
                   "debug_pose_tail_f32")
        assert _same(d_pose.cpu().numpy(), pose)
    res, q = d_res.cpu().numpy(), d_q.cpu().numpy()
    assert np.all(res[n:] == SENTINEL) and np.all(q[n:] == SENTINEL), "rows past `rows` were written"
    return res[:n], q[:n]


def _check_tail(rows, k, f64):
    _, cr = _center_rows(len(rows), k)
    dt = np.float64 if f64 else np.float32
    want_res, want_q = P.pose_tail(rows.astype(dt), cr, quad=not f64)
    res, q = _run_tail(rows, k, f64)
    assert _same(res, want_res), _first_diff(res, want_res)
    assert _same(q, want_q), _first_diff(q, want_q)


CASES_F64 = [(f, 1) for f in pe.FAMILIES] + [("all", 7)] + [(n, 1) for n in (1, 255, 256, 257)]
CASES_F32 = [(n, k) for n in (1, 15, 16, 17, 63, 64, 65, "all") for k in (1, 7)] + [(f, 3) for f in pe.FAMILIES]


def _select(what):
    inp = inputs()
    if what == "all":
        return inp["rows"]
    if isinstance(what, str):
        return inp["rows"][inp["slices"][what]]
    return inp["rows"][:what]                    # the first rows alone


# ------------------------------------------------------------------------------------------ a. float64 epilogue
@pytest.mark.parametrize("what,k", CASES_F64, ids=lambda v: str(v))
def test_epilogue_f64_is_the_restatement(what, k):
    """pose as rewritten in place and q equal the float64 restatement bit for bit (NaN positions equal): every
    family, the whole set with k = 7, and 1 / 255 / 256 / 257 rows around the kernel's 256-thread block. The
    expected translation is float64(t) + float64(centre)."""
    _check_tail(_select(what), k, True)


# ------------------------------------------------------------------------------------------ b. float32 probe
@pytest.mark.parametrize("what,k", CASES_F32, ids=lambda v: str(v))
def test_tail_f32_is_the_restatement(what, k):
    """The PC step's tail in its lane layout (gram_schmidt6_quad, the LDS gather, quat_from_gs<float>) equals the
    float32 restatement bit for bit: 1 .. 65 rows around the 16-row wave and the 64-row mark, the whole set, k = 1
    and 7, and every family on its own."""
    _check_tail(_select(what), k, False)


# ------------------------------------------------------------------------------------------ c. cross-precision
def test_tail_f32_vs_reference_f64_and_generator():
    """Well-conditioned families: the device's float32 q within 4 x 1.36e-7 (pose_ref.F32_VS_F64, the float32
    restatement's own distance from float64) of the reference's float64 q modulo sign, | |q| - 1 | within 4 x the
    float32 restatement's own 1.06e-7, and the rotation rebuilt from q (oracle.quaternion_to_matrix, float64
    arithmetic on the float32 q) within the first bound of the generator's R (the restatement: 2.6e-7).
    Measured on MI355X: 1.20e-7, 1.06e-7 and 2.63e-7, the restatement's own figures, as (b) implies."""
    inp, g = inputs(), golden("pose_edges")
    well = pe.well_mask(inp)
    _, q = _run_tail(inp["rows"], 7, False)
    q = q[well][:, :4].astype(np.float64)
    ref = g["q_f64"][well]
    sign = np.sign((q * ref).sum(-1, keepdims=True))
    e_q = float(np.abs(q * sign - ref).max())
    e_n = float(np.abs(np.sqrt((q * q).sum(-1)) - 1).max())
    e_r = float(np.abs(oracle.quaternion_to_matrix(q) - inp["R"][well]).max())
    print(f"q vs reference float64 {e_q:.3e} | | |q| - 1 | {e_n:.3e} | R(q) vs generator {e_r:.3e}")
    assert not np.any(sign == 0)
    assert e_q <= P.MARGIN * P.F32_VS_F64
    assert e_n <= P.MARGIN * P.QNORM_F32
    assert e_r <= P.MARGIN * P.F32_VS_F64


# ------------------------------------------------------------------------------------------ d. the real kernels
T_STEPS = 4
ENTRIES = ("pc_f16x3", "pc_f32", "pc_object", "pc_energy", "ode_denoise", "ode_denoise_energy", "ode_sample_object",
           "ode_sample_energy")


_HEADS = {}


def _heads(sd, kind, arith):
    from genpose2_amd import device
    if (kind, arith) not in _HEADS:
        h = _HEADS[kind, arith] = device.HeadModel(sd, torch.device(DEV))
        h.set_arith(arith)
    return _HEADS[kind, arith]


def _run_entry(entry, B, K, score_sd, energy_sd):
    from genpose2_amd import sde
    from genpose2_amd.ode import time_scalars
    R = B * K
    gen = torch.Generator(device=DEV).manual_seed(1000 * B + K)
    energy = entry.endswith("energy")
    h = _heads(energy_sd if energy else score_sd, "energy" if energy else "score",
               "f32" if entry == "pc_f32" else "f16x3")
    pobj = h.object_proj(torch.rand(B, 1024, device=DEV, generator=gen))
    center = torch.rand(B, 3, device=DEV, generator=gen)
    x0 = torch.randn(R, 9, device=DEV, generator=gen) * 50
    if entry.startswith("pc"):
        tab = sde.pc_step_table(T_STEPS)
        tproj = h.time_proj(torch.from_numpy(tab[:, 0]).to(DEV))
        res, q, _ = h.pc_sample(pobj, tproj, tab, x0.clone(), K, center, seed=5, energy_grad=energy,
                                coupling="object" if entry == "pc_object" else "batch")
    elif entry.startswith("ode_denoise"):
        eps = 1e-5
        t32, sig, _ = time_scalars(eps)
        g2 = float(sde.diffusion(torch.full((1,), eps, dtype=torch.float32)).to(torch.float32) ** 2)
        step = float(np.float32((1 - eps) / T_STEPS))
        ws = torch.empty(int(h.lib.gp_ode_workspace_size(R)), dtype=torch.uint8, device=DEV)
        res, q = h.ode_denoise(pobj, t32, sig, g2, step, x0.double().contiguous(), K, center, ws, energy_grad=energy)
    elif entry == "ode_sample_object":
        res, q, _, status = h.ode_sample_object(pobj, x0, K, center, 1.0, 1e-5, T_STEPS)
        assert np.all(status == 1)
    else:
        res, q, _, status = h.ode_sample_energy(pobj, x0, K, center, 1.0, 1e-5, T_STEPS)
        assert status == 1
    torch.cuda.synchronize()
    return res.cpu().numpy(), q.cpu().numpy()


@pytest.mark.parametrize("B,K", [(3, 7), (5, 50)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_sampler_tail_is_the_restatement_of_its_pose(entry, B, K, score_sd, energy_sd):
    """Synthetic weights, x0 = 50 * normal, 4 steps; 21 rows (a ragged 16-row tile) and 250 rows. For every sampler
    entry: q[:, :4] is quat_from_gs of the entry's own returned pose bit for bit in the output's precision,
    q[:, 4:] is the pose's translation, and the returned rotation columns are a fixed point of the restated
    Gram-Schmidt: b1 to 2 ulp of 1 (one normalisation of a unit vector); b2 to 2 ulp of 1 plus |d| (1 + |d|) with
    d = b1 . b2 of the returned columns, because the second pass subtracts d b1 before it normalises -- d is
    rounding noise over the sine of the angle between the sampler's raw columns, so b2 is a 2-ulp fixed point only
    where those were well apart (on CPU draws of 1e5 random rows the restated pass moves b2 by up to 925 ulp).
    Measured on MI355X: b1 at most 1 ulp everywhere; b2 at most 1 ulp in the four PC entries, which normalise
    the columns every step, and 1.2 .. 15.5 ulp (|d| up to 19.8 ulp) in the ODE entries, 230 .. 246 of 250 rows
    within 2 ulp. The branch census is printed, not asserted: it depends on the device's output (PC score
    entries at 250 rows: 65 / 171 / 1 / 13; the others spread over all four branches)."""
    res, q = _run_entry(entry, B, K, score_sd, energy_sd)
    dt = np.float32 if entry.startswith("pc") else np.float64
    assert res.dtype == dt and q.dtype == dt and res.shape == (B * K, 9) and q.shape == (B * K, 7)
    assert np.isfinite(res).all() and np.isfinite(q).all()
    want, info = P.quat_from_gs(res[:, :6].copy(), want_info=True)
    print(f"{entry} {B}x{K}: branch census {P.branch_census(info['best'])}, w <= 0 on {int((want[:, 0] <= 0).sum())} rows")
    assert _same(q[:, :4], want), _first_diff(q[:, :4], want)
    assert _same(q[:, 4:], res[:, 6:])
    ulp = float(np.finfo(dt).eps)
    again = P.gram_schmidt6(res[:, :6].copy())
    d = np.abs((res[:, :3].astype(np.float64) * res[:, 3:6]).sum(-1))
    m1 = np.abs(again[:, :3] - res[:, :3]).max(-1)
    m2 = np.abs(again[:, 3:] - res[:, 3:6]).max(-1)
    print(f"  fixed point: b1 {m1.max() / ulp:.2f} ulp, b2 {m2.max() / ulp:.2f} ulp (max |d| {d.max() / ulp:.2f} ulp; "
          f"{int((m2 <= 2 * ulp).sum())} of {len(m2)} rows within 2 ulp)")
    assert m1.max() <= 2 * ulp
    assert np.all(m2 <= 2 * ulp + d * (1 + d))


# ------------------------------------------------------------------------------------------ e. aggregation
def _pose_rows(R, rng):
    """Rotations (..., 3, 3) float64 -> pose rows (..., 9) float32 with translations normal * 0.3."""
    t = rng.normal(size=R.shape[:-2] + (3,)) * 0.3
    return np.concatenate([R[..., :, 0], R[..., :, 1], t], -1).astype(np.float32)


def _preconditions(pose, energy, keep, clustering, eps, min_samples):
    """Asserted on the CPU before any device comparison, so that a flipped borderline decision cannot be blamed on
    the kernel: no DBSCAN row distance within 1e-4 of eps (float64), and the two largest eigenvalues of every
    averaged A (the kept set's, and each cluster's) at least 0.1 apart. -> modes_ref's result (M = 4)."""
    ref = modes_ref.modes_ref(pose, energy, keep, clustering, eps, max(min_samples, 1), 4)
    sp, _, _, _ = oracle.sort_poses_by_energy(pose, energy)
    bs = pose.shape[0]
    q = oracle.matrix_to_quaternion(oracle.rot6_to_matrix(sp[:, :keep, :6].reshape(bs * keep, 6))).reshape(bs, keep, 4)
    for j in range(bs):
        if clustering:
            assert ref["margin"][j] * eps > 1e-4, (j, ref["margin"][j])
        sets = [np.ones(keep, bool)] + [ref["labels"][j] == l for l in range(int(ref["n_clusters"][j]))]
        for member in sets:
            qq = q[j, member].astype(np.float64)
            lam = np.linalg.eigvalsh(np.einsum("ni,nk->ik", qq, qq) / len(qq))
            assert lam[-1] - lam[-2] >= 0.1 or (member.all() and ref["n_clusters"][j] > 0), (j, lam)
    return ref, q


def _angle_deg(Ra, Rb):
    c = (np.einsum("bij,bij->b", Ra.astype(np.float64), Rb.astype(np.float64)) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


@pytest.mark.parametrize("clustering", (0, 1))
def test_aggregate_cube_rotations(clustering):
    """24 objects, one per element of the cube group, K = 10 (keep = 4), every candidate that rotation exactly:
    exact argmax ties, w == 0 and q_abs == 0 in rot6_to_quat, a rank-one A in the Jacobi. The result is that
    matrix within 1e-6 (2 eps x a few operations) and within the existing 1e-5 of oracle.aggregate_pose and
    modes_ref. clustering_minpts is 0.5 (min_samples 2): the default's int(0.1667 * 4) is 0, which sklearn, the
    oracle's DBSCAN, refuses."""
    from genpose2_amd import aggregate
    rng = np.random.default_rng(31)
    C = pe.cube_rotations()
    pose = _pose_rows(np.repeat(C[:, None], 10, 1), rng)
    energy = rng.normal(size=(24, 10, 2)).astype(np.float32)
    ref, _ = _preconditions(pose, energy, 4, clustering, 0.05, 2)
    want = oracle.aggregate_pose(pose, energy, clustering=clustering, clustering_minpts=0.5)
    assert np.abs(want[:, :3, :3] - C).max() < 1e-6
    got = aggregate.aggregate_pose(_t(pose), _t(energy), clustering=clustering, clustering_minpts=0.5).cpu().numpy()
    modes = aggregate.aggregate_modes(_t(pose), _t(energy), clustering=clustering, clustering_minpts=0.5)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() < 1e-5
    assert np.abs(got[:, :3, :3] - C).max() < 1e-6
    assert np.array_equal(modes.aggregated.cpu().numpy(), got)
    assert np.abs(modes.mode_pose.cpu().numpy() - ref["mode_pose"]).max() < 1e-5
    assert np.array_equal(modes.mode_count.cpu().numpy(), ref["mode_count"])
    assert np.array_equal(modes.n_clusters.cpu().numpy(), ref["n_clusters"])


def test_aggregate_clusters_around_half_turns():
    """16 objects, K = 50 (keep = 20), each a cluster around a rotation C by exactly pi about a random axis: every
    candidate is axis_angle(normal(3), 1 deg x |normal|) @ C, so the kept quaternions' w changes sign inside
    every cluster (asserted on the CPU: 1 to 19 of 20 positive) and the sign orientation of the average is
    exercised. Within 1e-5 of the oracle and within 1 degree of C (the float64 oracle: 0.3 degrees)."""
    from genpose2_amd import aggregate
    rng = np.random.default_rng(47)
    B, K, keep = 16, 50, 20
    C = pe.half_turn(rng.normal(size=(B, 3)))
    noise = pe.axis_angle(rng.normal(size=(B * K, 3)), np.radians(1.0) * np.abs(rng.normal(size=B * K)))
    pose = _pose_rows(noise.reshape(B, K, 3, 3) @ C[:, None], rng)
    energy = rng.normal(size=(B, K, 2)).astype(np.float32)
    for clustering in (0, 1):
        ref, q = _preconditions(pose, energy, keep, clustering, 0.05, 3)
        pos = (q[:, :, 0] > 0).sum(1)
        print("kept quaternions with w > 0 per object:", pos.tolist())
        assert np.all((pos >= 1) & (pos <= keep - 1))
        assert not clustering or (np.all(ref["n_clusters"] == 1) and np.all(ref["noise_count"] == 0))
        want = oracle.aggregate_pose(pose, energy, clustering=clustering)
        got = aggregate.aggregate_pose(_t(pose), _t(energy), clustering=clustering).cpu().numpy()
        ang = _angle_deg(got[:, :3, :3], C)
        print(f"clustering {clustering}: vs oracle {np.abs(got - want).max():.2e}, degrees from C max {ang.max():.3f}")
        assert np.abs(got - want).max() < 1e-5
        assert np.abs(got - ref["aggregated"]).max() < 1e-5
        assert ang.max() < 1.0 and _angle_deg(want[:, :3, :3], C).max() < 1.0


def test_modes_nearest_to_a_half_turn():
    """aggregate_modes with prev_rot a 180-degree element of the cube group (w == 0 exactly in rot6_to_quat) and two
    clusters: 12 candidates around that element, 8 around it turned by 90 degrees, 30 random ones of lower
    rotation energy; one object per 180-degree element (9). ``nearest`` and slot 0 are as modes_ref gives them,
    for prev_rot the first cluster's centre and for the second's."""
    from genpose2_amd import aggregate
    rng = np.random.default_rng(59)
    cube = pe.cube_rotations()
    half = cube[np.isclose(np.trace(cube, axis1=1, axis2=2), -1)]
    assert len(half) == 9
    B, K, keep = len(half), 50, 20
    turn = pe.axis_angle(np.array([[0.0, 0.0, 1.0]]), np.pi / 2)[0]
    second = half @ turn
    centre = np.concatenate([np.repeat(half[:, None], 12, 1), np.repeat(second[:, None], 8, 1)], 1)
    noise = pe.axis_angle(rng.normal(size=(B * keep, 3)), np.radians(1.0) * np.abs(rng.normal(size=B * keep)))
    rot = np.concatenate([noise.reshape(B, keep, 3, 3) @ centre,
                          pe.axis_angle(rng.normal(size=(B * 30, 3)), rng.uniform(0, np.pi, B * 30)).reshape(B, 30, 3, 3)], 1)
    pose = _pose_rows(rot, rng)
    energy = rng.normal(size=(B, K, 2)).astype(np.float32)
    energy[:, :keep, 0] = rng.uniform(0.5, 1.0, size=(B, keep))
    energy[:, keep:, 0] = rng.uniform(-1.0, 0.25, size=(B, K - keep))
    perm = rng.permutation(K)
    pose, energy = pose[:, perm], energy[:, perm]
    _preconditions(pose, energy, keep, 1, 0.05, 3)
    for which, prev in enumerate((half, second)):
        prev = prev.astype(np.float32)
        ref = modes_ref.modes_ref(pose, energy, keep, 1, 0.05, 3, 4, prev)
        assert np.all(ref["n_clusters"] == 2) and np.all(ref["mode_count"][:, :2] == [12, 8])
        assert np.all(ref["nearest"] == which) and np.all(ref["nearest_gap"] > 1e-2)
        m = aggregate.aggregate_modes(_t(pose), _t(energy), max_modes=4, prev_rot=_t(prev))
        assert np.array_equal(m.nearest.cpu().numpy(), ref["nearest"])
        assert np.array_equal(m.mode_count.cpu().numpy(), ref["mode_count"])
        assert np.array_equal(m.n_clusters.cpu().numpy(), ref["n_clusters"])
        mp = m.mode_pose.cpu().numpy()
        assert np.abs(mp - ref["mode_pose"]).max() < 1e-5
        assert np.abs(m.aggregated.cpu().numpy() - ref["aggregated"]).max() < 1e-5
        assert _angle_deg(mp[:, 0, :3, :3], half).max() < 1.0 and _angle_deg(mp[:, 1, :3, :3], second).max() < 1.0


def test_bbox_length_on_cube_poses():
    """gp_bbox_length, which the size stage runs on the aggregated pose, with each of the 24 cube rotations as that
    pose, against oracle.bbox_length at the existing 1e-6 (relative to the largest length)."""
    from genpose2_amd import device as dev
    rng = np.random.default_rng(61)
    C = pe.cube_rotations()
    pcl = (rng.normal(size=(24, 1000, 3)) * np.array([0.05, 0.1, 0.2]) + 0.3).astype(np.float32)
    pose = np.zeros((24, 4, 4), np.float32)
    pose[:, :3, :3] = C
    pose[:, :3, 3] = oracle.points_mean(pcl)
    pose[:, 3, 3] = 1
    got = dev.bbox_length(_t(pcl), _t(pose)).cpu().numpy()
    want = oracle.bbox_length(pcl, pose)
    assert np.abs(got.astype(np.float64) - want).max() / np.abs(want).max() < 1e-6
