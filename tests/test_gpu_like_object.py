"""GPU checks of the object-coupled likelihood (cfg.like_coupling = "object", gp_like_sample_object): one RK45 solve
per object over [x_b (9K) | logp_b (K)]. One attempt against gp_like_attempt on each object's rows alone (bit for
bit), the whole mode against the reference called once per object (golden_like_object), and the contract itself: an
object's ll, latent, nfev and status are bit-identical whatever else the call holds and however a batch is split into
calls."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _agent(**kw):
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    return PoseNet(GenPoseConfig(device=DEV, **kw)).eval()


@pytest.fixture(scope="module")
def agent():
    a = _agent(like_coupling="object")
    yield a
    a.heads.set_arith("f16x3")


@pytest.fixture(scope="module")
def batch_agent():
    return _agent(like_coupling="batch")


def _neighbours():
    """The batch-coupled get_likelihood on golden_like_ode and the object-coupled ODE sampler on golden_ode_object,
    each on an agent of its own -> their outputs."""
    import ode_object_inputs as oi
    from genpose2_amd.agent import NoiseFeed
    g = golden("like_ode")
    a = _agent(sampler_mode=["ode"])
    a.noise_feed = NoiseFeed(torch.from_numpy(g["eps_unit"]))
    data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    ll, z = a.get_likelihood(data, torch.from_numpy(g["pose_samples"]).to(DEV), return_latent=True)
    g = golden("ode_object")
    s = _agent(sampler_mode=["ode"], ode_coupling="object", sampling_steps=oi.STEPS)
    s.noise_feed = NoiseFeed(torch.from_numpy(g["prior"]))
    data = {"pts": torch.zeros((oi.B, 1, 3), device=DEV), "pts_feat": torch.from_numpy(g["pts_feat"]).to(DEV),
            "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
    pose, q = s.pred_func(data, repeat_num=oi.K, extract_feature=False, T0=oi.T0)
    torch.cuda.synchronize()
    return ll.clone(), z.clone(), a.last_nfev, pose.clone(), q.clone(), s.last_nfev_objects.copy()


@pytest.fixture(scope="module", autouse=True)
def neighbours_before():
    """Runs before this module's first object-coupled likelihood call (test_neighbours_untouched compares)."""
    return _neighbours()


@pytest.fixture(scope="module")
def spread():
    """The reference's own float32 spread about its float64 run on golden_like_object, called once per object: the
    largest max and the largest mean of |ll32* - ll64| over the 21 rows among its three float32 runs."""
    g = golden("like_object")
    refs = [np.abs(g[k] - g["ll64"]) for k in ("ll32", "ll32_p1", "ll32_p2")]
    return {"max": max(float(e.max()) for e in refs), "mean": max(float(e.mean()) for e in refs)}


class _Objects:
    """B <= 3 objects x K poses: golden_like_object's features and centers (solves of known length), seeded poses
    about each center and unit normals behind eps for a whole batch of `total` objects."""

    def __init__(self, B, K, seed=911, total=None):
        from like_inputs import _gs6
        g = golden("like_object")
        self.B, self.K = B, K
        self.total = B if total is None else total
        rng = np.random.default_rng(seed)
        self.feat = torch.from_numpy(g["pts_feat"][:B].copy()).to(DEV)
        self.center = torch.from_numpy(g["pts_center"][:B].copy()).to(DEV)
        local = np.concatenate([_gs6(rng.normal(size=(B * K, 6))), 0.05 * rng.normal(size=(B * K, 3))], 1)
        cam = local.astype(np.float32)
        cam[:, 6:] += np.repeat(g["pts_center"][:B], K, 0)
        self.poses = torch.from_numpy(cam.reshape(B, K, 9)).to(DEV)
        self.prior = torch.from_numpy(rng.standard_normal((self.total * K, 9)).astype(np.float32))

    def run(self, a, lo=0, hi=None, feat=None, poses=None, prior=None, window=True):
        """Objects [lo, hi) as one get_likelihood call of agent `a`, as a window of the whole batch (object
        coupling) -> (ll, z, nfev per object, status per object)."""
        from genpose2_amd.agent import NoiseFeed
        hi = self.B if hi is None else hi
        feat = self.feat if feat is None else feat
        poses = self.poses if poses is None else poses
        prior = self.prior if prior is None else prior
        obj = a.cfg.like_coupling == "object"
        a.noise_feed = NoiseFeed(prior if obj else prior[lo * self.K:hi * self.K])
        a.object_window = (self.total, lo) if (obj and window) else None
        try:
            data = {"pts": torch.zeros((hi - lo, 1, 3), device=DEV), "pts_feat": feat[lo:hi].contiguous(),
                    "pts_center": self.center[lo:hi].contiguous()}
            ll, z = a.get_likelihood(data, poses[lo:hi].contiguous(), extract_feature=False, return_latent=True)
        finally:
            a.object_window = None
            a.noise_feed = None
        torch.cuda.synchronize()
        assert ll.dtype == torch.float64 and z.dtype == torch.float64
        assert tuple(ll.shape) == (hi - lo, self.K) and tuple(z.shape) == (hi - lo, self.K, 9)
        assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(z).all())
        if obj:
            assert a.last_nfev == int(a.last_nfev_objects.max())
            return ll, z, a.last_nfev_objects.copy(), a.last_status_objects.copy()
        return ll, z, np.asarray([a.last_nfev]), None


def _same(full, part, lo, hi, what):
    assert torch.equal(full[0][lo:hi], part[0]) and torch.equal(full[1][lo:hi], part[1]), (what, "ll / z")
    assert np.array_equal(full[2][lo:hi], part[2]) and np.array_equal(full[3][lo:hi], part[3]), (what, "nfev / status")


@pytest.fixture(scope="module")
def obj3():
    return _Objects(3, 7)


def _other_object(o):
    """o's inputs with object 1 replaced by another object (features and poses)."""
    feat, poses = o.feat.clone(), o.poses.clone()
    feat[1] = 0.5 * o.feat[0] + 0.5 * o.feat[2]
    poses[1] = o.poses[0]
    poses[1, :, 6:] = o.poses[0, :, 6:] - o.center[0] + o.center[1] + 0.01
    return feat, poses


# ---------------------------------------------------------------------------------------------------- 1. one attempt
class OdeObjRec(ctypes.Structure):
    """Host mirror of the per-object controller record (gp_ode.h OdeObjRec, 168 bytes)."""
    _fields_ = [("t", ctypes.c_double), ("h_abs", ctypes.c_double), ("t_old", ctypes.c_double),
                ("h", ctypes.c_double), ("t_new", ctypes.c_double), ("h_abs_loc", ctypes.c_double),
                ("coef", ctypes.c_double * 6), ("t32", ctypes.c_float * 6), ("sig", ctypes.c_float * 6),
                ("status", ctypes.c_int), ("active", ctypes.c_int), ("rejected", ctypes.c_int),
                ("nfev", ctypes.c_int), ("n_acc", ctypes.c_int), ("pend", ctypes.c_int)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("arith", ("f16x3", "f32"))
def test_attempt_is_the_composition(agent, arith):
    """One object-coupled attempt (gp_debug_like_obj_attempt) on B = 3 x K = 7 with the objects at three different
    (t, h), against gp_like_attempt on each object's rows alone at that object's (t, h): K_1..K_6 and y_new bitwise
    equal for all ten entries per row; each object's error norm from the row sums within 1e-12 relative of math.fsum
    of the same float64 terms (scipy's expression over the downloaded stages); an accepted step pending its copy
    (pend = 1: the state in y_new, its derivative in K_6) gives the same bits; an object marked inactive keeps its
    fill values."""
    from genpose2_amd import _lib, ode
    h_, lib = agent.heads, agent.heads.lib
    h_.set_arith(arith)
    try:
        B, K = 3, 7
        R, n = B * K, 10 * B * K
        rtol = atol = 1e-5
        assert ctypes.sizeof(OdeObjRec) == int(lib.gp_debug_ode_obj_rec_size())
        rng = np.random.default_rng(41)
        feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
        pobj = h_.object_proj(torch.from_numpy(feat).to(DEV))
        x = rng.normal(size=(R, 9))
        x[:, 6:] *= 0.3
        y = torch.from_numpy(np.concatenate([x.reshape(-1), 0.1 * rng.normal(size=R)])).to(DEV)
        eps = torch.from_numpy((rng.standard_normal((R, 9)) * 50.0).astype(np.float32)).to(DEV)
        th = [(0.3, 2e-3), (0.05, 4e-4), (0.81, 7e-3)]
        s = h_._s()

        def rows_of(v, b):   # object b's entries of a vector in the state's layout, as a state of K rows
            return torch.cat([v[9 * K * b: 9 * K * (b + 1)], v[9 * R + K * b: 9 * R + K * (b + 1)]]).contiguous()

        def put(dst, b, v):
            dst[9 * K * b: 9 * K * (b + 1)] = v[:9 * K]
            dst[9 * R + K * b: 9 * R + K * (b + 1)] = v[9 * K:]

        # per object alone: K_0 = f(t, y_b), then gp_like_attempt
        ws = torch.empty(int(lib.gp_like_workspace_size(K)), dtype=torch.uint8, device=DEV)
        K0 = torch.zeros(n, dtype=torch.float64, device=DEV)
        solo, recs = [], (OdeObjRec * B)()
        for b, (t, h) in enumerate(th):
            yb, eb, pb = rows_of(y, b), eps[K * b: K * (b + 1)].contiguous(), pobj[b:b + 1].contiguous()
            t32, sig, coef = ode.time_scalars(np.float64(t))
            k0 = torch.zeros(10 * K, dtype=torch.float64, device=DEV)
            _lib.check(lib.gp_like_rhs(ctypes.byref(h_.w), _p(pb), t32, sig, coef, _p(yb), _p(eb), None, None, 0, 0.0,
                                       K, K, _p(k0), _p(ws), ws.numel(), s), "like_rhs")
            put(K0, b, k0)
            Ks = [k0] + [torch.zeros(10 * K, dtype=torch.float64, device=DEV) for _ in range(6)]
            yn = torch.zeros(10 * K, dtype=torch.float64, device=DEV)
            err = torch.zeros(1, dtype=torch.float64, device=DEV)
            t32s, sigs, coefs = ode.stage_scalars([t + c * h for c in ode.C[1:]] + [t + h])
            _lib.check(lib.gp_like_attempt(
                ctypes.byref(h_.w), _p(pb), t32s.ctypes.data_as(ctypes.c_void_p), sigs.ctypes.data_as(ctypes.c_void_p),
                coefs.ctypes.data_as(ctypes.c_void_p), _p(yb), _p(eb), ode._ptr_array(Ks),
                ode._A6.ctypes.data_as(ctypes.c_void_p), ode._B6.ctypes.data_as(ctypes.c_void_p),
                ode._E7.ctypes.data_as(ctypes.c_void_p), float(h), rtol, atol, K, K, _p(yn), _p(err), _p(ws), ws.numel(),
                s), "like_attempt")
            torch.cuda.synchronize()
            solo.append((Ks, yn, float(err.cpu()[0])))
            r = recs[b]
            r.t, r.h, r.active = t, h, 1
            for j in range(6):
                r.t32[j], r.sig[j], r.coef[j] = float(t32s[j]), float(sigs[j]), float(coefs[j])

        def attempt(recs, y_, ynew, Ks, fill=None):
            rec = torch.from_numpy(np.frombuffer(bytes(recs), dtype=np.uint8).copy()).to(DEV)
            rowsq = torch.full((R,), 0.0 if fill is None else fill, dtype=torch.float64, device=DEV)
            scratch = torch.zeros((6 * B + 1) * 768, dtype=torch.float32, device=DEV)
            _lib.check(lib.gp_debug_like_obj_attempt(ctypes.byref(h_.w), _p(pobj), _p(rec), _p(eps), _p(y_), _p(ynew),
                                                     ode._ptr_array(Ks), _p(rowsq), _p(scratch), R, K, R, rtol, atol,
                                                     s), "debug_like_obj_attempt")
            torch.cuda.synchronize()
            return rowsq

        Ka = [K0.clone()] + [torch.zeros(n, dtype=torch.float64, device=DEV) for _ in range(6)]
        ynew = torch.zeros(n, dtype=torch.float64, device=DEV)
        rowsq = attempt(recs, y.clone(), ynew, Ka)
        E = np.asarray(ode.E, np.float64)
        for b, (t, h) in enumerate(th):
            Ks, yn, err = solo[b]
            for j in range(1, 7):   # the figures first: entries that differ, among the x entries and the logp entries
                d = (rows_of(Ka[j], b) - Ks[j]).abs()
                if float(d.max()) != 0.0:
                    print(f"{arith} object {b} K_{j}: {int((d[:9 * K] != 0).sum())} of {9 * K} x entries differ (max "
                          f"{float(d[:9 * K].max()):.3e}), {int((d[9 * K:] != 0).sum())} of {K} logp entries (max "
                          f"{float(d[9 * K:].max()):.3e}; max |K| {float(Ks[j].abs().max()):.3e})")
            for j in range(1, 7):
                assert torch.equal(rows_of(Ka[j], b), Ks[j]), (arith, b, j)
            assert torch.equal(rows_of(ynew, b), yn), (arith, b)
            Kn = np.stack([k.cpu().numpy() for k in Ks])
            y0, y1 = rows_of(y, b).cpu().numpy(), yn.cpu().numpy()
            e = np.dot(Kn.T, E) * h / (atol + np.maximum(np.abs(y0), np.abs(y1)) * rtol)
            want = math.sqrt(math.fsum((e * e).tolist())) / math.sqrt(10 * K)
            got = math.sqrt(math.fsum(rowsq[K * b: K * (b + 1)].cpu().tolist())) / math.sqrt(10 * K)
            print(f"{arith} object {b}: error norm {got:.17g} vs fsum {want:.17g} (gp_like_attempt alone {err:.17g})")
            assert e.size == 10 * K and abs(got - want) <= 1e-12 * want, (arith, b, got, want)

        # the accepted step not yet copied: the state in y_new, its derivative in K_6; y and K_0 hold something else
        for b in range(B):
            recs[b].pend = 1
        Kp = [torch.full((n,), 3.0, dtype=torch.float64, device=DEV)] + \
             [torch.zeros(n, dtype=torch.float64, device=DEV) for _ in range(5)] + [K0.clone()]
        yp, ynp = torch.full((n,), -2.0, dtype=torch.float64, device=DEV), y.clone()
        rowsq_p = attempt(recs, yp, ynp, Kp)
        assert torch.equal(yp, y) and torch.equal(Kp[0], K0)            # the prologue's copies
        assert torch.equal(ynp, ynew) and torch.equal(rowsq_p, rowsq)
        for j in range(1, 7):
            assert torch.equal(Kp[j], Ka[j]), (arith, "pend", j)

        # object 1 inactive: its rows keep their fill, the others their bits
        FILL = 7.0
        for b in range(B):
            recs[b].pend = 0
        recs[1].active = 0
        Kf = [K0.clone()] + [torch.full((n,), FILL, dtype=torch.float64, device=DEV) for _ in range(6)]
        ynf = torch.full((n,), FILL, dtype=torch.float64, device=DEV)
        yf = y.clone()
        rowsq_f = attempt(recs, yf, ynf, Kf, fill=FILL)
        assert torch.equal(yf, y) and torch.equal(Kf[0], K0)
        for v, ref in [(ynf, ynew)] + list(zip(Kf[1:], Ka[1:])):
            assert bool((rows_of(v, 1) == FILL).all())
            for b in (0, 2):
                assert torch.equal(rows_of(v, b), rows_of(ref, b))
        assert bool((rowsq_f[K:2 * K] == FILL).all())
        assert torch.equal(rowsq_f[:K], rowsq[:K]) and torch.equal(rowsq_f[2 * K:], rowsq[2 * K:])
    finally:
        h_.set_arith("f16x3")


# ------------------------------------------------------------------------------------- 2. against the reference
@pytest.mark.parametrize("arith", ("f16x3", "f32"))
def test_get_likelihood_vs_reference_per_object(agent, spread, arith):
    """get_likelihood with like_coupling='object' on golden_like_object (B = 3 x K = 7: object 2 straddles the
    16-row tile boundary, the last tile is partial; eps injected through noise_feed) against the reference's float64
    run called once per object: |ll - ll64| within 2x the spread of the reference's own three float32 runs about
    ll64, in max and in mean over the 21 rows (the batch-coupled test's rule and margin: the solve is chaotic at
    solver-tolerance scale). nfev per object is printed beside the reference's, not asserted; every status is 1.

    Measured, MI355X: see DESIGN.md "Likelihood: one RK45 solve per object"."""
    from genpose2_amd.agent import NoiseFeed
    g = golden("like_object")
    B, K = g["pose_samples"].shape[:2]
    agent.heads.set_arith(arith)
    try:
        data = {"pts": torch.from_numpy(g["pts"]).to(DEV), "pts_center": torch.from_numpy(g["pts_center"]).to(DEV)}
        agent.noise_feed = NoiseFeed(torch.from_numpy(g["eps_unit"]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll, z = agent.get_likelihood(data, torch.from_numpy(g["pose_samples"]).to(DEV), return_latent=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        agent.noise_feed = None
        agent.heads.set_arith("f16x3")
    assert ll.dtype == torch.float64 and tuple(ll.shape) == (B, K)
    assert z.dtype == torch.float64 and tuple(z.shape) == (B, K, 9)
    e = np.abs(ll.cpu().numpy() - g["ll64"])
    ours = {"max": float(e.max()), "mean": float(e.mean())}
    print(f"{arith}: get_likelihood (object) vs ll64: ours {ours}, reference fp32 spread {spread}; nfev per object "
          f"{agent.last_nfev_objects.tolist()} (reference fp32 {g['nfev_ll32'].tolist()}, float64 "
          f"{g['nfev_ll64'].tolist()}); per object max |ll - ll64| {e.max(1).round(3).tolist()}; "
          f"latent max |z - z64| {np.abs(z.cpu().numpy() - g['z64']).max():.3e}; call {dt * 1e3:.0f} ms")
    assert agent.last_status_objects.tolist() == [1] * B
    assert agent.last_nfev == int(agent.last_nfev_objects.max()) and np.all((agent.last_nfev_objects - 2) % 6 == 0)
    assert ours["max"] <= 2 * spread["max"] and ours["mean"] <= 2 * spread["mean"], (ours, spread)


# --------------------------------------------------------------------------------------------- 3. - 6. the contract
def test_composition_invariance_exact(agent, obj3):
    """The batch of 3 against each object alone as a window (total = 3): ll, z, nfev and status bitwise; then
    object 1 replaced by another (features and poses): objects 0 and 2 keep their bits, object 1's change."""
    o = obj3
    t0 = time.perf_counter()
    full = o.run(agent)
    print(f"  B = 3 x K = 7: nfev {full[2].tolist()}, call {(time.perf_counter() - t0) * 1e3:.0f} ms")
    assert full[3].tolist() == [1] * o.B
    for b in range(o.B):
        _same(full, o.run(agent, b, b + 1), b, b + 1, f"object {b} alone")
    feat, poses = _other_object(o)
    other = o.run(agent, feat=feat, poses=poses)
    for b in (0, 2):
        _same(full, tuple(t[b:b + 1] for t in other), b, b + 1, f"object {b} beside another object 1")
    assert not torch.equal(full[0][1], other[0][1]) and not torch.equal(full[1][1], other[1][1])


def test_batch_coupling_lacks_the_property(batch_agent, obj3):
    """The same replacement under like_coupling='batch' changes object 0's ll."""
    o = obj3
    feat, poses = _other_object(o)
    assert not torch.equal(o.run(batch_agent)[0][0], o.run(batch_agent, feat=feat, poses=poses)[0][0])


def test_objects_finish_apart(agent, obj3):
    """At least two objects differ in attempts, so the earliest finisher sits inactive while the others go on. Its
    result equals its solo run (in which nothing follows its last step): its rows were not written after it
    finished."""
    o = obj3
    full = o.run(agent)
    attempts = (full[2] - 2) // 6
    print(f"  attempts per object {attempts.tolist()}")
    assert np.all((full[2] - 2) % 6 == 0) and full[3].tolist() == [1] * o.B
    assert len(set(attempts.tolist())) >= 2
    first = int(np.argmin(attempts))
    _same(full, o.run(agent, first, first + 1), first, first + 1, "the earliest finisher alone")


def test_one_call_against_two_calls(agent, obj3):
    """One call on 3 objects against two calls on objects [0,1) and [1,3) through PoseNet.object_window, with the
    agent's own eps draw (every call restarts the generator, as ranks of a sharded run hold the same state)."""
    o = obj3

    def call(lo, hi, window):
        agent._gen.manual_seed(agent.cfg.noise_seed)
        agent.object_window = window
        try:
            data = {"pts": torch.zeros((hi - lo, 1, 3), device=DEV), "pts_feat": o.feat[lo:hi].contiguous(),
                    "pts_center": o.center[lo:hi].contiguous()}
            ll, z = agent.get_likelihood(data, o.poses[lo:hi].contiguous(), extract_feature=False, return_latent=True)
            return ll, z, agent.last_nfev_objects.copy(), agent.last_status_objects.copy()
        finally:
            agent.object_window = None

    one = call(0, 3, None)
    for lo, hi in ((0, 1), (1, 3)):
        _same(one, call(lo, hi, (3, lo)), lo, hi, f"objects [{lo},{hi})")
    _same(one, call(0, 3, (3, 0)), 0, 3, "the whole batch as a window")


# ------------------------------------------------------------------------------------------------- 7. edge shapes
def _solo_vs_batch_coupling(agent, batch_agent, o, spread):
    """Every object alone has the bits it has in the call. Against the batch-coupled solve of the object alone only
    the 2x spread bar of golden_like_object: the two differ in the order of the norm's sum, and the solve is
    chaotic."""
    t0 = time.perf_counter()
    full = o.run(agent)
    print(f"  B = {o.B} x K = {o.K}: nfev {full[2].tolist()}, call {(time.perf_counter() - t0) * 1e3:.0f} ms")
    assert full[3].tolist() == [1] * o.B
    for b in range(o.B):
        _same(full, o.run(agent, b, b + 1), b, b + 1, f"object {b} alone")
        lb, _, nb, _ = o.run(batch_agent, b, b + 1)
        d = (lb - full[0][b:b + 1]).abs()
        print(f"  object {b}: nfev {int(full[2][b])}, batch coupling alone {int(nb[0])}; |ll - ll_batch| max "
              f"{d.max().item():.3f} mean {d.mean().item():.3f}")
        assert d.max().item() <= 2 * spread["max"] and d.mean().item() <= 2 * spread["mean"], (b, d, spread)


def test_one_pose_per_object(agent, batch_agent, spread):
    """B = 3 x K = 1: every norm is over the ten entries of one row."""
    _solo_vs_batch_coupling(agent, batch_agent, _Objects(3, 1), spread)


def test_object_wider_than_four_tiles(agent, batch_agent, spread):
    """B = 2 x K = 70: each object spans five 16-row tiles, so its error norm gathers row sums that other workgroups
    wrote, and a lane of the summing wave holds two rows."""
    _solo_vs_batch_coupling(agent, batch_agent, _Objects(2, 70), spread)


# ------------------------------------------------------------------------------------------------ 8. wide tiling
def test_wide_tiling_on_a_tiny_grid(agent):
    """B = 2 x K = 5 as a window of rows_total = 4,100 (f16x3): two primal tiles per workgroup. Bit-identical to
    object-alone calls under the same rows_total. Whether it equals the 16-row tiling's result is printed; nothing
    is asserted across tile classes."""
    agent.heads.set_arith("f16x3")
    K = 5
    o = _Objects(2, K, total=4100 // K)
    wide = o.run(agent)
    assert wide[3].tolist() == [1, 1]
    for b in range(2):
        _same(wide, o.run(agent, b, b + 1), b, b + 1, f"object {b} alone")
    narrow = _Objects(2, K)
    narrow.prior, narrow.poses = o.prior[:2 * K], o.poses
    n = narrow.run(agent)
    print(f"  equal to the 16-row tiling's result: ll {torch.equal(wide[0], n[0])}, z {torch.equal(wide[1], n[1])}; "
          f"nfev {wide[2].tolist()} (16-row tiles {n[2].tolist()}); max |ll - ll_16| "
          f"{(wide[0] - n[0]).abs().max().item():.3e}")


# -------------------------------------------------------------------------------------------- 9. status fallback
def test_status_fallback_same_bits(agent, obj3, monkeypatch):
    """GENPOSE2_ODE_ZC=0 reads the status through an event and a copy instead of the host-mapped words."""
    out = {}
    for zc in ("1", "0"):
        monkeypatch.setenv("GENPOSE2_ODE_ZC", zc)
        out[zc] = obj3.run(agent)
    _same(out["1"], out["0"], 0, obj3.B, "event-and-copy status reads")


# ---------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals(agent, obj3):
    data = {"pts": torch.zeros((1, 1, 3), device=DEV), "pts_feat": torch.zeros((1, 1024), device=DEV),
            "pts_center": torch.zeros((1, 3), device=DEV)}
    poses = torch.zeros((1, 2, 9), device=DEV)

    def like(a):
        return a.get_likelihood(dict(data), poses, extract_feature=False)

    agent.global_batch = object()
    try:
        with pytest.raises(NotImplementedError, match="like_coupling='object'"):
            like(agent)
    finally:
        agent.global_batch = None
    with pytest.raises(NotImplementedError, match="agent_type='score'"):
        like(_agent(like_coupling="object", agent_type="energy"))
    b = _agent(like_coupling="batch")
    b.object_window = (2, 0)
    with pytest.raises(ValueError, match="object_window"):
        like(b)
    for window in ((1, 1), (2, 2), (1, -1), (0, 0)):
        agent.object_window = window
        try:
            with pytest.raises(ValueError, match="object_window"):
                like(agent)
        finally:
            agent.object_window = None
    # ode_coupling does not switch the likelihood's coupling: the pinned refusal stays
    with pytest.raises(NotImplementedError, match="ode_coupling='object'"):
        like(_agent(sampler_mode=["ode"], ode_coupling="object", like_coupling="batch"))
    # ... and is not consulted under like_coupling='object'
    full = obj3.run(agent)
    _same(full, obj3.run(_agent(sampler_mode=["ode"], ode_coupling="object", like_coupling="object")), 0, obj3.B,
          "an ode_coupling='object' agent")

    # the raw entry: a status and a message, and nothing launched (the outputs keep their fill)
    from genpose2_amd import _lib, arch, sde
    o, h = obj3, agent.heads
    lib, R, K = h.lib, obj3.B * obj3.K, obj3.K
    pobj = h.object_proj(o.feat)
    x = o.poses.reshape(R, 9).clone()
    x[:, 6:] -= o.center.repeat_interleave(K, 0)
    eps = (o.prior.to(DEV) * sde.prior_sigma(arch.SDE_T)).contiguous()
    ws = torch.empty(int(lib.gp_like_object_workspace_size_k(R, K)), dtype=torch.uint8, device=DEV)
    z = torch.full((R, 9), float("nan"), dtype=torch.float64, device=DEV)
    ll = torch.full((R,), float("nan"), dtype=torch.float64, device=DEV)
    nfev, status = (ctypes.c_int * o.B)(), (ctypes.c_int * o.B)()

    def raw(rows, k, rows_total, t0=1e-5, bytes_=None, z_=z):
        return lib.gp_like_sample_object(ctypes.byref(h.w), _p(pobj), _p(x), _p(eps), rows, k, rows_total, t0, 1.0, 1e-5,
                                         1e-5, None if z_ is None else _p(z_), _p(ll), nfev, status, _p(ws),
                                         ws.numel() if bytes_ is None else bytes_, h._s())

    for args, word in (((R - 1, K, R), "whole objects"), ((R, K, R - K), "rows_total"), ((R, K, R + 1), "rows_total"),
                       ((R, K, R, 1.0), "empty integration interval"), ((R, K, R, 1e-5, 1024), "workspace too small"),
                       ((R, K, R, 1e-5, None, None), "null pointer")):
        assert raw(*args) != 0, args
        assert word in lib.gp_last_error().decode(), (args, lib.gp_last_error())
        with pytest.raises(_lib.GenPoseHipError, match=word):
            _lib.check(raw(*args), "like_sample_object")
    torch.cuda.synchronize()
    assert bool(torch.isnan(z).all()) and bool(torch.isnan(ll).all()) and list(nfev) == [0] * o.B
    assert raw(R, K, R) == 0                                         # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ll).all())
    assert list(status) == [1] * o.B and min(nfev) >= 8
    # the agent's call on the same inputs is this entry's
    assert torch.equal(full[0].reshape(-1), ll) and torch.equal(full[1].reshape(R, 9), z)
    assert full[2].tolist() == list(nfev)


# ------------------------------------------------------------------------------------------------- 11. neighbours
def test_neighbours_untouched(agent, obj3, neighbours_before):
    """The batch-coupled get_likelihood on golden_like_ode and the object-coupled ODE sampler on golden_ode_object,
    run before this module's object-coupled likelihood calls and again after them: bitwise equal."""
    obj3.run(agent)
    after = _neighbours()
    for a, b in zip(neighbours_before, after):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)
        else:
            assert np.array_equal(a, b)
