"""The point encoders off N = 1024 / 2048 and on adversarial geometry, on a real MI355X.

Inputs: the seeded clouds of tests/golden/encoder_edge_inputs.py (tests/test_cpu_encoder_edge.py keeps them adversarial).
Bars: FPS indices, centroids and ball lists bit-exact against the oracle chained level by level; features within 1e-5
of max|ref| per object (the bar of test_encoder_levels_vs_golden and test_fus_encoder_vs_reference_golden); batch
independence bitwise. Every oracle result is computed once per case and shared by the tests that read it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import encoder_edge_inputs as ei
from genpose2_amd import arch
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARITHS = ("split_f16", "f32")
BAR = 1e-5


def _vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_per_object(got, ref):
    """max |got - ref| / max |ref|, the worst object of the batch (leading axis)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    b = ref.shape[0]
    d = np.abs(np.asarray(got, np.float64).reshape(b, -1) - ref.reshape(b, -1)).max(1)
    return float((d / np.maximum(np.abs(ref).reshape(b, -1).max(1), 1e-30)).max())


@pytest.fixture(scope="module")
def lib():
    from genpose2_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def score_sd():
    from genpose2_amd import weights
    return weights.synthetic_state_dict("score", seed=0)


@pytest.fixture(scope="module")
def fus_sd():
    from genpose2_amd import weights
    return weights.synthetic_state_dict("score_pointwise", seed=0)


@pytest.fixture(scope="module")
def enc(score_sd):
    from genpose2_amd.device import EncoderModel
    return EncoderModel(score_sd, torch.device(DEV))


@pytest.fixture(scope="module")
def fus(fus_sd):
    from genpose2_amd.fus_encoder import FusEncoderModel
    return FusEncoderModel(fus_sd, torch.device(DEV))


# ---------------------------------------------------------------- shared references
def oracle_chain(pts):
    """FPS + both ball queries of the four levels, each level over the previous level's centroids."""
    cur, out = pts, []
    for lv in range(4):
        fidx = oracle.furthest_point_sample(cur, arch.NPOINTS[lv])
        new = np.take_along_axis(cur, fidx[..., None].astype(np.int64), 1)
        balls = [oracle.ball_query(r, ns, cur, new) for r, ns in zip(arch.RADII[lv], arch.NSAMPLES[lv])]
        out.append(dict(fps_idx=fidx, new_xyz=new, ball_idx=balls))
        cur = new
    return out


@functools.lru_cache(maxsize=None)
def geometry_ref(name):
    pts = ei.case_points(ei.GEOMETRY_CASES[name])
    return pts, oracle_chain(pts)


_ENC_REF = {}


def encoder_ref(name, sd):
    if name not in _ENC_REF:
        pts = ei.case_points(ei.ENCODER_CASES[name])
        _ENC_REF[name] = (pts,) + tuple(oracle.encoder_forward(sd, pts, return_levels=True))
    return _ENC_REF[name]


def assert_geometry(levels, ref, tag):
    """Bit-exact FPS indices, centroids and both ball lists of levels 0-3; the message names the first
    mismatching (object, centroid)."""
    for lv in range(4):
        for key, got, want in [("fps_idx", levels[lv]["fps_idx"], ref[lv]["fps_idx"]),
                               ("new_xyz", levels[lv]["new_xyz"], ref[lv]["new_xyz"]),
                               ("ball_idx a", levels[lv]["ball_idx"][0], ref[lv]["ball_idx"][0]),
                               ("ball_idx b", levels[lv]["ball_idx"][1], ref[lv]["ball_idx"][1])]:
            got = got.cpu().numpy()
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)[0]
                raise AssertionError(f"{tag}: level {lv} {key} differs first at {tuple(bad)}: got "
                                     f"{got[tuple(bad[:2])]} want {want[tuple(bad[:2])]}")


# ---------------------------------------------------------------- a. geometry only
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("name", list(ei.GEOMETRY_CASES))
def test_geometry_vs_oracle(name, overlap, enc):
    """EncoderModel.geometry() alone (the FPS chain in each of its size classes, then ball_query_kernel<2>), with
    levels 1-3 on the side stream and without: every index against the oracle, no MLP involved."""
    pts, ref = geometry_ref(name)
    B, N = pts.shape[:2]
    enc.workspace(B, N).fill_(0xFF)   # nothing a previous case left can pass for this one's lists
    enc.geometry_overlap = overlap
    try:
        g = enc.geometry(_dev(pts))
        torch.cuda.synchronize()
    finally:
        enc.geometry_overlap = True
    assert (g.event0 is not None) == overlap
    assert_geometry(enc.levels(B, N, g.ws), ref, f"{name} overlap={overlap}")


# ---------------------------------------------------------------- b. whole plain encoder
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(ei.ENCODER_CASES))
def test_encoder_vs_oracle(name, arith, enc, score_sd):
    """gp_encoder_forward on the edge clouds: geometry bit-exact, features of levels 0-3 and the 1024-d output
    within 1e-5 of max|ref| per object."""
    pts, ref_out, ref = encoder_ref(name, score_sd)
    B, N = pts.shape[:2]
    enc.workspace(B, N).fill_(0xFF)
    enc.set_arith(arith)
    try:
        feat, ws = enc.forward(_dev(pts), return_workspace=True)
        torch.cuda.synchronize()
    finally:
        enc.set_arith("split_f16")
    levels = enc.levels(B, N, ws)
    assert_geometry(levels, ref, f"{name} {arith}")
    errs = {lv: rel_per_object(levels[lv]["features"].transpose(1, 2), ref[lv]["features"]) for lv in range(4)}
    errs["out"] = rel_per_object(feat, ref_out)
    print(f"encoder {name} {arith}: rel errors {errs}")
    assert max(errs.values()) < BAR, f"{name} {arith}: geometry exact, features off: {errs}"


# ---------------------------------------------------------------- c. batch independence
INDEP_B = (1, 2, 5, 7, 33)


@functools.lru_cache(maxsize=None)
def indep_points(src):
    if src == "edge600":
        return np.stack([ei.cloud(ei.KINDS[i % 6], 600, 100 + i) for i in range(max(INDEP_B))])
    from genpose2_amd import synthetic
    return synthetic.make_batch(7, max(INDEP_B), 1024, n_unique_every=4)[0]


def _snapshot(enc, pts):
    """Everything forward() leaves per object: the output, and per level the indices and features."""
    B, N = pts.shape[:2]
    enc.workspace(B, N).fill_(0xFF)
    feat, ws = enc.forward(_dev(pts), return_workspace=True)
    torch.cuda.synchronize()
    out = {"out": feat.cpu()}
    for lv, d in enumerate(enc.levels(B, N, ws)[:4]):
        out.update({f"l{lv}_fps": d["fps_idx"].cpu(), f"l{lv}_xyz": d["new_xyz"].cpu(),
                    f"l{lv}_ball_a": d["ball_idx"][0].cpu(), f"l{lv}_ball_b": d["ball_idx"][1].cpu(),
                    f"l{lv}_feat": d["features"].cpu()})
    return out


_SINGLES = {}


def singles(enc, src, arith):
    if (src, arith) not in _SINGLES:
        pts = indep_points(src)
        _SINGLES[src, arith] = [_snapshot(enc, pts[i:i + 1]) for i in range(len(pts))]
    return _SINGLES[src, arith]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B", INDEP_B)
@pytest.mark.parametrize("src", ["edge600", "synth1024"])
def test_batch_independence_per_level(src, B, arith, enc):
    """Object i of a batch of B equals its single-object run bit for bit: indices, centroids, ball lists, the
    features of levels 0-3 and the output. B = 2, 5, 7, 33 leave every tile loop over objects a partial last pass."""
    enc.set_arith(arith)
    try:
        one = singles(enc, src, arith)
        got = _snapshot(enc, indep_points(src)[:B])
    finally:
        enc.set_arith("split_f16")
    for i in range(B):
        for k, v in got.items():
            assert torch.equal(v[i], one[i][k][0]), f"{src} {arith} B={B}: object {i} {k} differs from its own run"


# ---------------------------------------------------------------- d. level 0 on ragged B * N
def point_features(n, obj):
    """(n, 384) seeded normal(0, 1) features of object `obj` of a case (the same in every batch it joins)."""
    return np.random.Generator(np.random.PCG64([7100, n, obj])).standard_normal((n, arch.DINO_DIM), dtype=np.float32)


def run_level0(lib, model, pts, feats):
    """gp_encoder_fps + gp_sa_level(level 0) of `model` (its packed weights and table) -> (B, 512, 96) cpu."""
    from genpose2_amd import _lib
    B, N = pts.shape[:2]
    p, f = _dev(pts), (None if feats is None else _dev(feats))
    # NaN-filled: a projection row the kernel left out cannot read as a value an earlier run left in the block
    ws = torch.full((int(lib.gp_encoder_workspace_size(B, N)),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((B, arch.NPOINTS[0], arch.level_out_channels(0)), float("nan"), device=DEV)
    _lib.check(lib.gp_encoder_fps(_vp(p), B, N, _vp(ws), ws.numel(), _s()), "encoder_fps")
    _lib.check(lib.gp_sa_level(_vp(model.wbuf), model.offsets.ctypes.data_as(_lib.c_int64_p), 0,
                               0 if feats is None else feats.shape[2], _vp(p), B, N, _vp(f), _vp(ws), ws.numel(),
                               _vp(out), _s()), "sa_level 0")
    torch.cuda.synchronize()
    return out.cpu()


_L0_REF = {}


def level0_ref(name, c_prev, sd):
    if (name, c_prev) not in _L0_REF:
        pts = ei.case_points(ei.LEVEL0_CASES[name])
        B, N = pts.shape[:2]
        feats = np.stack([point_features(N, i) for i in range(B)]) if c_prev else None
        branches = (arch.fus_sa_branches() if c_prev else arch.sa_branches())[0]
        _, _, ref = oracle.sa_level(sd, "pts_encoder.", 0, branches, pts,
                                    None if feats is None else feats.transpose(0, 2, 1))
        _L0_REF[name, c_prev] = (pts, feats, ref.transpose(0, 2, 1))   # point-major (B, 512, 96)
    return _L0_REF[name, c_prev]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("c_prev", [arch.DINO_DIM, 0], ids=["feat384", "xyz"])
@pytest.mark.parametrize("name", list(ei.LEVEL0_CASES))
def test_level0_ragged_tail(name, c_prev, arith, lib, enc, fus, score_sd, fus_sd):
    """Level 0 where B * N is no multiple of a projection workgroup (B * N % 256 = 1, 88, 8, 254): proj_feat_kernel
    (384 point features, the pointwise encoder) and proj_xyz_kernel (none, the plain encoder) leave through their
    tail guards. Against the oracle's level within 1e-5 of max|ref| per object; and every object bitwise equal to
    its run alone (another tail) and, for one-object cases, to its run behind another object."""
    model, sd = (fus, fus_sd) if c_prev else (enc, score_sd)
    pts, feats, ref = level0_ref(name, c_prev, sd)
    B, N = pts.shape[:2]
    assert (B * N) % 256 != 0
    model.set_arith(arith)
    try:
        got = run_level0(lib, model, pts, feats)
        alone = [run_level0(lib, model, pts[i:i + 1], None if feats is None else feats[i:i + 1]) for i in range(B)]
        if B == 1:   # the same object as row 1 of a batch of two: its points start mid-workgroup
            other = ei.cloud("lattice", N, 9)[None]
            pair = run_level0(lib, model, np.concatenate([other, pts]),
                              None if feats is None else np.concatenate([point_features(N, 9)[None], feats]))
    finally:
        model.set_arith("split_f16")
    assert torch.isfinite(got).all()
    err = rel_per_object(got, ref)
    print(f"level 0 {name} c_prev={c_prev} {arith}: rel {err:.2e}")
    assert err < BAR, f"level 0 {name} c_prev={c_prev} {arith}: rel {err:.2e}"
    for i in range(B):
        assert torch.equal(got[i], alone[i][0]), f"object {i} of {name} differs from its run alone"
    if B == 1:
        assert torch.equal(pair[1], got[0]), f"{name}: the object differs behind another object"


# ---------------------------------------------------------------- e. whole fused encoder
_FUS_REF = {}


def fus_ref(name, sd):
    if name not in _FUS_REF:
        import make_golden_fus as mf
        pts = ei.case_points(ei.FUS_CASES[name])
        rgb = mf.rgb_features(pts.shape[0], pts.shape[1])
        _FUS_REF[name] = (pts, rgb) + tuple(oracle.fus_encoder_forward(sd, pts, rgb, return_levels=True)) + \
            (oracle_chain(pts),)
    return _FUS_REF[name]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(ei.FUS_CASES))
def test_fus_encoder_vs_oracle(name, arith, fus, enc, fus_sd):
    """The DINO-pointwise fused encoder on the edge clouds: geometry bit-exact, then every level's sa / tf / fused
    entry and the output within 1e-5 of max|ref| per object."""
    pts, rgb, ref_out, ref, chain = fus_ref(name, fus_sd)
    B, N = pts.shape[:2]
    fus.workspace(B, N).fill_(0xFF)
    fus.set_arith(arith)
    try:
        out, levels = fus.forward(_dev(pts), _dev(rgb), return_levels=True)
        torch.cuda.synchronize()
    finally:
        fus.set_arith("split_f16")
    assert_geometry(enc.levels(B, N, fus._ws), chain, f"fused {name} {arith}")
    errs = {(lv, k): rel_per_object(levels[lv][k].transpose(1, 2), ref[lv][k])
            for lv in range(5) for k in ("fused", "sa", "tf") if k in ref[lv]}
    errs["out"] = rel_per_object(out, ref_out)
    print(f"fused encoder {name} {arith}: rel errors {errs}")
    bad = {k: v for k, v in errs.items() if not v < BAR}
    assert not bad, f"fused {name} {arith}: geometry exact, entries over 1e-5: {bad}"


# ---------------------------------------------------------------- f. refusals
@pytest.mark.parametrize("N", [511, 8193])
def test_out_of_range_n_is_refused_and_writes_nothing(N, lib, enc, fus):
    from genpose2_amd import _lib
    B = 2
    pts = _dev(ei.batch([("lattice", 1), ("mixed", 1)], N))
    feats = torch.zeros(B, N, arch.DINO_DIM, device=DEV)
    ws = torch.full((int(lib.gp_encoder_workspace_size(B, 8192)),), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((B, 1024), 7.0, device=DEV)
    tab = enc.offsets.ctypes.data_as(_lib.c_int64_p)
    calls = {
        "encoder_forward": lambda: lib.gp_encoder_forward(_vp(enc.wbuf), tab, _vp(pts), B, N, _vp(ws), ws.numel(),
                                                          _vp(out), _s()),
        "encoder_fps": lambda: lib.gp_encoder_fps(_vp(pts), B, N, _vp(ws), ws.numel(), _s()),
        "encoder_geometry": lambda: lib.gp_encoder_geometry(_vp(pts), B, N, _vp(ws), ws.numel(), _s()),
        "sa_level": lambda: lib.gp_sa_level(_vp(fus.wbuf), fus.offsets.ctypes.data_as(_lib.c_int64_p), 0,
                                            arch.DINO_DIM, _vp(pts), B, N, _vp(feats), _vp(ws), ws.numel(), _vp(out),
                                            _s()),
    }
    for what, call in calls.items():
        assert call() != 0, what
        msg = lib.gp_last_error().decode()
        assert msg == f"encoder: need 1<=b and 512<=n<=8192 (b={B} n={N})", (what, msg)
        with pytest.raises(_lib.GenPoseHipError, match="512<=n<=8192"):
            _lib.check(call(), what)
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((out == 7.0).all())
