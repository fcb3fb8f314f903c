"""The C ABI driven the way a non-Python host would (cgo / JNI / C++), on a real MI355X: weights packed and
uploaded by gp_weights_pack from plain state-dict arrays, then the encoder, head projections and the PC
sampler called through the handle's structs. The packed bytes equal pack.py's (tests/test_cpu_host.py), so
results must equal PoseNet's bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _pack(kind_id, sd):
    from genpose2_amd import _lib
    lib = _lib.load()
    keys = [k for k, v in sd.items() if v.dtype == np.float32]
    arrs = [np.ascontiguousarray(sd[k], np.float32) for k in keys]
    names = (ctypes.c_char_p * len(keys))(*[k.encode() for k in keys])
    data = (ctypes.c_void_p * len(keys))(*[a.ctypes.data for a in arrs])
    numel = np.array([a.size for a in arrs], np.int64)
    h = ctypes.c_void_p()
    _lib.check(lib.gp_weights_pack(kind_id, len(keys), ctypes.cast(names, ctypes.c_void_p),
                                   ctypes.cast(data, ctypes.c_void_p), numel.ctypes.data, ctypes.byref(h)),
               "weights_pack")
    return lib, h


def test_weights_pack_handle_drives_pc_pred_func():
    from genpose2_amd import _lib, arch, sde, synthetic, weights
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    B, K, T = 3, 6, 20
    sd = weights.synthetic_state_dict("score")
    lib, h = _pack(0, sd)
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pts_np, center_np = synthetic.make_batch(17, B, 1024)
        pts, center = torch.from_numpy(pts_np).to(DEV), torch.from_numpy(center_np).to(DEV)
        # encoder through the handle
        tab = _lib.c_int64_p()
        wbuf = lib.gp_weights_encoder(h, ctypes.byref(tab))
        assert wbuf
        ws = torch.empty(int(lib.gp_encoder_workspace_size(B, 1024)), dtype=torch.uint8, device=DEV)
        feat = torch.empty(B, 1024, device=DEV)
        _lib.check(lib.gp_encoder_forward(ctypes.c_void_p(wbuf), tab, _vp(pts), B, 1024, _vp(ws), ws.numel(),
                                          _vp(feat), s), "encoder_forward")
        # heads + PC sampler through the handle's gp_head_weights
        hw = lib.gp_weights_heads(h)
        pobj = torch.empty(B, 768, device=DEV)
        _lib.check(lib.gp_head_object_proj(hw, _vp(feat), B, _vp(pobj), s))
        tab_np = sde.pc_step_table(T)
        tvals = torch.from_numpy(np.ascontiguousarray(tab_np[:, 0])).to(DEV)
        tproj = torch.empty(T, 768, device=DEV)
        _lib.check(lib.gp_head_time_proj(hw, _vp(tvals), T, _vp(tproj), s))
        rng = np.random.default_rng(9)
        prior = rng.standard_normal((B * K, 9)).astype(np.float32)
        z1 = torch.from_numpy(rng.standard_normal((T, B * K, 9)).astype(np.float32)).to(DEV)
        z2 = torch.from_numpy(rng.standard_normal((T, B * K, 9)).astype(np.float32)).to(DEV)
        x = (torch.from_numpy(prior).to(DEV) * sde.prior_sigma(arch.SDE_T)).contiguous()   # as PoseNet.pred_func
        R = B * K
        res, q = torch.empty(R, 9, device=DEV), torch.empty(R, 7, device=DEV)
        pws = torch.empty(int(lib.gp_pc_workspace_size(R)), dtype=torch.uint8, device=DEV)
        stab = np.ascontiguousarray(tab_np, np.float32)
        _lib.check(lib.gp_pc_sample(hw, _vp(pobj), _vp(tproj), stab.ctypes.data_as(ctypes.c_void_p), T, _vp(x), R, K,
                                    _vp(center), _vp(z1), _vp(z2), ctypes.c_uint64(0), ctypes.c_float(arch.SNR),
                                    _vp(res), _vp(q), None, _vp(pws), pws.numel(), s), "pc_sample")
        torch.cuda.synchronize()
        # the same call through PoseNet (pack.py buffers)
        agent = PoseNet(GenPoseConfig(device=DEV, sampling_steps=T)).eval()
        agent.noise_feed = NoiseFeed(torch.from_numpy(prior), z1.cpu(), z2.cpu())
        data = {"pts": pts, "pts_center": center}
        pose, pq = agent.pred_func(data, repeat_num=K)
        torch.cuda.synchronize()
        assert torch.equal(feat, data["pts_feat"])
        assert torch.equal(res.view(B, K, 9), pose)
        assert torch.equal(q.view(B, K, 7), pq)
    finally:
        lib.gp_weights_free(h)


def test_weights_pack_scale_handle():
    from genpose2_amd import _lib, weights
    from genpose2_amd.device import ScaleModel
    sd = weights.synthetic_state_dict("scale")
    lib, h = _pack(2, sd)
    try:
        assert not lib.gp_weights_heads(h) and not lib.gp_weights_encoder(h, None)
        rng = np.random.default_rng(2)
        axes = torch.from_numpy(rng.normal(size=(4, 3, 3)).astype(np.float32)).to(DEV)
        feat = torch.from_numpy(rng.normal(size=(4, 1024)).astype(np.float32)).to(DEV)
        out = torch.empty(4, 3, device=DEV)
        _lib.check(lib.gp_scale_forward(lib.gp_weights_scale(h), _vp(axes), _vp(feat), 4, _vp(out),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        ref = ScaleModel(sd, torch.device(DEV)).forward(axes, feat)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    finally:
        lib.gp_weights_free(h)


def _handle_features(lib, h, pts, B, N, s):
    from genpose2_amd import _lib
    tab = _lib.c_int64_p()
    wbuf = lib.gp_weights_encoder(h, ctypes.byref(tab))
    ws = torch.empty(int(lib.gp_encoder_workspace_size(B, N)), dtype=torch.uint8, device=DEV)
    feat = torch.empty(B, 1024, device=DEV)
    _lib.check(lib.gp_encoder_forward(ctypes.c_void_p(wbuf), tab, _vp(pts), B, N, _vp(ws), ws.numel(), _vp(feat), s))
    hw = lib.gp_weights_heads(h)
    pobj = torch.empty(B, 768, device=DEV)
    _lib.check(lib.gp_head_object_proj(hw, _vp(feat), B, _vp(pobj), s))
    return hw, pobj


def test_c_host_pc_sampler_with_c_step_table():
    """The PC sampler driven with nothing from genpose2_amd's Python (sde.py, PoseNet): gp_weights_pack,
    encoder, gp_pc_step_table, gp_head_time_proj, gp_pc_sample -- against the reference's own
    golden_pc_k10_t100 at the golden tolerances (rotation 1e-4 absolute, translation 1e-5 relative)."""
    from conftest import golden
    from genpose2_amd import _lib, weights
    g = golden("pc_k10_t100")
    K, T = int(g["K"]), int(g["T"])
    lib, h = _pack(0, weights.synthetic_state_dict("score"))
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pts, center = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["pts_center"]).to(DEV)
        B = pts.shape[0]
        hw, pobj = _handle_features(lib, h, pts, B, 1024, s)
        tab = np.zeros((T, 5), np.float32)
        _lib.check(lib.gp_pc_step_table(T, ctypes.c_float(1e-5), tab.ctypes.data_as(ctypes.c_void_p)))
        tvals = torch.from_numpy(np.ascontiguousarray(tab[:, 0])).to(DEV)
        tproj = torch.empty(T, 768, device=DEV)
        _lib.check(lib.gp_head_time_proj(hw, _vp(tvals), T, _vp(tproj), s))
        R = B * K
        x = (torch.from_numpy(g["prior"]).to(DEV) * np.float32(0.01 * 5000.0 ** 1.0)).contiguous()   # sde.py:30-34
        z1, z2 = torch.from_numpy(g["z1"]).to(DEV), torch.from_numpy(g["z2"]).to(DEV)
        res, q = torch.empty(R, 9, device=DEV), torch.empty(R, 7, device=DEV)
        pws = torch.empty(int(lib.gp_pc_workspace_size(R)), dtype=torch.uint8, device=DEV)
        _lib.check(lib.gp_pc_sample(hw, _vp(pobj), _vp(tproj), tab.ctypes.data_as(ctypes.c_void_p), T, _vp(x), R, K,
                                    _vp(center), _vp(z1), _vp(z2), ctypes.c_uint64(0), ctypes.c_float(0.16),
                                    _vp(res), _vp(q), None, _vp(pws), pws.numel(), s), "pc_sample")
        torch.cuda.synchronize()
        p, ref = res.view(B, K, 9).cpu().numpy(), g["pred_pose"]
        assert np.abs(p[..., :6] - ref[..., :6]).max() < 1e-4
        assert np.abs(p[..., 6:] - ref[..., 6:]).max() / np.abs(ref[..., 6:]).max() < 1e-5
    finally:
        lib.gp_weights_free(h)


def _c_ode(lib, hw, pobj, prior, T0, steps, K, center, s):
    from genpose2_amd import _lib
    R = prior.shape[0]
    x0 = (torch.from_numpy(prior).to(DEV) * (0.01 * 5000.0 ** T0)).contiguous()   # prior(sigma(T0)), sde.py:30-34
    pose = torch.empty(R, 9, dtype=torch.float64, device=DEV)
    q = torch.empty(R, 7, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.gp_ode_sample_workspace_size(R)), dtype=torch.uint8, device=DEV)
    nfev, status = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.gp_ode_sample(hw, _vp(pobj), _vp(x0), R, K, T0, 1e-5, steps, 1e-5, 1e-5, _vp(center), _vp(pose),
                                 _vp(q), ctypes.byref(nfev), ctypes.byref(status), _vp(ws), ws.numel(), s), "ode_sample")
    torch.cuda.synchronize()
    return pose.cpu().numpy(), q.cpu().numpy(), nfev.value, status.value


@pytest.mark.parametrize("tag,rot_tol,tr_rel,same_nfev", [("t055_s20", 1e-4, 1e-5, True),
                                                         ("t1_none", 5e-4, 1e-4, False)])
def test_c_host_ode_sample_vs_golden(tag, rot_tol, tr_rel, same_nfev):
    """gp_ode_sample (select_initial_step + device-controlled RK45 + dense output + denoise in one C
    call) against the reference's golden_ode at the golden tolerances of test_ode_pred_func_vs_golden:
    nfev identical at T0=0.55; from T0=1 (sigma = 50) the adaptive controller may take a different
    accept/reject path on last-bit differences (as the oracle, which runs scipy itself, does), so there
    nfev is only held within 5 % and the poses at 5e-4 / 1e-4."""
    from conftest import golden
    from genpose2_amd import weights
    g = golden("ode")
    steps = int(g[f"{tag}_steps"])
    lib, h = _pack(0, weights.synthetic_state_dict("score"))
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pts = torch.from_numpy(g[f"{tag}_pts"]).to(DEV)
        center = torch.from_numpy(g[f"{tag}_pts_center"]).to(DEV)
        B = pts.shape[0]
        hw, pobj = _handle_features(lib, h, pts, B, 1024, s)
        pose, q, nfev, status = _c_ode(lib, hw, pobj, g[f"{tag}_prior"], float(g[f"{tag}_T0"]), max(steps, 0), 5,
                                       center, s)
        ref = g[f"{tag}_pred_pose"].reshape(-1, 9)
        print(tag, "nfev", nfev, "reference", int(g[f"{tag}_nfev"]))
        assert status == 1
        assert nfev == int(g[f"{tag}_nfev"]) if same_nfev else abs(nfev - int(g[f"{tag}_nfev"])) <= 0.05 * nfev
        assert np.abs(pose[:, :6] - ref[:, :6]).max() < rot_tol
        assert np.abs(pose[:, 6:] - ref[:, 6:]).max() / np.abs(ref[:, 6:]).max() < tr_rel
    finally:
        lib.gp_weights_free(h)


def test_c_host_ode_sample_large_rows():
    """gp_ode_sample at R = 4800 (ode_r4800, the shipped T0=0.55): nfev identical to the reference's and
    the north-star bar against the reference (rotation 1e-4 absolute, translation 1e-5 relative). Not
    the calibrated 2x bar PoseNet's path meets: the C host forms sigma(t) with a correctly rounded power
    where torch uses Sleef's (1-2 ulp apart on 1.7 % of times, gp_pc_step_table), which moves
    select_initial_step's h0 by ~1e-7 relative and so the whole RK45 step sequence -- the two solutions
    then differ at the solver's tolerance scale (rtol = atol = 1e-5), as any two RK45 runs do."""
    import large_noise
    from conftest import golden
    from genpose2_amd import weights
    from genpose2_amd.agent import NoiseFeed, PoseNet
    from genpose2_amd.config import GenPoseConfig
    name = "ode_r4800"
    gl = golden(f"large_{name}")
    _, _, B, K, _, T0, _ = large_noise.CASES[name]
    pts_np, center_np, prior, _, _ = large_noise.inputs(name)
    lib, h = _pack(0, weights.synthetic_state_dict("score"))
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pts, center = torch.from_numpy(pts_np).to(DEV), torch.from_numpy(center_np).to(DEV)
        hw, pobj = _handle_features(lib, h, pts, B, 1024, s)
        pose, q, nfev, status = _c_ode(lib, hw, pobj, prior, T0, 0, K, center, s)
    finally:
        lib.gp_weights_free(h)
    assert status == 1 and nfev == int(gl["nfev"])
    ref = gl["pred_pose"].reshape(-1, 9)
    rot = np.abs(pose[:, :6] - ref[:, :6]).max()
    tr = np.abs(pose[:, 6:] - ref[:, 6:]).max() / np.abs(ref[:, 6:]).max()
    print("C-host ODE R=4800: rotation", rot, "translation rel", tr, "nfev", nfev)
    assert rot < 1e-4 and tr < 1e-5
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=None)).eval()
    agent.noise_feed = NoiseFeed(torch.from_numpy(prior))
    ppose, _ = agent.pred_func({"pts": pts, "pts_center": center}, repeat_num=K, T0=T0)
    assert agent.last_nfev == nfev
    assert np.abs(ppose.cpu().numpy().reshape(-1, 9)[:, :6] - pose[:, :6]).max() < 1e-4


def test_c_host_pc_sample_global_one_shard_and_exchange_failure():
    """gp_pc_sample_global through the C ABI: one shard of a one-shard batch (the exchange callback is called
    after every scoring launch with the slot the launch wrote, and has nothing to gather) gives gp_pc_sample's
    bits; a callback that fails ends the call with an error instead of sampling on."""
    from genpose2_amd import _lib, weights
    B, K, T, N = 4, 64, 12, 1024
    lib, h = _pack(0, weights.synthetic_state_dict("score"))
    try:
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        from genpose2_amd import synthetic
        pts, center = synthetic.make_batch(3, B, N)
        pts, center = torch.from_numpy(pts).to(DEV), torch.from_numpy(center).to(DEV)
        hw, pobj = _handle_features(lib, h, pts, B, N, s)
        tab = np.zeros((T, 5), np.float32)
        _lib.check(lib.gp_pc_step_table(T, ctypes.c_float(1e-5), tab.ctypes.data_as(ctypes.c_void_p)))
        tproj = torch.empty(T, 768, device=DEV)
        _lib.check(lib.gp_head_time_proj(hw, _vp(torch.from_numpy(np.ascontiguousarray(tab[:, 0])).to(DEV)), T,
                                         _vp(tproj), s))
        R = B * K
        x0 = torch.randn(R, 9, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 50.0
        pws = torch.empty(int(lib.gp_pc_workspace_size(R)), dtype=torch.uint8, device=DEV)

        def plain():
            x, res, q = x0.clone(), torch.empty(R, 9, device=DEV), torch.empty(R, 7, device=DEV)
            _lib.check(lib.gp_pc_sample(hw, _vp(pobj), _vp(tproj), tab.ctypes.data_as(ctypes.c_void_p), T, _vp(x), R, K,
                                        _vp(center), None, None, ctypes.c_uint64(9), ctypes.c_float(0.16), _vp(res),
                                        _vp(q), None, _vp(pws), pws.numel(), s), "pc_sample")
            return res

        n = int(lib.gp_pc_global_partials(R, R, 1, 1))
        part = torch.zeros(2 * n, device=DEV)
        calls = []

        def run_global(fail_at=None):
            def cb(ctx, step, slot, nn, stream):
                calls.append((step, slot - part.data_ptr(), nn))
                return -1 if step == fail_at else 0
            fn = _lib.PC_EXCHANGE_FN(cb)
            x, res, q = x0.clone(), torch.empty(R, 9, device=DEV), torch.empty(R, 7, device=DEV)
            rc = lib.gp_pc_sample_global(hw, _vp(pobj), _vp(tproj), tab.ctypes.data_as(ctypes.c_void_p), T, _vp(x), R,
                                         K, _vp(center), ctypes.c_uint64(9), ctypes.c_float(0.16), _vp(res), _vp(q),
                                         None, R, 0, 0, 1, R, _vp(part), fn, None, _vp(pws), pws.numel(), s)
            return rc, res
        ref = plain()
        rc, got = run_global()
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        assert [c[0] for c in calls] == list(range(T)) and all(c[2] == n for c in calls)
        assert [c[1] for c in calls] == [4 * n * (i & 1) for i in range(T)]   # slot i & 1 of the partials
        calls.clear()
        rc, _ = run_global(fail_at=3)
        torch.cuda.synchronize()
        assert rc != 0 and [c[0] for c in calls] == [0, 1, 2, 3]
        assert "exchange" in lib.gp_last_error().decode()
    finally:
        lib.gp_weights_free(h)


@pytest.fixture(scope="module")
def ode_entry_args():
    """Valid small arguments of the six raw ODE entries (R = 16 rows, one object of k = 16), filled outputs."""
    from genpose2_amd import _lib, ode
    from genpose2_amd.agent import PoseNet
    from genpose2_amd.config import GenPoseConfig
    R, K, fill = 16, 16, 7.25
    heads = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"])).eval().heads
    gen = torch.Generator(DEV).manual_seed(11)
    f64 = dict(dtype=torch.float64, device=DEV)
    a = dict(lib=_lib.load(), R=R, K=K, fill=fill, heads=heads,
             pobj=torch.randn(1, 768, device=DEV, generator=gen),
             y=torch.randn(R * 10, generator=gen, **f64), eps=torch.randn(R, 9, device=DEV, generator=gen),
             k=[torch.full((R * 10,), fill, **f64) for _ in range(7)], y1=torch.full((R * 10,), fill, **f64),
             err=torch.full((1,), fill, **f64), ws=torch.zeros(int(_lib.load().gp_ode_workspace_size(R)),
                                                              dtype=torch.uint8, device=DEV))
    a["scal"] = ode.stage_scalars([0.5 - 0.01 * c for c in (0.2, 0.3, 0.8, 8 / 9, 1.0, 1.0)])
    return a


@pytest.mark.parametrize("name", ["ode_rhs", "like_rhs", "ode_rhs_energy", "ode_attempt", "like_attempt",
                                  "ode_attempt_energy"])
def test_ode_entries_refuse_an_empty_workspace(ode_entry_args, name):
    """Each raw right-hand side and host-controlled attempt, called with valid buffers and workspace_bytes = 0,
    returns a status before any launch; the message carries the entry's own name and "workspace too small"."""
    from genpose2_amd import ode
    a = ode_entry_args
    lib, h, R, K = a["lib"], a["heads"], a["R"], a["K"]
    t32, sig, coef = a["scal"]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    np_p = lambda v: v.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    head = (ctypes.byref(h.w), ctypes.byref(h.grad_weights)) if name.endswith("_energy") else (ctypes.byref(h.w),)
    extra = (_vp(a["eps"]),) if name.startswith("like_") else ()
    kptr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in a["k"]])
    if "_rhs" in name:
        rc = getattr(lib, "gp_" + name)(*head, _vp(a["pobj"]), float(t32[0]), float(sig[0]), float(coef[0]),
                                        _vp(a["y"]), *extra, None, None, 0, 0.0, R, K, _vp(a["k"][1]), _vp(a["ws"]),
                                        0, s)
    else:
        rc = getattr(lib, "gp_" + name)(*head, _vp(a["pobj"]), np_p(t32), np_p(sig), np_p(coef), _vp(a["y"]), *extra,
                                        kptr, np_p(ode._A6), np_p(ode._B6), np_p(ode._E7), -0.01, 1e-5, 1e-5, R, K,
                                        _vp(a["y1"]), _vp(a["err"]), _vp(a["ws"]), 0, s)
    msg = lib.gp_last_error().decode()
    assert rc != 0, name
    assert name + ":" in msg and "workspace too small" in msg, (name, msg)
    torch.cuda.synchronize()
    for t in a["k"] + [a["y1"], a["err"]]:
        assert bool((t == a["fill"]).all())
    assert not bool(a["ws"].any())
