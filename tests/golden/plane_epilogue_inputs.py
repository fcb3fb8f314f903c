"""Seeded inputs and runs behind golden_plane_epilogue.npz (make_golden_plane_epilogue.py records it, from the
library of the commit before the activation-plane epilogues changed; tests/test_gpu_plane_epilogue.py runs the same
calls on the tree under test and compares bits).

Every run is recorded as the SHA-256 of its output's bytes (so the sign of a zero counts) and the bit patterns of
a fixed sample of its rows (the first and the last 80 rows, which hold the ragged last tile, and every 41st row in
between), which say where a difference sits when the digest moves. The whole outputs would not fit a fixture file.
"""
import ctypes
import hashlib

import numpy as np
import torch

DEV = "cuda:0"
K_PC, T_PC = 50, 3
# (name, rows, set_pc_small form): 64-candidate ragged tiles on the hybrid kernel the benchmark runs; one ragged
# 16-row tile on the hybrid kernel; the same on the six-product form
PC_CASES = (("r8250_auto", 8250, "auto"), ("r50_fp8", 50, "fp8"), ("r50_f16", 50, "f16"))
SCORE_STEPS = (0, 2)            # rows of the T = 3 step table whose time / sigma score() is evaluated at
ODE_R, ODE_K, ODE_SEED = 4097, 1, 29
ODE_T, ODE_H = 0.3, 2e-3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _rows(n):
    return np.unique(np.concatenate([np.arange(min(80, n)), np.arange(max(0, n - 80), n), np.arange(0, n, 41)]))


def entry(a):
    """{"sha": digest bytes as uint8, "rows": sampled rows' bit patterns} of an array whose first axis is rows."""
    a = np.ascontiguousarray(a)
    sha = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()
    return {"sha": sha, "rows": _bits(a)[_rows(a.shape[0])]}


def _heads():
    from genpose2_amd import device, weights
    return device.HeadModel(weights.synthetic_state_dict("score"), torch.device(DEV))


def pc_case(heads, name, R, form):
    """score() at two times and a T = 3 gp_pc_sample with injected z1 / z2 on R seeded rows."""
    from genpose2_amd import sde
    rng = np.random.default_rng(9100 + R)
    B = R // K_PC
    assert B * K_PC == R
    feat = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32)).to(DEV)
    x0 = torch.from_numpy(rng.standard_normal((R, 9)).astype(np.float32)).to(DEV)
    z = torch.from_numpy(rng.standard_normal((2, T_PC, R, 9)).astype(np.float32)).to(DEV)
    center = torch.zeros((B, 3), device=DEV)
    tab = sde.pc_step_table(T_PC)
    heads.set_pc_small(form)
    heads.set_arith("f16x3")
    try:
        pobj = heads.object_proj(feat)
        tproj = heads.time_proj(torch.from_numpy(tab[:, 0]).to(DEV))
        out = {}
        for j in SCORE_STEPS:
            out[f"{name}_score{j}"] = heads.score(pobj, tproj[j], float(tab[j, 1]), x0, K_PC).cpu().numpy()
        res, q, xs = heads.pc_sample(pobj, tproj, tab, x0.clone(), K_PC, center, z1=z[0].contiguous(),
                                     z2=z[1].contiguous(), want_xs=True)
        out[f"{name}_res"], out[f"{name}_q"], out[f"{name}_xs"] = res.cpu().numpy(), q.cpu().numpy(), xs.cpu().numpy()
    finally:
        heads.set_pc_small("auto")
    return out


def ode_case(heads):
    """One gp_ode_attempt at 4,097 rows (two tiles per workgroup, the last workgroup holds one row): the six stage
    derivatives, y_new and the error scalars."""
    from genpose2_amd import ode
    rng = np.random.default_rng(ODE_SEED)
    R, K = ODE_R, ODE_K
    B = (R + K - 1) // K
    heads.set_arith("f16x3")
    feat = np.maximum(rng.normal(size=(B, 1024)), 0).astype(np.float32)
    pobj = heads.object_proj(torch.from_numpy(feat).to(DEV))
    x = rng.normal(size=(R, 9))
    x[:, 6:] *= 0.3
    be = ode.DeviceRk45(heads, pobj, torch.from_numpy(x.reshape(-1)).to(DEV), K)
    be.rhs0(ODE_T)
    be.attempt(ODE_T, ODE_H)
    torch.cuda.synchronize()
    out = {f"ode_k{s}": be.K[s].cpu().numpy().reshape(R, 9) for s in range(7)}
    out["ode_ynew"] = be.y_new.cpu().numpy().reshape(R, 9)
    out["ode_err"] = be.scal[3:].cpu().numpy().reshape(-1, 1)
    return out


def run_all():
    """name -> full output array of every recorded run."""
    heads = _heads()
    out = {}
    for name, R, form in PC_CASES:
        out.update(pc_case(heads, name, R, form))
    out.update(ode_case(heads))
    return out


def lib_path():
    from genpose2_amd import _lib
    _lib.load()
    return _lib.LIB_PATH, int(ctypes.CDLL(_lib.LIB_PATH).gp_abi_version())
