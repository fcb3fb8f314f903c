"""Digests of the ODE entries' outputs on seeded inputs, for a bit-for-bit comparison of two builds (tuning aid, not
a test). One process, one library (GENPOSE_HIP_LIB) and one package tree (ODE_DIGEST_ROOT, default this checkout),
under the GENPOSE2_HEAD_ARITH it is started with; prints one JSON line {case: sha256 prefix}.

    GENPOSE_HIP_LIB=/path/libgenpose_hip.so python scripts/ode_digest.py OUT.json

A comparison against a parent commit takes a checkout of it (PARENT, built) beside this one, one process per side
and arithmetic, each step only after the one before succeeded, then the merge (profiles/r13/ode_bits_vs_parent.json
was made so):

    for A in f16x3 f32; do
      GENPOSE2_HEAD_ARITH=$A ODE_DIGEST_ROOT=PARENT GENPOSE_HIP_LIB=PARENT/genpose2_amd/libgenpose_hip.so \
          python scripts/ode_digest.py parent_$A.json &&
      GENPOSE2_HEAD_ARITH=$A python scripts/ode_digest.py new_$A.json || break
    done
    python scripts/ode_digest.py --compare OUT.json parent_f16x3.json new_f16x3.json parent_f32.json new_f32.json

Cases per shape R (k): one right-hand side (nk 0 and 1) and one host-controlled attempt of the score, likelihood and
energy backends; three device-controlled attempts of the score and energy entries, fused and stage by stage; both
denoise entries; gp_ode_sample / gp_ode_sample_energy with steps 0 and 20 at T0 0.55; the per-object solves; pred_func
on the ODE sampler (device and host controller) and get_likelihood (batch coupling)."""
import ctypes
import hashlib
import json
import os
import sys



def compare(out_path, files):
    """Merge (parent, new) pairs of this script's outputs into one record; exit status 1 on a difference."""
    rec = {"what": "sha256 prefixes of the outputs on the same seeded inputs (scripts/ode_digest.py), parent package "
                   "and library vs this tree's, each in a fresh process", "all_equal": True, "cases": {}}
    for pf, nf in zip(files[::2], files[1::2]):
        p, n = (json.loads(open(f).read()) for f in (pf, nf))
        assert p["arith"] == n["arith"] and list(p["cases"]) == list(n["cases"]), (pf, nf)
        for c, d in p["cases"].items():
            eq = d == n["cases"][c]
            rec["all_equal"] = rec["all_equal"] and eq
            rec["cases"][f"{p['arith']} {c}"] = {"parent": d, "new": n["cases"][c], "equal": eq}
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print("all equal" if rec["all_equal"] else "DIFFERENT", len(rec["cases"]), "cases")
    sys.exit(0 if rec["all_equal"] else 1)


if len(sys.argv) > 2 and sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3:])

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.environ.get("ODE_DIGEST_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from genpose2_amd import _lib, arch, ode, sde, synthetic  # noqa: E402
from genpose2_amd.agent import NoiseFeed, PoseNet  # noqa: E402
from genpose2_amd.config import GenPoseConfig  # noqa: E402

DEV = "cuda:0"
SHAPES = [(50, 25), (4112, 16), (8208, 16)]
OBJECT_SHAPES = [(50, 25), (4112, 16)]
OUT = {}


def vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def np_p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def put(case, *items):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for it in items:
        if isinstance(it, torch.Tensor):
            it = it.detach().cpu().contiguous().numpy()
        h.update(np.ascontiguousarray(it).tobytes() if isinstance(it, np.ndarray) else repr(it).encode())
    OUT[case] = h.hexdigest()[:16]


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_entries(lib, heads, R, k):
    g = torch.Generator().manual_seed(1000 + R)
    nobj = R // k
    pobj = torch.randn(nobj, 768, generator=g).to(DEV)
    x0 = torch.randn(R, 9, generator=g).to(DEV)
    eps = torch.randn(R, 9, generator=g).to(DEV)
    center = torch.randn(nobj, 3, generator=g).to(DEV)
    tag = f"R={R} "
    backends = {
        "ode": lambda: ode.DeviceRk45(heads, pobj, x0.to(torch.float64), k),
        "like": lambda: ode.LikelihoodRk45(heads, pobj, x0, eps, k),
        "energy": lambda: ode.DeviceRk45(heads, pobj, x0.to(torch.float64), k, energy_grad=True),
    }
    for name, make in backends.items():
        be = make()
        be.rhs0(0.5)
        put(tag + name + " rhs nk=0", be.K[0])
        be.rhs_euler(0.5 - 0.01, -0.01)
        put(tag + name + " rhs nk=1", be.f1)
        err = be.attempt(0.5, -0.01)
        put(tag + name + " attempt", *be.K, be.y_new, np.float64(err))
    # three device-controlled attempts from a host-made record, fused and stage by stage
    w, gw = ctypes.byref(heads.w), ctypes.byref(heads.grad_weights)
    rec = ctypes.sizeof(ode.OdeCtl)
    for energy in (False, True):
        for fused in (None, "0"):
            os.environ.pop("GENPOSE2_ODE_FUSED", None)
            if fused is not None:
                os.environ["GENPOSE2_ODE_FUSED"] = fused
            be = backends["energy" if energy else "ode"]()
            be.rhs0(0.5)
            ws = torch.zeros(int(lib.gp_ode_auto_workspace_size(R)), dtype=torch.uint8, device=DEV)
            c0 = ode.OdeCtl(t=0.5, h_abs=0.01, nfev=2)
            c0.kidx[:] = list(range(7))
            ws[:rec].copy_(torch.frombuffer(bytearray(bytes(c0)), dtype=torch.uint8))
            y1 = torch.zeros_like(be.y)
            karr = ode._ptr_array(be.K)
            args = (1e-3, -1.0, 1e-5, 1e-5, arch.SIGMA_MIN, arch.SIGMA_MAX / arch.SIGMA_MIN, float(sde._DIFF_SCALE_T),
                    vp(be.y), vp(y1), karr, np_p(ode._A6), np_p(ode._B6), np_p(ode._E7), R, k, vp(ws), ws.numel())
            for n in range(4):   # control n decides attempt n - 1: the fourth control decides the third attempt
                what = 3 if n < 3 else 1
                if energy:
                    _lib.check(lib.gp_ode_auto_attempt_energy(w, gw, vp(pobj), n, what, *args, None, stream()))
                else:
                    _lib.check(lib.gp_ode_auto_attempt(w, vp(pobj), n, what, *args, stream()))
            put(tag + ("energy" if energy else "ode") + f" auto x3 fused={fused}", be.y, y1, *be.K, ws[:2 * rec])
    os.environ.pop("GENPOSE2_ODE_FUSED", None)
    # denoise
    dws = torch.zeros(int(lib.gp_ode_workspace_size(R)), dtype=torch.uint8, device=DEV)
    xd = x0.to(torch.float64).reshape(-1).contiguous()
    for energy in (False, True):
        pose, q = heads.ode_denoise(pobj, 1e-3, float(sde.sigma(torch.tensor([1e-3]))[0]), 0.04, 0.05, xd, k, center, dws,
                                    energy_grad=energy)
        put(tag + ("energy" if energy else "ode") + " denoise", pose, q)
    # whole samplers
    for steps in (0, 20):
        sws = torch.zeros(int(lib.gp_ode_sample_workspace_size(R)), dtype=torch.uint8, device=DEV)
        pose = torch.zeros(R, 9, dtype=torch.float64, device=DEV)
        q = torch.zeros(R, 7, dtype=torch.float64, device=DEV)
        nfev, status = ctypes.c_int(0), ctypes.c_int(0)
        xs = (x0 * float(sde.prior_sigma(0.55))).contiguous()
        _lib.check(lib.gp_ode_sample(w, vp(pobj), vp(xs), R, k, 0.55, 1e-3, steps, 1e-5, 1e-5, vp(center), vp(pose), vp(q),
                                     ctypes.byref(nfev), ctypes.byref(status), vp(sws), sws.numel(), stream()))
        put(tag + f"ode_sample steps={steps}", pose, q, nfev.value, status.value)
        pose, q, nf, st = heads.ode_sample_energy(pobj, xs, k, center, 0.55, 1e-3, steps or None)
        put(tag + f"ode_sample_energy steps={steps}", pose, q, nf, st)
    if (R, k) in OBJECT_SHAPES:
        for steps in (None, 20):
            pose, q, nf, st = heads.ode_sample_object(pobj, xs, k, center, 0.55, 1e-3, steps)
            put(tag + f"ode_sample_object steps={steps}", pose, q, nf, st)
        z, ll, nf, st = heads.like_sample_object(pobj, x0, eps, k, 1e-3, 1.0)
        put(tag + "like_sample_object", z, ll, nf, st)


def agent_entries(R, k):
    B = R // k
    pts, center = synthetic.make_batch(7, B, 1024)
    prior = np.random.default_rng(R).standard_normal((R, 9)).astype(np.float32)
    data = {"pts": torch.from_numpy(pts).to(DEV), "pts_center": torch.from_numpy(center).to(DEV)}
    agent = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"], sampling_steps=20)).eval()
    pose = None
    for host in (False, True):
        agent.ode_host_control = host
        agent.noise_feed = NoiseFeed(torch.from_numpy(prior))
        pose, q = agent.pred_func(dict(data), repeat_num=k, T0=0.55)
        put(f"R={R} pred_func ode host_control={host}", pose, q, agent.last_nfev)
    agent.noise_feed = NoiseFeed(torch.from_numpy(prior))
    ll, z = agent.get_likelihood(dict(data), pose.view(B, k, -1)[..., :9].to(torch.float32), return_latent=True)
    put(f"R={R} get_likelihood batch", ll, z, agent.last_nfev)


def main():
    lib = _lib.load()
    heads = PoseNet(GenPoseConfig(device=DEV, sampler_mode=["ode"])).eval().heads
    for R, k in SHAPES:
        raw_entries(lib, heads, R, k)
        agent_entries(R, k)
        print("done", R, flush=True)
    line = json.dumps({"lib": _lib.LIB_PATH, "arith": os.environ.get("GENPOSE2_HEAD_ARITH", "default"), "cases": OUT})
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
