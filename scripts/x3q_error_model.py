"""CPU gate for the hybrid f16 + block-scaled FP8 form of the head trunk's two per-candidate GEMMs
(pose_encoder.2 and head layer 1's pose block; gp_head.h). numpy only, no GPU.

Three forms of the two GEMMs are emulated on the 12,800 states the reference's PC run entered steps 1 and
400 with (tests/golden/golden_large_steps_r12800.npz, weights.synthetic_state_dict("score")):

  f16x3   today's trunk: three f16 planes per operand (hi, mid, lo of the value times its power-of-two
          scale), six products per 32-deep chunk; hi*hi into `acc`, the five cross products into `cor`
          (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid in the kernel's order), one fp32 rounding per MFMA,
          acc + cor once per layer
  hybrid  hi*hi into `acc`; mid*hi and hi*mid into `cor` per 32-deep chunk; the three products of plane
          order 2 (w_hi*a_lo, w_mid*a_mid, w_lo*a_hi) on v_mfma_scale_f32_16x16x128_f8f6f4 with OCP e4m3fn
          operands, one MFMA each per 128-deep group, into `cor` as well (product k of group g after
          chunk 4g + k's two f16 cross products, the kernel's order); acc + cor once per layer
  fp32    exact fp32: one sequential fp32 FMA chain over K per output (the reference's arithmetic)

The e4m3 operands are the f16 planes times a power of two (round to nearest even, subnormals down to
2^-9, saturation at 448). The plane scales are constants, since the per-candidate and per-matrix scales
already put the value's bound (activations: a rigorous one; weights: the maximum) in [2^14, 2^15):
hi x 2^-7, mid x 2^4 (|mid| <= 2^3), lo x 2^16 (|lo| <= 2^-9), pack.Q8_PLANE_EXPONENTS. The E8M0 block
scales of the instruction undo these constants, so the products enter `cor` in its scaled domain.
Each MFMA is modelled as the exact sum of its products added to the fp32 accumulator with one rounding
(scripts/mfma_round_probe.hip measured the f16 instruction that way).

Everything around the two GEMMs (pose_encoder.0, the hoisted object/time rows, head layer 2) is computed in
float64 from the fp32 inputs and rounded to fp32 once, the same for all three forms, so that the table
isolates the GEMM arithmetic. The per-candidate activation scales are the kernel's (split_col_scales: the
bound chain from max|pose|, not the measured maximum), so the e4m3 planes see the headroom the kernel gives
them.

Statistic: per-row relative score error against float64, as tests/test_gpu_large.py
test_head_gemm_arith_vs_float64_r12800 (|s - ref| / max_row|ref|; mean, p99.9, max).

Gate: the hybrid's mean and p99.9 are <= the exact-fp32 emulation's at both steps, and its max < 1e-5.

Usage: python scripts/x3q_error_model.py [--feat FEATURES.npy] [--out profiles/r7/x3q_error_model.json]
--feat: a cached (256, 1024) float32 array of the encoder features (computed with oracle.encoder_forward
and written there when the file is missing; the CPU encoder takes minutes).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from genpose2_amd import arch, pack, sde, weights  # noqa: E402

F32, F64 = np.float32, np.float64
A_HI8, A_MID8, A_LO8 = pack.Q8_PLANE_EXPONENTS   # exponents of the constant e4m3 plane scales (both operands)


def r32(x):
    return x.astype(F32).astype(F64)


def f16(x):
    return x.astype(np.float16).astype(F64)


def planes3(x):
    """hi, mid, lo f16 planes of the (already scaled) fp32 values x, as float64."""
    h = f16(x)
    r = x - h
    m = f16(r)
    return h, m, f16(r - m)


def e4m3(x):
    """OCP e4m3fn, round to nearest even, subnormals (quantum 2^-9), saturating at +-448."""
    a = np.abs(x)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.maximum(e, -6.0)
    quantum = np.exp2(e - 3)
    q = np.rint(a / quantum) * quantum          # np.rint rounds half to even
    return np.sign(x) * np.minimum(q, 448.0)


def col_scales(x, hsc):
    """split_col_scales (gp_head.h) in fp32: log2 of s1 and s2 per candidate."""
    A0, B0, A2, B2 = (F32(v) for v in hsc[:4])
    m0 = np.abs(x).max(1).astype(F32)
    k = F32(1.0009765625)
    b1 = np.maximum((A0 * m0 + B0).astype(F32) * k, F32(1e-18)).astype(F32)
    b2 = np.maximum((A2 * b1 + B2).astype(F32) * k, F32(1e-18)).astype(F32)
    return 14 - np.floor(np.log2(b1.astype(F64))), 14 - np.floor(np.log2(b2.astype(F64)))


def gemm_fp32(a, w):
    """(R,K) x (N,K) -> (R,N): one fp32 FMA chain over k per output."""
    acc = np.zeros((a.shape[0], w.shape[0]), F64)
    a, w = a.astype(F64), w.astype(F64)
    for k in range(a.shape[1]):
        acc = r32(acc + a[:, k:k + 1] * w[None, :, k])
    return acc


def gemm_split(a, w, ea, ew, form, init=None, stats=None):
    """a (R,K) fp32 activations with per-row scale exponents ea, w (N,K) fp32 weights with exponent ew.
    Returns the fp32 result (as float64) with the scales undone; init (R,N) fp32 enters `acc` in the scaled
    domain first (head layer 1's hoisted rows)."""
    sa = np.exp2(ea)[:, None]
    sw = 2.0 ** ew
    ah, am, al = planes3(r32(a.astype(F64) * sa))
    wh, wm, wl = planes3(r32(w.astype(F64) * sw))
    R, K = a.shape
    acc = np.zeros((R, w.shape[0]), F64) if init is None else r32(init.astype(F64) * sa * sw)
    cor = np.zeros_like(acc)
    if form == "hybrid":
        ewh8, ewm8, ewl8 = A_HI8, A_MID8, A_LO8
        ah8, am8, al8 = e4m3(ah * 2.0 ** A_HI8), e4m3(am * 2.0 ** A_MID8), e4m3(al * 2.0 ** A_LO8)
        wh8, wm8, wl8 = e4m3(wh * 2.0 ** ewh8), e4m3(wm * 2.0 ** ewm8), e4m3(wl * 2.0 ** ewl8)
        if stats is not None:
            for name, p8 in (("a_hi8", ah8), ("a_mid8", am8), ("a_lo8", al8), ("w_hi8", wh8), ("w_mid8", wm8),
                             ("w_lo8", wl8)):
                nz = np.abs(p8[p8 != 0])
                stats[name] = {"max": float(nz.max()) if nz.size else 0.0,
                               "subnormal_fraction_of_nonzero": float((nz < 2.0 ** -6).mean()) if nz.size else 0.0,
                               "saturated": int((nz >= 448.0).sum())}
        u_hl, u_mm, u_lh = 2.0 ** -(ewh8 + A_LO8), 2.0 ** -(ewm8 + A_MID8), 2.0 ** -(ewl8 + A_HI8)   # E8M0 scales
    for k0 in range(0, K, 32):
        s = slice(k0, k0 + 32)
        if form == "f16x3":
            for x, y in ((ah, wl), (al, wh), (am, wm), (ah, wm), (am, wh)):
                cor = r32(cor + x[:, s] @ y[:, s].T)
        else:
            for x, y in ((ah, wm), (am, wh)):
                cor = r32(cor + x[:, s] @ y[:, s].T)
            k = (k0 % 128) // 32
            if k < 3:
                g = slice(k0 - 32 * k, k0 - 32 * k + 128)
                x8, y8, u = ((al8, wh8, u_hl), (am8, wm8, u_mm), (ah8, wl8, u_lh))[k]
                cor = r32(cor + (x8[:, g] @ y8[:, g].T) * u)
        acc = r32(acc + ah[:, s] @ wh[:, s].T)
    return r32(r32(acc + cor) / (sa * sw))


def features(path):
    if path and os.path.exists(path):
        return np.load(path)
    import large_noise
    from oracle import oracle
    pts = large_noise.inputs("pc_r12800_t500")[0]
    feat = oracle.encoder_forward(weights.synthetic_state_dict("score"), pts).astype(F32)
    if path:
        np.save(path, feat)
    return feat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feat", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "x3q_error_model.json"))
    args = ap.parse_args()
    import large_noise
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_large_steps_r12800.npz"))
    src = str(g["src"])
    _, _, B, K, T, _, _ = large_noise.CASES[src]
    sd = weights.synthetic_state_dict("score")
    p32 = weights.head_params(sd)
    p = {k: np.asarray(v).astype(F64) for k, v in p32.items()}
    H = arch.HEAD_HID
    w2 = np.asarray(p32["pe2_w"], F32)
    whp = np.asarray(p32["h1_pose"], F32).reshape(3 * H, arch.POSE_HID)
    ew2, ewh = pack.split_exponent(w2), pack.split_exponent(whp)
    hsc = pack.split_constants(p32, ew2, ewh)
    feat = features(args.feat).astype(F64)
    tab = sde.pc_step_table(T)
    out = {"case": src, "rows": B * K, "statistic": "per-row |score - float64| / max_row |float64|",
           "e4m3_plane_exponents_hi_mid_lo": [A_HI8, A_MID8, A_LO8], "steps": {}}
    ok = True
    for j in (int(s) for s in g["steps"]):
        x = g[f"x_{j}"]
        t = float(tab[j, 0])
        xp = t * p["gfp_w"] * 2.0 * np.pi
        tf = np.maximum(p["te_w"] @ np.concatenate([np.sin(xp), np.cos(xp)]) + p["te_b"], 0.0)
        rows = [feat @ p["h1_pts"][k].T + p["h1_t"][k] @ tf + p["h1_b"][k] for k in range(3)]
        init64 = np.repeat(np.concatenate(rows, 1), K, 0)                       # (R, 768)
        h64 = np.maximum(x.astype(F64) @ p["pe0_w"].T + p["pe0_b"], 0.0)
        sig = arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** t

        def tail(u):
            return np.concatenate([u[:, H * k:H * (k + 1)] @ p["h2_w"][k].T + p["h2_b"][k] for k in range(3)], 1) / (sig + 1e-7)

        pf64 = np.maximum(h64 @ p["pe2_w"].T + p["pe2_b"], 0.0)
        ref = tail(np.maximum(init64 + pf64 @ whp.astype(F64).T, 0.0))
        scale = np.abs(ref).max(1, keepdims=True)
        h32, init32 = h64.astype(F32), init64.astype(F32)
        e1, e2 = col_scales(x, hsc)
        b2 = p["pe2_b"]
        res, planes = {}, {}
        for form in ("f16x3", "hybrid", "fp32"):
            if form == "fp32":
                pf = np.maximum(r32(gemm_fp32(h32, w2) + b2), 0.0).astype(F32)
                u = np.maximum(r32(init32.astype(F64) + gemm_fp32(pf, whp)), 0.0)
            else:
                st2, sth = ({}, {}) if form == "hybrid" else (None, None)
                pf = np.maximum(r32(gemm_split(h32, w2, e1, ew2, form, stats=st2) + b2), 0.0).astype(F32)
                u = np.maximum(gemm_split(pf, whp, e2, ewh, form, init=init32, stats=sth), 0.0)
                if form == "hybrid":
                    planes = {"pose_encoder.2": st2, "head_layer_1": sth}
            e = np.abs(r32(tail(u)) - ref) / scale
            res[form] = {"mean": float(e.mean()), "p999": float(np.percentile(e, 99.9)), "max": float(e.max())}
            print(f"step {j} {form:6s} mean {res[form]['mean']:.3e} p99.9 {res[form]['p999']:.3e} "
                  f"max {res[form]['max']:.3e}", flush=True)
        passed = (res["hybrid"]["mean"] <= res["fp32"]["mean"] and res["hybrid"]["p999"] <= res["fp32"]["p999"]
                  and res["hybrid"]["max"] < 1e-5)
        ok = ok and passed
        out["steps"][str(j)] = {"t": t, "errors": res, "e4m3_planes": planes, "gate": bool(passed)}
    out["gate"] = "hybrid mean and p99.9 <= exact fp32's, hybrid max < 1e-5"
    out["gate_passed"] = bool(ok)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("gate", "PASSED" if ok else "FAILED", "->", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
