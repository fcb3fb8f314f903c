"""CPU checks of the energy agent on the ODE sampler (GenPoseConfig.energy_ode, the gp_ode_*_energy entries): the C
ABI's new names, the config field, the fixture's own conditions (tests/golden/make_golden_energy_ode.py) and the
float64 restatement of the energy's score stepped through the reference's float64 solve."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden

NEW = ("gp_ode_rhs_energy", "gp_ode_attempt_energy", "gp_ode_auto_attempt_energy", "gp_ode_denoise_energy",
       "gp_ode_sample_energy")


def test_energy_ode_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        m = re.search(r"\b%s\(([^;]*)\);" % n, header)
        assert m, n
        assert "const gp_head_grad_weights *gw" in m.group(1), n
        assert n in _lib.EXPORTED, n
        # the namesake's arguments plus gw: one more argument in the binding
        base = n[:-len("_energy")] + ("_hs" if n == "gp_ode_auto_attempt_energy" else "")
        assert len(_lib._SIGS[n][1]) == len(_lib._SIGS[base][1]) + 1, n
    assert set(NEW) <= set(_lib.exported_symbols())
    assert _lib.load().gp_abi_version() == 7                       # additive: the ABI version stays
    assert re.search(r"#define GP_ABI_VERSION 7\b", header)


def test_config_field():
    from genpose2_amd.config import GenPoseConfig
    assert GenPoseConfig().energy_ode is False
    GenPoseConfig(energy_ode=True, agent_type="energy", sampler_mode=["ode"]).validate()
    GenPoseConfig(energy_ode=False, agent_type="energy", sampler_mode=["ode"]).validate()
    GenPoseConfig(energy_ode=True).validate()                      # read only by the energy agent's ODE sampler
    with pytest.raises(ValueError, match="energy_ode"):
        GenPoseConfig(energy_ode="yes").validate()


def test_fixture_inputs_and_conditions():
    """The inputs regenerate from their seed bit for bit, and the generator's conditions hold on what it wrote."""
    import energy_ode_inputs as ei
    g = golden("energy_ode")
    R = ei.B * ei.K
    assert int(g["seed"]) == ei.SEED
    for k, v in ei.inputs().items():
        assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), k
    assert g["pred_pose32"].shape == (R, 9) and g["pred_q32"].shape == (R, 7) and g["pred_pose64"].shape == (R, 9)
    assert g["pred_pose32"].dtype == np.float64 and g["y64"].shape == (R * 9,) and g["y32_forced"].shape == (R * 9,)
    tr = g["trace64"]
    assert tr.ndim == 2 and tr.shape[1] == 3 and g["norm32_forced"].shape == (len(tr),)
    assert int(g["nfev32"]) == int(g["nfev64"]) == 2 + 6 * len(tr)
    assert np.abs(tr[:, 2] - 1).min() >= ei.NEAR_ONE
    assert np.array_equal(g["norm32_forced"] < 1, tr[:, 2] < 1)
    assert np.abs(g["norm64_forced"] / tr[:, 2] - 1).max() <= 1e-12
    # the accepted steps lead from T0 to eps
    acc = tr[tr[:, 2] < 1]
    assert acc[0, 0] == ei.T0 and np.allclose(acc[:-1, 0] + acc[:-1, 1], acc[1:, 0], rtol=0, atol=1e-15)
    assert abs(acc[-1, 0] + acc[-1, 1] - 1e-5) < 1e-15
    rot, trans = ei.row_errors(g["pred_pose32"], g["pred_pose64"])
    assert np.median(rot) >= ei.MIN_MEDIAN_ROW                     # the typical regime, not a lucky seed
    assert rot.max() <= float(g["spread_rot"]) and trans.max() <= float(g["spread_trans"])
    assert int(g["nfev_lo"]) <= int(g["nfev32"]) <= int(g["nfev_hi"])


def test_float64_restatement_reproduces_the_forced_norms(energy_sd):
    """genpose2_amd.ode.NumpyRk45 over tests/energy_ref.energy_score64 (right-hand side -(g^2 / 2) score at
    float32(y), the scalars of ode.time_scalars) stepped through trace64's (t, h), accepting where norm64 < 1,
    reproduces the reference's float64 error norms. Measured here: the largest |norm / norm64 - 1| over the 29
    attempts is 6.44e-15 (autograd's float64 summation order against the reference's own); the bar is 10x that.
    This holds the restatement, the scalars and NumpyRk45's stage arithmetic to the reference along the whole
    solve; the GPU tests use the same pieces around the device's score."""
    import energy_ode_inputs as ei
    import energy_ref
    from genpose2_amd import arch, ode
    g = golden("energy_ode")
    R = ei.B * ei.K
    feat = np.repeat(g["pts_feat"], ei.K, 0)

    def fun(t, y):
        t32, _, coef = ode.time_scalars(t)
        x = y.reshape(R, 9).astype(np.float32).astype(np.float64)
        s, _, _ = energy_ref.energy_score64(energy_sd, feat, x, t32)
        return coef * s.reshape(-1)

    sig = np.float32(arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** ei.T0)
    be = ode.NumpyRk45(fun, (g["prior"] * sig).astype(np.float32).reshape(-1))
    be.rhs0(ei.T0)
    rel = []
    for t, h, n64 in g["trace64"]:
        t, h = np.float64(t), np.float64(h)
        rel.append(abs(float(be.attempt(t, h)) / n64 - 1))
        if n64 < 1:
            be.accept(t, t + h)
    print(f"float64 restatement through trace64: |norm / norm64 - 1| max {max(rel):.2e}")
    assert max(rel) <= 6.5e-14, max(rel)
    print(f"final state vs y64 (the last step's dense output at eps): {np.abs(be.y - g['y64']).max():.2e}")
