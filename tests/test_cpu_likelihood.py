"""CPU checks of the likelihood mode (cond_ode_likelihood, samplers.py:25-110): the C ABI's new names, the
forward-mode divergence against the reference's autograd result, the controller over the augmented state, and
the fixtures' seeded inputs."""
import os
import re

import numpy as np

from conftest import GOLDEN, REPO, golden

NEW = ("gp_score_div_eval", "gp_like_rhs", "gp_like_attempt", "gp_like_workspace_size")


def test_likelihood_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7                       # additive: the ABI version stays
    assert lib.gp_like_workspace_size(50) >= 6 * 768 * 4 + 8 * 4


def test_forward_mode_divergence_equals_reference_autograd(score_sd):
    """eps . (J eps) pushed forward through the trunk with the primal's ReLU masks (like_ref.score_div64) is the
    reference's reverse-mode eps . grad_x(sum(score * eps)) in float64: 1e-10 of max |div64| per time, and the
    same score and kink margins."""
    import like_ref
    g = golden("like_eval")
    feat_rows = np.repeat(g["pts_feat"], g["pose"].shape[0] // g["pts_feat"].shape[0], 0)
    for j, t in enumerate(g["t"]):
        s, d, m = like_ref.score_div64(score_sd, feat_rows, g["pose"], t, g["eps"])
        es = np.abs(s - g["score64"][j]).max() / np.abs(g["score64"][j]).max()
        ed = np.abs(d - g["div64"][j]).max() / np.abs(g["div64"][j]).max()
        print(f"t={t:g}: forward-mode vs autograd float64: score {es:.2e}, div {ed:.2e}")
        assert es <= 1e-10 and ed <= 1e-10, (t, es, ed)
        np.testing.assert_allclose(m, g["margin"][j], rtol=1e-6, atol=1e-12)


def test_fixture_kink_exclusions_within_cap():
    import like_inputs as li
    g = golden("like_eval")
    excl = g["margin"] < li.KINK_MARGIN
    print("rows under the kink margin:", int(excl.sum()), "of", excl.size)
    assert excl.size == 200 and excl.sum() <= li.MAX_EXCLUDED * excl.size


def test_rk45_drive_augmented_state_equals_solve_ivp():
    """The controller over an augmented [x | logp] state whose logp derivative is a divergence-like function of
    x (and no function of logp), one RMS norm over all entries: t, y and nfev of scipy's solve_ivp exactly."""
    from scipy.integrate import solve_ivp
    from genpose2_amd import ode
    R = 7
    rng = np.random.default_rng(3)
    Wm = rng.standard_normal((9, 9)) / 3.0
    e = rng.standard_normal((R, 9))
    y0 = np.concatenate([rng.standard_normal(R * 9), np.zeros(R)])

    def fun(t, y):
        x = y[:-R].reshape(R, 9)
        g2 = 0.5 * (0.01 * 5000.0 ** t * 4.1) ** 2
        s = np.tanh(x @ Wm.T) / (0.01 * 5000.0 ** t)
        js = ((1.0 - np.tanh(x @ Wm.T) ** 2) * (e @ Wm.T)) / (0.01 * 5000.0 ** t)
        return np.concatenate([(-g2 * s).reshape(-1), -g2 * (e * js).sum(1)])

    res = solve_ivp(fun, (1e-5, 1.0), y0, method="RK45", rtol=1e-5, atol=1e-5)
    be = ode.NumpyRk45(fun, y0, 1e-5, 1e-5)
    ts, nfev, status = ode.rk45_drive(be, 1e-5, 1.0, 1e-5, 1e-5)
    assert status == res.status == 0 and nfev == res.nfev
    assert np.array_equal(ts, res.t)
    assert np.array_equal(np.stack(be.ys, 1), res.y)


def test_fixture_inputs_regenerate_from_their_seeds():
    import like_inputs as li
    g = golden("like_eval")
    inp = li.eval_inputs()
    for k, v in inp.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    o = golden("like_ode")
    inp = li.ode_inputs(o["pts_center"])
    for k, v in inp.items():
        assert o[k].dtype == v.dtype and np.array_equal(o[k], v), k
    from genpose2_amd import synthetic
    pts, center = synthetic.make_batch(21, li.ODE_B, 1024)
    assert np.array_equal(o["pts"], pts)
    assert os.path.exists(os.path.join(GOLDEN, "make_golden_likelihood.py"))
