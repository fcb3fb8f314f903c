"""CPU checks of per-object ODE sampling (cfg.ode_coupling = "object", gp_ode_sample_object): the C ABI's new names,
the config field, the fixture's seeded inputs, and the oracle's ODE sampler called once per object against the
reference's own per-object runs (tests/golden/make_golden_ode_object.py)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
from oracle import oracle

NEW = ("gp_ode_sample_object", "gp_ode_object_workspace_size", "gp_ode_object_workspace_size_k")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_ode_object_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7                       # additive: the ABI version stays
    # y, y_new, K_0..K_6, f1, the output (R,9) fp64 | six 768-rows fp32 per object
    rows, k = 30, 10
    need = 8 * 11 * rows * 9 + 4 * 6 * 768 * (rows // k)
    assert need <= lib.gp_ode_object_workspace_size_k(rows, k) <= lib.gp_ode_object_workspace_size(rows)
    assert lib.gp_ode_object_workspace_size(rows) == lib.gp_ode_object_workspace_size_k(rows, 1)
    assert lib.gp_ode_object_workspace_size_k(rows, 7) == 0      # not whole objects


def test_config_field():
    from genpose2_amd.config import GenPoseConfig
    assert GenPoseConfig().ode_coupling == "batch"
    GenPoseConfig(ode_coupling="object", sampler_mode=["ode"]).validate()
    GenPoseConfig(ode_coupling="object").validate()        # read only by the ODE sampler
    GenPoseConfig(ode_coupling="batch").validate()
    with pytest.raises(ValueError, match="ode_coupling"):
        GenPoseConfig(ode_coupling="row").validate()


def test_runner_names_the_coupled_field():
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.runner import object_coupled
    assert object_coupled(GenPoseConfig()) is None
    assert object_coupled(GenPoseConfig(ode_coupling="object")) is None                 # the PC sampler runs
    assert object_coupled(GenPoseConfig(ode_coupling="object", sampler_mode=["ode"])) == "ode_coupling"
    assert object_coupled(GenPoseConfig(pc_coupling="object")) == "pc_coupling"
    assert object_coupled(GenPoseConfig(pc_coupling="object", sampler_mode=["ode"])) is None


def test_fixture_inputs_regenerate_from_their_seeds():
    import ode_object_inputs as oi
    g = golden("ode_object")
    inp = oi.inputs()
    assert inp["prior"].shape == (oi.B * oi.K, 9) and inp["pts_feat"].shape == (oi.B, 1024)
    for k, v in inp.items():
        assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), k
    R = oi.B * oi.K
    assert g["pred_pose32"].shape == (R, 9) and g["pred_q32"].shape == (R, 7)
    assert g["pred_pose32"].dtype == np.float64 and g["pred_pose64"].dtype == np.float64   # the ODE path's dtype
    assert g["pred_pose_batch"].shape == (R, 9)
    assert g["nfev32"].shape == (oi.B,) and g["nfev64"].shape == (oi.B,)
    assert np.array_equal(g["nfev32"], g["nfev64"])       # the generator's first condition


def test_oracle_per_object_vs_reference(score_sd):
    """oracle.ode_sample once per object, on that object's prior rows, against the reference's per-object calls:
    the bars of test_oracle_golden.py (rotation < 1e-4 absolute, translation < 1e-5 of max |t|) and equal nfev."""
    import ode_object_inputs as oi
    from genpose2_amd import arch
    g = golden("ode_object")
    K = oi.K
    sig = np.float32(arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** oi.T0)
    res, nfev = [], []
    for b in range(oi.B):
        rows = slice(b * K, (b + 1) * K)
        feat_rows = np.repeat(g["pts_feat"][b:b + 1], K, 0)
        x0 = (g["prior"][rows] * sig).astype(np.float32)
        _, x, n = oracle.ode_sample(lambda x, t: oracle.score_forward(score_sd, feat_rows, x, t), x0,
                                    np.repeat(g["pts_center"][b:b + 1], K, 0), oi.T0, oi.STEPS)
        res.append(x), nfev.append(n)
    res = np.concatenate(res, 0)
    assert res.dtype == np.float64
    assert nfev == g["nfev32"].tolist()
    assert np.abs(res[:, :6] - g["pred_pose32"][:, :6]).max() < 1e-4
    assert rel(res[:, 6:], g["pred_pose32"][:, 6:]) < 1e-5
    q = oracle.pose_to_quat_rows(res)
    assert np.abs(q[:, :4] - g["pred_q32"][:, :4]).max() < 1e-4


def test_fixture_tells_the_two_semantics_apart():
    """The reference's one call on all 30 rows (one solve_ivp, error norms over the batch) is outside those
    tolerances of its per-object calls on every object, and takes another number of evaluations than at least one
    object's own solve."""
    import ode_object_inputs as oi
    g = golden("ode_object")
    a, b = g["pred_pose_batch"].reshape(oi.B, oi.K, 9), g["pred_pose32"].reshape(oi.B, oi.K, 9)
    tsc = np.abs(b[..., 6:]).max()
    apart = [np.abs(a[o, :, :6] - b[o, :, :6]).max() > 1e-4 or np.abs(a[o, :, 6:] - b[o, :, 6:]).max() / tsc > 1e-5
             for o in range(oi.B)]
    assert all(apart)
    assert np.any(g["nfev32"] != int(g["nfev_batch"]))
