"""CPU checks of per-object PC sampling (cfg.pc_coupling = "object", gp_pc_sample_object): the C ABI's new names,
the config field, the fixture's seeded inputs, and the oracle's PC sampler called once per object against the
reference's own per-object runs (tests/golden/make_golden_pc_object.py)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
from oracle import oracle

NEW = ("gp_pc_sample_object", "gp_pc_object_workspace_size")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_pc_object_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7                       # additive: the ABI version stays
    # s (R,9) | row norms (2,R) | draws (2,2,R,9), fp32
    assert lib.gp_pc_object_workspace_size(30) >= 4 * (30 * 9 * 5 + 2 * 30)


def test_config_field():
    from genpose2_amd.config import GenPoseConfig
    assert GenPoseConfig().pc_coupling == "batch"
    GenPoseConfig(pc_coupling="object").validate()
    GenPoseConfig(pc_coupling="batch").validate()
    with pytest.raises(ValueError, match="pc_coupling"):
        GenPoseConfig(pc_coupling="row").validate()


def test_fixture_inputs_regenerate_from_their_seeds():
    import pc_object_inputs as pi
    g = golden("pc_object")
    inp = pi.inputs()
    assert inp["prior"].shape == (pi.B * pi.K, 9) and inp["z1"].shape == (pi.T, pi.B * pi.K, 9)
    for k, v in inp.items():
        assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), k
    R = pi.B * pi.K
    assert g["pred_pose32"].shape == (R, 9) and g["pred_q32"].shape == (R, 7) and g["xs32"].shape == (R, pi.T, 9)
    assert g["pred_pose32"].dtype == np.float32 and g["pred_pose64"].dtype == np.float64
    assert g["pred_pose32_batch"].shape == (R, 9)


def _oracle_per_object(sd, g):
    """oracle.pc_sample once per object, on that object's rows of the prior and of z1 / z2 -> (res, q, xs) rows."""
    import pc_object_inputs as pi
    from genpose2_amd import arch
    K, T = pi.K, pi.T
    sig = np.float32(arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** 1.0)
    res, xs = [], []
    for b in range(pi.B):
        rows = slice(b * K, (b + 1) * K)
        feat_rows = np.repeat(g["pts_feat"][b:b + 1], K, 0)
        x0 = (g["prior"][rows] * sig).astype(np.float32)
        x, r = oracle.pc_sample(lambda x, t: oracle.score_forward(sd, feat_rows, x, t), x0,
                                np.repeat(g["pts_center"][b:b + 1], K, 0), T, g["z1"][:, rows], g["z2"][:, rows])
        res.append(r), xs.append(x)
    res = np.concatenate(res, 0)
    return res, oracle.pose_to_quat_rows(res), np.concatenate(xs, 0)


def test_oracle_per_object_vs_reference(score_sd):
    """The small-golden PC tolerances of test_oracle_golden.py: rotation <= 1e-4 absolute, translation <= 1e-5 of
    max |t|."""
    g = golden("pc_object")
    res, q, xs = _oracle_per_object(score_sd, g)
    assert np.abs(res[:, :6] - g["pred_pose32"][:, :6]).max() < 1e-4
    assert rel(res[:, 6:], g["pred_pose32"][:, 6:]) < 1e-5
    assert np.abs(q[:, :4] - g["pred_q32"][:, :4]).max() < 1e-4
    assert np.abs(xs[..., :6] - g["xs32"][..., :6]).max() < 1e-4
    assert rel(xs[..., 6:], g["xs32"][..., 6:]) < 1e-5


def test_fixture_tells_the_two_semantics_apart():
    """The reference's one call on all 30 rows (grad_norm over the batch) is outside those tolerances of its
    per-object calls on at least one object -- here on every object."""
    import pc_object_inputs as pi
    g = golden("pc_object")
    a, b = g["pred_pose32_batch"].reshape(pi.B, pi.K, 9), g["pred_pose32"].reshape(pi.B, pi.K, 9)
    tsc = np.abs(b[..., 6:]).max()
    apart = [np.abs(a[o, :, :6] - b[o, :, :6]).max() > 1e-4 or np.abs(a[o, :, 6:] - b[o, :, 6:]).max() / tsc > 1e-5
             for o in range(pi.B)]
    assert any(apart)
    assert all(apart)
