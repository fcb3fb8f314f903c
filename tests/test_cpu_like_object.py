"""CPU checks of the object-coupled likelihood (cfg.like_coupling = "object", gp_like_sample_object): the config
field, the C ABI's new names, the fixture's seeded inputs, the workspace sizes, and the entry's argument checks, which
return before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden

NEW = ("gp_like_sample_object", "gp_like_object_workspace_size", "gp_like_object_workspace_size_k",
       "gp_debug_like_obj_attempt")


def test_config_field():
    from genpose2_amd.config import GenPoseConfig
    assert GenPoseConfig().like_coupling == "batch"
    GenPoseConfig(like_coupling="object").validate()
    GenPoseConfig(like_coupling="object", sampler_mode=["ode"], ode_coupling="batch").validate()
    GenPoseConfig(like_coupling="batch", sampler_mode=["ode"], ode_coupling="object").validate()
    with pytest.raises(ValueError, match="like_coupling"):
        GenPoseConfig(like_coupling="row").validate()
    with pytest.raises(ValueError, match="like_coupling"):
        GenPoseConfig(like_coupling="").validate()


def test_runner_does_not_read_the_field():
    """The likelihood is not a runner stage: runner.object_coupled names the sampler's field only."""
    from genpose2_amd.config import GenPoseConfig
    from genpose2_amd.runner import object_coupled
    assert object_coupled(GenPoseConfig(like_coupling="object")) is None
    assert object_coupled(GenPoseConfig(like_coupling="object", sampler_mode=["ode"])) is None


def test_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert set(NEW) <= set(_lib.exported_symbols())
    assert re.search(r"#define GP_ABI_VERSION 7\b", header)
    assert _lib.load().gp_abi_version() == 7                  # additive: the ABI version stays


def test_workspace_sizes():
    from genpose2_amd import _lib
    lib = _lib.load()
    for rows, k in ((21, 7), (3, 1), (140, 70), (12800, 50)):
        # y, y_new, K_0..K_6, f1 of 10 rows doubles | six 768-rows fp32 per object
        need = 8 * 10 * 10 * rows + 4 * 6 * 768 * (rows // k)
        assert need <= lib.gp_like_object_workspace_size_k(rows, k) <= lib.gp_like_object_workspace_size(rows), (rows, k)
        assert lib.gp_like_object_workspace_size(rows) == lib.gp_like_object_workspace_size_k(rows, 1)
    for rows, k in ((20, 7), (21, 0), (0, 7), (-7, 7), (21, -1)):   # not whole objects
        assert lib.gp_like_object_workspace_size_k(rows, k) == 0, (rows, k)
    assert lib.gp_like_object_workspace_size(0) == 0


def test_fixture_inputs_regenerate_from_their_seeds():
    import like_object_inputs as lo
    from genpose2_amd import synthetic
    g = golden("like_object")
    B, K = lo.B, lo.K
    pts, _ = synthetic.make_batch(lo.CONFIG_ID, B, lo.N_POINTS)
    pts = lo.scale_clouds(pts)
    assert pts.dtype == g["pts"].dtype and pts.tobytes() == g["pts"].tobytes()
    inp = lo.pose_inputs(g["pts_center"])
    for k, v in inp.items():
        assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), k
    assert g["pose_samples"].shape == (B, K, 9) and g["eps_unit"].shape == (B * K, 9)
    assert g["pts_feat"].shape == (B, 1024) and g["pts_center"].shape == (B, 3)
    for tag in ("ll32", "ll32_p1", "ll32_p2", "ll64"):
        assert g[tag].shape == (B, K) and g[tag].dtype == np.float64, tag
        assert g["nfev_" + tag].shape == (B,) and g["status_" + tag].tolist() == [0] * B, tag
        assert g["nfev_" + tag].max() <= 30000 and np.all((g["nfev_" + tag] - 2) % 6 == 0), tag
    assert g["z64"].shape == (B, K, 9) and g["ll32_batch"].shape == (B, K)
    assert len(set(g["nfev_ll32"].tolist())) == B             # the scaled clouds give solves of different lengths


def test_bad_arguments_return_before_any_device_work():
    """Every bad-argument case returns non-zero with its word in gp_last_error(). No device is present here, and the
    pointers are not addresses of anything: a call that went on to launch would fail otherwise or fault."""
    from genpose2_amd import _lib
    lib = _lib.load()
    w = _lib.HeadWeights()
    R, K = 21, 7
    need = int(lib.gp_like_object_workspace_size_k(R, K))
    nfev, status = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    P = ctypes.c_void_p(0x1000)

    def raw(rows=R, k=K, rows_total=R, t0=1e-5, t1=1.0, bytes_=need, **null):
        ptr = {n: (None if null.get(n) else P) for n in ("pobj", "x", "eps", "z", "ll", "ws")}
        return lib.gp_like_sample_object(None if null.get("w") else ctypes.byref(w), ptr["pobj"], ptr["x"], ptr["eps"],
                                         rows, k, rows_total, t0, t1, 1e-5, 1e-5, ptr["z"], ptr["ll"],
                                         None if null.get("nfev") else nfev, None if null.get("status") else status,
                                         ptr["ws"], bytes_, None)

    cases = [(dict(rows=R - 1), "whole objects"), (dict(rows=0), "bad arguments"), (dict(k=0), "bad arguments"),
             (dict(rows_total=R - K), "rows_total"), (dict(rows_total=R + 1), "rows_total"),
             (dict(t0=1.0, t1=1.0), "empty integration interval"), (dict(bytes_=need - 1), "workspace too small"),
             (dict(bytes_=0), "workspace too small")]
    cases += [({n: True}, "null pointer") for n in ("w", "pobj", "x", "eps", "z", "ll", "nfev", "status", "ws")]
    for kw, word in cases:
        assert raw(**kw) != 0, kw
        assert word in lib.gp_last_error().decode(), (kw, lib.gp_last_error())
        with pytest.raises(_lib.GenPoseHipError, match=word):
            _lib.check(raw(**kw), "like_sample_object")
    assert list(nfev) == [0, 0, 0] and list(status) == [0, 0, 0]

    # the test aid checks its arguments the same way
    ks = (ctypes.c_void_p * 7)(*([0x1000] * 7))
    dbg = lambda rows, k, total, kslots=ks, rec=P: lib.gp_debug_like_obj_attempt(  # noqa: E731
        ctypes.byref(w), P, rec, P, P, P, kslots, P, P, rows, k, total, 1e-5, 1e-5, None)
    assert dbg(R - 1, K, R) != 0 and "whole objects" in lib.gp_last_error().decode()
    assert dbg(R, K, R - K) != 0 and "whole objects" in lib.gp_last_error().decode()
    assert dbg(R, K, R, rec=None) != 0 and "null pointer" in lib.gp_last_error().decode()
    ks[3] = None
    assert dbg(R, K, R) != 0 and "null K slot" in lib.gp_last_error().decode()
