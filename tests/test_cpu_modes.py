"""CPU-only tests of the pose hypotheses: the C entry's declaration, export and argument checks (none launches),
the NumPy restatement (tests/modes_ref.py) against the reference-made fixture (golden_modes.npz), and the
follow-previous selection and the per-frame split on hand-made PoseModes tensors. No HIP compute calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden

import modes_inputs as mi
import modes_ref

NEW = "gp_rank_aggregate_modes"


@pytest.fixture(autouse=True)
def _the_entry_exists():
    """Everything here describes the entry: without it in the binding no test of this file passes."""
    from genpose2_amd import _lib
    assert NEW in _lib.EXPORTED


def test_entry_is_declared_and_exported():
    from genpose2_amd import _lib
    hdr = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    assert NEW in set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert NEW in _lib.EXPORTED and NEW in set(_lib.exported_symbols())
    assert _lib.load().gp_abi_version() == 7
    assert re.search(r"#define GP_ABI_VERSION 7\b", hdr)


def test_argument_checks_return_a_status_without_a_device():
    from genpose2_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    outs = ("mode_pose", "mode_count", "mode_energy", "mode_spread", "n_clusters", "noise_count", "nearest")

    def call(poses=p, energy=p, b=1, k=50, retain=20, clustering=1, min_samples=3, max_modes=4, prev_rot=None,
             aggregated=p, **kw):
        o = [kw.get(n, p) for n in outs]
        return lib.gp_rank_aggregate_modes(poses, energy, b, k, retain, clustering, 0.05, min_samples, max_modes,
                                           prev_rot, aggregated, None, None, *o, None)

    def err():
        return lib.gp_last_error()

    for m in (0, -1, 9):
        assert call(max_modes=m) == -1 and b"max_modes" in err(), m
    for name in outs:
        assert call(**{name: None}) == -1 and b"null mode output" in err(), name
    for name in ("poses", "energy", "aggregated"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    assert call(k=0) == -1 and b"k=0" in err()
    assert call(k=1025, retain=20) == -1 and b"k=1025" in err()
    assert call(retain=0) == -1 and b"retain" in err()
    assert call(k=10, retain=11) == -1 and b"retain" in err()
    assert call(k=300, retain=129) == -1 and b"retain" in err()
    assert call(min_samples=0) == -1 and b"min_samples" in err()
    assert call(b=-1) == -1
    # b == 0: GP_OK and nothing launched, whatever the pointers hold
    assert call(b=0, poses=None, energy=None, aggregated=None, **{n: None for n in outs}) == 0
    assert call(b=0, max_modes=9) == -1 and b"max_modes" in err()


def test_python_argument_checks_need_no_device():
    from genpose2_amd import aggregate
    from genpose2_amd.infer import GenPose2
    pose, energy = torch.zeros(2, 10, 9), torch.zeros(2, 10, 2)
    with pytest.raises(ValueError, match="keeps no candidate"):
        aggregate.aggregate_modes(pose, energy, retain_ratio=0.0)
    with pytest.raises(ValueError, match="exceeds"):
        aggregate.aggregate_modes(pose, energy, retain_num=11)
    with pytest.raises(ValueError, match="HIP device"):
        aggregate.aggregate_modes(pose, energy)
    for m in (0, 9):   # before the front end or any agent is touched
        with pytest.raises(ValueError, match="max_modes"):
            GenPose2.inference_modes(None, {}, max_modes=m)
        with pytest.raises(ValueError, match="max_modes"):
            GenPose2.inference_frames_modes(None, {}, max_modes=m)


@pytest.fixture(scope="module")
def ref_on_golden():
    g = golden("modes")
    out = {p: modes_ref.modes_ref(g["pred_pose"], g["pred_energy"], mi.KEEP, 1, mi.EPS, mi.MIN_SAMPLES, mi.MAX_SLOTS,
                                  g["prev_rot"][p]) for p in (0, 1)}
    return g, out


def test_fixture_is_what_its_inputs_module_builds():
    g = golden("modes")
    pose, energy, _ = mi.build_inputs(g["seeds"], g["noise_deg"])
    np.testing.assert_array_equal(pose, g["pred_pose"])
    np.testing.assert_array_equal(energy, g["pred_energy"])
    assert g["pred_pose"].shape == (mi.B, mi.K, 9)
    nc = g["n_clusters"]
    assert (nc > 4).any() and (nc == 0).any()
    assert any(nc[j] >= 2 and g["mode_count"][j, 0] == g["mode_count"][j, 1] for j in range(mi.B))
    for j, (sizes, outliers, _) in enumerate(mi.OBJECTS):   # the designed cluster sizes, largest first
        want = sorted((s for s in sizes if s >= mi.MIN_SAMPLES), reverse=True) or [mi.KEEP]
        assert g["mode_count"][j][g["mode_count"][j] > 0].tolist() == want, j


def test_restatement_reproduces_the_reference_fixture(ref_on_golden):
    g, out = ref_on_golden
    r = out[0]
    assert r["margin"].min() > 1e-3
    for name in ("labels", "slot_label", "mode_count", "n_clusters", "noise_count"):
        np.testing.assert_array_equal(r[name], g[name], err_msg=name)
    filled = np.maximum(1, np.minimum(g["n_clusters"], mi.MAX_SLOTS))
    for j in range(mi.B):
        assert np.abs(r["mode_pose"][j, :, :3, :3] - g["mode_rot"][j]).max() < 1e-5, j
        assert not r["mode_pose"][j, filled[j]:].any() and not g["mode_rot"][j, filled[j]:].any()
    assert np.abs(r["aggregated"] - g["aggregated"]).max() < 1e-5
    np.testing.assert_array_equal(r["mode_pose"][:, 0, :3, :3], r["aggregated"][:, :3, :3])
    tol_mean = max(1e-6, 2 * float(g["mean_gap"]))
    tol_spread = max(1e-6, 2 * float(g["spread_gap"]))
    assert np.abs(r["mode_pose"][:, :, :3, 3] - g["mode_trans_f32"]).max() <= tol_mean
    assert np.abs(r["mode_energy"] - g["mode_energy_f32"]).max() <= tol_mean
    assert np.abs(r["mode_spread"] - g["mode_spread_f32"]).max() <= tol_spread


def test_restatement_nearest_and_cap(ref_on_golden):
    g, _ = ref_on_golden
    for p in (0, 1):   # nearest is recorded for max_modes = 4
        r = modes_ref.modes_ref(g["pred_pose"], g["pred_energy"], mi.KEEP, 1, mi.EPS, mi.MIN_SAMPLES, 4,
                                g["prev_rot"][p])
        np.testing.assert_array_equal(r["nearest"], g["nearest"][p])
        np.testing.assert_array_equal(r["n_clusters"], g["n_clusters"])      # not capped by M
        np.testing.assert_array_equal(r["mode_count"], g["mode_count"][:, :4])
    assert set(g["nearest"][1].tolist()) == {0, 1}
    r = modes_ref.modes_ref(g["pred_pose"], g["pred_energy"], mi.KEEP, 0, mi.EPS, mi.MIN_SAMPLES, 4)
    assert not r["n_clusters"].any() and not r["noise_count"].any() and (r["nearest"] == -1).all()
    assert (r["mode_count"][:, 0] == mi.KEEP).all() and not r["mode_count"][:, 1:].any()


def _hand_made_modes(B=5, M=3):
    from genpose2_amd.aggregate import PoseModes
    g = torch.Generator().manual_seed(3)
    return PoseModes(aggregated=torch.randn(B, 4, 4, generator=g), mode_pose=torch.randn(B, M, 4, 4, generator=g),
                     mode_count=torch.arange(B * M, dtype=torch.int32).view(B, M),
                     mode_energy=torch.randn(B, M, generator=g), mode_spread=torch.rand(B, M, generator=g),
                     n_clusters=torch.arange(B, dtype=torch.int32), noise_count=torch.arange(B, dtype=torch.int32) + 7,
                     nearest=torch.tensor([2, 0, -1, 1, 0], dtype=torch.int32))


def test_follow_takes_the_nearest_slots_rotation_only():
    modes = _hand_made_modes()
    pose = modes.aggregated
    before = pose.clone()
    out = modes.follow(pose)
    assert torch.equal(pose, before) and out.data_ptr() != pose.data_ptr()      # the input is left alone
    for j, n in enumerate(modes.nearest.tolist()):
        want = modes.mode_pose[j, n, :3, :3] if n >= 0 else pose[j, :3, :3]      # -1: no previous rotation
        assert torch.equal(out[j, :3, :3], want), j
        assert torch.equal(out[j, :, 3], pose[j, :, 3]) and torch.equal(out[j, 3], pose[j, 3]), j


def test_split_by_frame_offsets():
    from dataclasses import fields
    modes = _hand_made_modes()
    parts = modes.split([0, 2, 2, 5])            # the middle frame holds no object
    assert [int(p.nearest.shape[0]) for p in parts] == [2, 0, 3]
    for f in fields(modes):
        whole = getattr(modes, f.name)
        assert torch.equal(torch.cat([getattr(p, f.name) for p in parts]), whole), f.name
        assert getattr(parts[1], f.name).shape[1:] == whole.shape[1:]
    assert torch.equal(parts[2].mode_pose, modes.mode_pose[2:5])
