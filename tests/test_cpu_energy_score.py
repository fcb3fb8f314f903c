"""CPU checks of the energy model as a score model (PoseEnergyNet.forward(return_item='score'), energynet.py:211-233):
the C ABI's new names, the transposed weight packing of the reverse pass, the float64 restatement against the
reference's own float64 run, and the fixtures' seeded inputs and exclusion caps."""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import GOLDEN, REPO, golden

NEW = ("gp_head_grad_floats", "gp_head_grad_pack", "gp_energy_score_eval", "gp_pc_sample_energy")


def test_energy_score_names_in_header_binding_and_library():
    from genpose2_amd import _lib
    header = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTED, n
    assert "gp_head_grad_weights" in header
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.gp_abi_version() == 7                       # additive: the ABI version stays
    assert lib.gp_head_grad_floats() == 16 * 256 + 256 * 256 + 256 * 768


def test_transposed_packing_unpacks_to_the_transpose(energy_sd):
    from genpose2_amd import pack, weights
    p = weights.head_params(energy_sd)
    g = pack.pack_heads_grad(energy_sd)
    assert tuple(g) == pack.HEAD_GRAD_FIELDS
    w0 = pack.unpack_a_fragments(g["pe0_wt"], 16, 256)
    assert np.array_equal(w0[:9], p["pe0_w"].T) and not w0[9:].any()
    assert np.array_equal(pack.unpack_a_fragments(g["pe2_wt"], 256, 256), p["pe2_w"].T)
    assert np.array_equal(pack.unpack_a_fragments(g["h1p_wt"], 256, 768), p["h1_pose"].reshape(768, 256).T)
    # the forward fragments hold the same matrices untransposed: the reverse pass streams W^T the way the trunk
    # streams W
    f = pack.pack_heads(energy_sd)
    assert np.array_equal(pack.unpack_a_fragments(f["h1p_w"], 768, 256).T, pack.unpack_a_fragments(g["h1p_wt"], 256, 768))


def test_host_grad_pack_is_byte_identical(energy_sd):
    from genpose2_amd import _lib, pack, weights
    lib = _lib.load()
    p = weights.head_params(energy_sd)
    arrs = [np.ascontiguousarray(a, np.float32) for a in
            (p["pe0_w"], p["pe2_w"], p["h1_pose"].reshape(768, 256))]
    out = np.full(int(lib.gp_head_grad_floats()), np.nan, np.float32)
    _lib.check(lib.gp_head_grad_pack(*[a.ctypes.data_as(ctypes.c_void_p) for a in arrs],
                                     out.ctypes.data_as(ctypes.c_void_p)), "head_grad_pack")
    g = pack.pack_heads_grad(energy_sd)
    want = np.concatenate([g[k] for k in pack.HEAD_GRAD_FIELDS])
    assert out.tobytes() == want.tobytes()
    assert lib.gp_head_grad_pack(None, None, None, None) != 0      # null pointers are an error, not a crash


def _grad_weights_worker(rank, world, port, out_dir):
    import types
    import torch.distributed as dist
    from genpose2_amd import device as dev, pack, shard, weights
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        cpu = torch.device("cpu")
        sd = weights.synthetic_state_dict("energy", seed=0 if rank == 0 else 99)
        # what broadcast_agent reads of an agent; the buffers live on the host, so the re-tiling (plain tensor
        # copies) and the collective run here as they do on the device
        agent = types.SimpleNamespace(device=cpu, encoder=dev.EncoderModel(sd, cpu), heads=dev.HeadModel(sd, cpu),
                                      scale=None, pointwise=False, _pc_cache={})
        h = agent.heads
        own = pack.pack_heads_grad(sd)
        gw = h.grad_weights
        ok = all(np.array_equal(h._gw[0][k].numpy(), own[k]) and h._gw[0][k].data_ptr() == getattr(gw, k)
                 for k in pack.HEAD_GRAD_FIELDS)
        ok &= h.grad_weights is gw                                   # kept while nobody reports a change
        before = [h.up.t[k]._version for k in ("pe0_w", "pe2_w", "h1p_w")]
        shard.broadcast_agent(agent, src=0)
        # the collective's write is invisible to the version counters: nothing but the explicit hook can follow it
        ok &= [h.up.t[k]._version for k in ("pe0_w", "pe2_w", "h1p_w")] == before
        want = pack.pack_heads_grad(weights.synthetic_state_dict("energy", seed=0))
        ok &= rank == 0 or not np.array_equal(own["pe2_wt"], want["pe2_wt"])
        ok &= h.grad_weights is not gw
        ok &= all(np.array_equal(h._gw[0][k].numpy(), want[k]) for k in pack.HEAD_GRAD_FIELDS)
        np.save(os.path.join(out_dir, f"ok_{rank}.npy"), np.array(bool(ok)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_grad_weights_follow_a_weight_broadcast(tmp_path):
    """Two gloo ranks with different weights: after shard.broadcast_agent the transposed buffers of the reverse
    pass are rebuilt from rank 0's forward fragments on every rank, although they had been made (and cached)
    from the rank's own weights before -- the collective writes the forward buffers in place without touching
    their version counters, so the broadcast drops the copies itself."""
    import torch.multiprocessing as mp
    world = 2
    port = 29800 + os.getpid() % 1000
    mp.spawn(_grad_weights_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all(np.load(tmp_path / f"ok_{r}.npy") for r in range(world))


def test_float64_restatement_equals_reference_float64(energy_sd):
    """energy_ref.energy_score64 is the reference's float64 return_item='score_and_energy' to 1e-10 of the
    per-time maximum, with the same kink margins."""
    import energy_ref
    g = golden("energy_score")
    feat_rows = np.repeat(g["pts_feat"], g["pose"].shape[0] // g["pts_feat"].shape[0], 0)
    for j, t in enumerate(g["t"]):
        s, e, m = energy_ref.energy_score64(energy_sd, feat_rows, g["pose"], t)
        es = np.abs(s - g["score64"][j]).max() / np.abs(g["score64"][j]).max()
        ee = np.abs(e - g["energy64"][j]).max() / np.abs(g["energy64"][j]).max()
        print(f"t={t:g}: restatement vs reference float64: score {es:.2e}, energy {ee:.2e}")
        assert es <= 1e-10 and ee <= 1e-10, (t, es, ee)
        np.testing.assert_allclose(m, g["margin"][j], rtol=1e-6, atol=1e-12)


def test_float64_pc_restatement_follows_reference_trajectory(energy_sd):
    """energy_ref.pc_step (the update the GPU test recomputes per step) with energy_score64's score, in float64,
    teacher-forced on the reference's float64 trajectory: every state and the result to 1e-9 of max |x|."""
    import energy_ref
    import energy_score_inputs as ei
    from genpose2_amd import arch
    g = golden("energy_pc")
    K, T = ei.PC_K, ei.PC_T
    feat_rows = np.repeat(g["pts_feat"], K, 0)
    cen = torch.from_numpy(np.repeat(g["pts_center"], K, 0)).double()
    ts = np.linspace(1.0, arch.SAMPLING_EPS, T)
    x = torch.from_numpy(g["prior"]).double() * (arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** 1.0)
    xs64 = torch.from_numpy(g["xs64"])
    for i, t in enumerate(ts):
        s, _, _ = energy_ref.energy_score64(energy_sd, feat_rows, x.numpy(), t)
        sig = arch.SIGMA_MIN * (arch.SIGMA_MAX / arch.SIGMA_MIN) ** t
        gt = sig * np.sqrt(2 * (np.log(arch.SIGMA_MAX) - np.log(arch.SIGMA_MIN)))
        dt = ts[0] - ts[1]
        nx, mean = energy_ref.pc_step(x, torch.from_numpy(s), torch.from_numpy(g["z1"][i]).double(),
                                      torch.from_numpy(g["z2"][i]).double(), gt, dt, np.sqrt(dt))
        want = xs64[:, i].clone()
        err = float((nx + torch.cat([torch.zeros_like(cen), torch.zeros_like(cen), cen], 1) - want).abs().max() /
                    want.abs().max())
        print(f"step {i}: restated update vs reference float64 trajectory {err:.2e}")
        assert err <= 1e-9, (i, err)
        x = want.clone()
        x[:, 6:] -= cen
    mean[:, 6:] += cen
    res = energy_ref.gs6(mean)
    err = float((res - torch.from_numpy(g["pred_pose64"])).abs().max() / np.abs(g["pred_pose64"]).max())
    assert err <= 1e-9, err


def test_fixture_inputs_regenerate_from_their_seeds():
    import energy_score_inputs as ei
    g = golden("energy_score")
    for k, v in ei.eval_inputs().items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    o = golden("energy_pc")
    for k, v in ei.pc_inputs().items():
        assert o[k].dtype == v.dtype and np.array_equal(o[k], v), k
    assert os.path.exists(os.path.join(GOLDEN, "make_golden_energy_score.py"))


def test_fixture_kink_exclusions_within_caps():
    import energy_score_inputs as ei
    g = golden("energy_score")
    excl = g["margin"] < ei.KINK_MARGIN
    print("eval: rows under the kink margin:", int(excl.sum()), "of", excl.size)
    assert excl.size == 200 and excl.sum() <= ei.MAX_EXCLUDED_EVAL * excl.size
    o = golden("energy_pc")
    excl = o["margin"] < ei.KINK_MARGIN
    print("pc: rows under the kink margin:", int(excl.sum()), "of", excl.size)
    assert excl.size == 40 and excl.sum() <= ei.MAX_EXCLUDED_PC * excl.size
