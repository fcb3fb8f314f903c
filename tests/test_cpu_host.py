"""CPU-only tests of the host side: C-ABI exports, packing, SDE scalars, RK45 controller,
DBSCAN restatement, aggregation, sharding (gloo, world_size 2). No HIP compute calls."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    so = os.path.join(REPO, "genpose2_amd", "libgenpose_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "genpose2_amd", "csrc")], check=True)
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gp_[a-z0-9_]+)$", nm, re.M))
    assert declared and declared <= exported, declared - exported
    from genpose2_amd import _lib
    assert set(_lib.EXPORTED) == declared   # the ctypes binding covers exactly the header
    lib = _lib.load()
    assert lib.gp_abi_version() == 7
    assert lib.gp_encoder_workspace_size(64, 1024) > 0 and lib.gp_pc_workspace_size(3200) >= 3200 * 36


def _gfx950_code_objects(so):
    """The gfx950 ELF code objects of a HIP shared library (its .hip_fatbin clang offload bundles)."""
    import struct
    import tempfile
    objcopy = "/opt/rocm/lib/llvm/bin/llvm-objcopy"
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fatbin")
        subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fb}", so, os.path.join(d, "copy")], check=True,
                       capture_output=True)
        b = open(fb, "rb").read()
    magic, out, pos = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (i := b.find(magic, pos)) >= 0:
        n = struct.unpack_from("<Q", b, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", b, off)
            off += 24
            triple = b[off:off + tl].decode()
            off += tl
            if triple.endswith("gfx950"):
                out.append(b[i + o:i + o + sz])
        pos = i + 1
    return out


def test_no_vector_loads_from_the_kernel_argument_segment():
    """Every kernel reads its arguments with scalar loads only. An argument array indexed per lane (the old
    proj_xyz_kernel's w0[br] / b0[br]) compiles to VECTOR loads from the kernel-argument segment, which the
    dispatch does not keep coherent for the vector caches: with other processes' kernels on the GPU a wave
    now and then read a stale pointer (the round-4 multirank mismatch, DESIGN (c)). Scans the disassembly of
    every gfx950 kernel for a vector memory instruction addressed from the argument pointer before that
    pointer's registers are overwritten, or a copy of it into a VGPR."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    so = os.path.join(REPO, "genpose2_amd", "libgenpose_hip.so")
    cos = _gfx950_code_objects(so)
    assert cos, "no gfx950 code object in the library"
    import tempfile
    bad, kernels = [], 0
    sreg = re.compile(r"^s\[?(\d+)(?::(\d+))?\]?$")
    for k, co in enumerate(cos):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        for fn, body in re.findall(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S):
            kernels += 1
            base = None           # the SGPR pair the first scalar load reads the arguments through
            for line in body.split("\n"):
                ins = line.split("//")[0].strip().replace(",", " ").split()
                if not ins:
                    continue
                op, args = ins[0], ins[1:]
                if base is None:
                    if op.startswith("s_load") and len(args) > 1:
                        base = args[1]
                    continue
                lo, hi = map(int, sreg.match(base).groups())
                if op.startswith(("global_load", "buffer_load", "flat_load")) and base in args[1:]:
                    bad.append(f"{fn}: {' '.join(ins)}")
                if op.startswith("v_mov") and len(args) > 1 and args[1] in (f"s{lo}", f"s{hi}"):
                    bad.append(f"{fn}: {' '.join(ins)}")
                # the pointer's registers overwritten: later uses are not the argument segment
                if args and op.startswith("s_") and not op.startswith(("s_cmp", "s_cbranch", "s_waitcnt", "s_barrier")):
                    m = sreg.match(args[0])
                    if m:
                        d0 = int(m.group(1))
                        d1 = int(m.group(2)) if m.group(2) else d0
                        if d0 <= hi and d1 >= lo:
                            break
    assert kernels > 50, kernels
    assert not bad, "\n".join(bad)


def test_no_12_byte_global_loads():
    """No kernel of the library reads memory with a 12-byte load (global/buffer/flat_load_dwordx3, ds_read_b96).
    Under other processes' kernels on the same GPU such a load now and then handed a wave a wrong second dword
    -- the level-0 projection lost its y term, then (with the projection fixed) the ball lists of levels 0-3
    changed from run to run: the round-4 multirank mismatch, DESIGN (c). Every 3-float read goes through
    gp_common.h ld1 (three 4-byte loads the compiler cannot merge). Scans the disassembly of every gfx950
    kernel."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    import tempfile
    cos = _gfx950_code_objects(os.path.join(REPO, "genpose2_amd", "libgenpose_hip.so"))
    assert cos, "no gfx950 code object in the library"
    bad, kernels = [], 0
    for co in cos:
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([objdump, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
        for fn, body in re.findall(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S):
            kernels += 1
            for line in body.split("\n"):
                ins = line.split("//")[0].strip().split()
                if ins and re.match(r"((global|buffer|flat)_load_dwordx3|ds_read_b96)$", ins[0]):
                    bad.append(f"{fn}: {' '.join(ins)}")
    assert kernels > 20
    assert not bad, "\n".join(bad[:20])


def test_invalid_arguments_return_status_not_exit():
    from genpose2_amd import _lib
    lib = _lib.load()
    rc = lib.gp_ball_query(1, 10, 1, 0.1, 0, None, None, None, None)
    assert rc == -1 and b"ball_query" in lib.gp_last_error()
    with pytest.raises(_lib.GenPoseHipError):
        _lib.check(lib.gp_furthest_point_sampling(1, 0, 1, None, None, None, None), "fps")
    # round-5 entry points: argument checks run before any device work
    assert lib.gp_encoder_geometry_levels(None, 1, 1024, None, 0, 0, 4, None) == -1
    assert b"encoder" in lib.gp_last_error()
    assert lib.gp_encoder_forward_geom_levels(None, None, None, 1, 1024, None, None, 0, None, 0, 5, None) == -1
    assert lib.gp_img_encoder2(None, None, None, 1, 256, 384, None, None, None, 0.0, None, None, None, 0.0, 0.0,
                               None, None, None, None, None, None, 0, None) == -1
    assert b"img_encoder" in lib.gp_last_error()
    buf = np.zeros(16, np.float32)   # non-null stand-ins: the level range is rejected before any launch
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.gp_encoder_geometry_levels(ptr, 1, 1024, ptr, 1 << 40, 2, 1, None) == -1
    assert b"levels [2, 1)" in lib.gp_last_error()


def test_a_fragment_packing_layout():
    from genpose2_amd import pack
    rng = np.random.default_rng(0)
    w = rng.normal(size=(40, 35)).astype(np.float32)
    p = pack.pack_a_fragments(w)
    assert p.size == 48 * 48
    # lane l of (tile T, k-group g) holds W[16T + l%16][16g + 4(l//16) + j]
    T, g, lane = 1, 2, 37
    off = ((T * 3 + g) * 64 + lane) * 4
    assert np.array_equal(p[off:off + 4], np.pad(w, ((0, 8), (0, 13)))[16 * T + lane % 16, 16 * g + 4 * (lane // 16):][:4])
    np.testing.assert_array_equal(pack.unpack_a_fragments(p, 48, 48)[:40, :35], w)


def test_split_f16_packing_layout_and_bounds(score_sd):
    from genpose2_amd import pack, weights
    rng = np.random.default_rng(1)
    w = (rng.normal(size=(32, 64)) * 0.05).astype(np.float32)
    e = pack.split_exponent(w)
    assert 2.0 ** 14 <= np.abs(w).max() * 2.0 ** e < 2.0 ** 15
    p = pack.pack_h16_fragments(w, e).view(np.float16).astype(np.float32)
    assert p.size == 2 * w.size
    # lane l of (tile T, chunk c, plane) holds W[16T + l%16][32c + 16(j//4) + 4(l//16) + j%4], j < 8
    T, c, lane = 1, 1, 37
    x = w.astype(np.float32) * np.float32(2.0 ** e)
    for j in range(8):
        k = 32 * c + 16 * (j // 4) + 4 * (lane // 16) + j % 4
        hi = p[(((T * 2 + c) * 2 + 0) * 64 + lane) * 8 + j]
        lo = p[(((T * 2 + c) * 2 + 1) * 64 + lane) * 8 + j]
        assert hi == np.float16(x[16 * T + lane % 16, k])
        assert abs((hi + lo) - x[16 * T + lane % 16, k]) <= 2.0 ** -21 * abs(x[16 * T + lane % 16, k])
    # hsc bounds the layer outputs for any pose input
    heads = pack.pack_heads(score_sd)
    p = weights.head_params(score_sd)
    A0, B0, A2, B2, e2, eh = heads["hsc"][:6]
    xs = rng.normal(size=(256, 9)).astype(np.float32) * 3
    a1 = np.maximum(xs @ p["pe0_w"].T + p["pe0_b"], 0)
    a2 = np.maximum(a1 @ p["pe2_w"].T + p["pe2_b"], 0)
    b1 = A0 * np.abs(xs).max(1) + B0
    assert (a1.max(1) <= b1).all() and (a2.max(1) <= A2 * b1 + B2).all()
    assert e2 == pack.split_exponent(p["pe2_w"]) and heads["pe2_h"].dtype == np.int32


def test_f16x3_head_planes_hold_every_bit(score_sd):
    """The head trunk's weight planes (pack.HEAD_PLANES = 3: hi, mid, lo): hi + mid + lo reproduces
    x = W * 2^e (max |x| in [2^14, 2^15)) to within half an f16 subnormal step, 2^-25 -- exactly unless
    the lo plane underflows, i.e. to 2^-39 of the layer's largest weight -- for every weight of
    pose_encoder.2 and head layer 1's pose block, in the [T][c][plane][lane][j] order gp_head.h streams."""
    from genpose2_amd import arch, pack, weights
    heads = pack.pack_heads(score_sd)
    p = weights.head_params(score_sd)
    for key, W in (("pe2_h", p["pe2_w"]), ("h1p_h", p["h1_pose"].reshape(3 * arch.HEAD_HID, arch.POSE_HID))):
        e = pack.split_exponent(W)
        n_out, k_in = W.shape
        pl = heads[key].view(np.float16).reshape(n_out // 16, k_in // 32, 3, 4, 16, 2, 4)
        assert pl.size == 3 * W.size
        full = pl.transpose(2, 0, 4, 1, 5, 3, 6).reshape(3, n_out, k_in).astype(np.float64)
        x = W.astype(np.float64) * 2.0 ** e
        err = np.abs(full[0] + full[1] + full[2] - x)
        assert err.max() <= 2.0 ** -25, (key, err.max())
        assert (err == 0).mean() > 0.999, key
        assert np.array_equal(full[0], x.astype(np.float16))       # hi = f16(x)
        assert (np.abs(full[2]) <= np.abs(x) * 2.0 ** -21).all()   # lo is ~2^-22 of the value
    # the 2-plane encoder layout is the first two planes of the same rule
    rng = np.random.default_rng(2)
    w = (rng.normal(size=(32, 64)) * 0.05).astype(np.float32)
    e = pack.split_exponent(w)
    two = pack.pack_h16_fragments(w, e, 2).view(np.float16).reshape(2, 2, 2, -1)
    three = pack.pack_h16_fragments(w, e, 3).view(np.float16).reshape(2, 2, 3, -1)
    assert np.array_equal(two, three[:, :, :2])


def test_encoder_packing_covers_every_layer(score_sd):
    from genpose2_amd import arch, pack, weights
    buf, off = pack.pack_encoder(score_sd)
    for lv, brs in enumerate(arch.sa_branches()):
        for br in brs:
            n = len(br.widths) - 1
            assert (off[lv, br.branch, :n, :2] >= 0).all() and (off[lv, br.branch, n:] == -1).all()
            assert (off[lv, br.branch, :n, :2] % 4 == 0).all()    # 16-byte aligned
            for i in range(n):   # split-f16 planes: every layer of levels 1-4, layers 1-2 of level 0
                has = lv >= 1 or i >= 1
                assert (off[lv, br.branch, i, 2] >= 0) == has == pack.enc_split_layer(lv, i)
                if has:
                    assert off[lv, br.branch, i, 2] % 4 == 0
                    W, _ = weights.encoder_layers(score_sd)[lv][br.branch][i]
                    if i == 0:   # layer-0 inputs permuted to [feats | xyz]
                        W = np.concatenate([W[:, 3:], W[:, :3]], 1)
                    e = int(off[lv, br.branch, i, 3])
                    n_pad, k_pad = pack.pad32(W.shape[0]), pack.pad32(W.shape[1])
                    words = buf[off[lv, br.branch, i, 2]:][: n_pad * k_pad].view(np.int32)
                    pl = words.view(np.float16).reshape(n_pad // 16, k_pad // 32, 2, 4, 16, 2, 4)
                    # [T][c][plane][q][i][half][j4] -> W[16T + i][32c + 16 half + 4q + j4] * 2^e
                    full = pl.transpose(2, 0, 4, 1, 5, 3, 6).reshape(2, n_pad, k_pad).astype(np.float64)
                    rec = (full[0] + full[1]) / 2.0 ** e
                    assert np.abs(rec[:W.shape[0], :W.shape[1]] - W).max() <= 2.0 ** -21 * np.abs(W).max()
                    assert not rec[W.shape[0]:].any() and not rec[:, W.shape[1]:].any()
    assert off[..., :3].max() < buf.size


def test_pc_step_table_matches_reference_formula():
    from genpose2_amd import sde
    from oracle import oracle
    tab = sde.pc_step_table(500)
    ts = oracle.time_grid(500)
    np.testing.assert_array_equal(tab[:, 0], ts)
    np.testing.assert_array_equal(tab[:, 1], oracle.ve_sigma(ts))
    np.testing.assert_array_equal(tab[:, 2], oracle.ve_diffusion(ts))
    assert tab[0, 3] == np.float32(ts[0] - ts[1])
    assert tab[0, 4] == np.sqrt(np.float32(ts[0] - ts[1]))


@pytest.mark.parametrize("t_eval", [None, 15, 400])
@pytest.mark.parametrize("t0", [1.0, 0.55])
def test_rk45_controller_matches_scipy(t_eval, t0):
    """The RK45 controller (rk45_drive) over scipy's own NumPy stage arithmetic (NumpyRk45)
    reproduces solve_ivp bit for bit: accept/reject sequence, times, outputs, nfev."""
    from scipy.integrate import solve_ivp
    from genpose2_amd.ode import NumpyRk45, rk45_drive
    A = np.array([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.0, -0.3, -0.1]])

    def f_np(t, y):
        return A @ y + np.sin(3 * t) * y ** 2 * 0.1

    y0 = np.array([1.0, -0.5, 2.0])
    te = None if t_eval is None else np.linspace(t0, 1e-5, t_eval)
    ref = solve_ivp(f_np, (t0, 1e-5), y0, method="RK45", rtol=1e-5, atol=1e-5, t_eval=te)
    be = NumpyRk45(f_np, y0)
    ts, nfev, status = rk45_drive(be, t0, 1e-5, t_eval=te)
    assert status == 0 and nfev == ref.nfev
    np.testing.assert_array_equal(ts, ref.t)
    ys = np.stack(be.ys, 1) if te is None else np.stack([v for _, v in be.dense_rows], 1)
    np.testing.assert_array_equal(ys, ref.y)


def test_ode_stage_scalars_vectorised():
    """stage_scalars (one vectorised pass per attempt) == time_scalars per value, which forms the
    scalars as ode_func does (samplers.py:209-216)."""
    from genpose2_amd.ode import stage_scalars, time_scalars
    rng = np.random.default_rng(3)
    ts = [np.float64(v) for v in np.concatenate([rng.uniform(1e-5, 1.0, 3000), [1.0, 0.55, 1e-5, 0.2]])]
    for i in range(0, len(ts) - 6, 6):
        t32, sig, coef = stage_scalars(ts[i:i + 6])
        for j in range(6):
            a, b, c = time_scalars(ts[i + j])
            assert (float(t32[j]), float(sig[j]), float(coef[j])) == (a, b, c)


def test_ode_first_rhs_uses_float32_diffusion():
    """solve_ivp passes t0 as a Python float, so ode_func's torch.tensor(t) is float32 for the first
    evaluation only (ivp.py map(float, t_span); sde.py:22-27)."""
    from genpose2_amd.ode import time_scalars
    a = time_scalars(0.55)[2]
    b = time_scalars(np.float64(0.55))[2]
    g32 = 0.01 * (50.0 / 0.01) ** torch.tensor(0.55)
    assert g32.dtype == torch.float32 and a != b


def test_dbscan_restatement_matches_sklearn():
    from sklearn.cluster import DBSCAN
    from oracle.oracle import dbscan_labels
    g = golden("pipeline")
    rng = np.random.default_rng(1)
    cases = [rng.normal(size=(20, 20)) * s for s in (0.01, 0.03, 0.1)]
    for j in range(4):   # the clustered fixture's distance matrices
        q = torch.from_numpy(g["cl_pose"][j, :20, :6])
        from genpose2_amd.aggregate import matrix_to_quaternion, rot6_to_matrix
        qq = matrix_to_quaternion(rot6_to_matrix(q))
        cases.append((1 - (qq[None] * qq[:, None]).sum(-1) ** 2).numpy())
    for X in cases:
        for ms in (1, 3, 5):
            ref = DBSCAN(eps=0.05, min_samples=ms).fit(X).labels_
            np.testing.assert_array_equal(dbscan_labels(X, 0.05, ms), ref)


def test_shard_ranges_cover_every_object_once():
    from genpose2_amd.shard import shard_range
    for total, world in [(2048, 8), (64, 2), (65, 8), (3, 8)]:
        seen = []
        for r in range(world):
            lo, hi = shard_range(total, world, r)
            seen += list(range(lo, hi))
        assert seen == list(range(total))


def _shard_reference(lo, hi, K, T):
    """The per-shard computation (oracle): encoder + PC sampler (noise rows of objects lo..hi-1)
    + energy + aggregation, i.e. a reference call on the sub-batch."""
    from genpose2_amd import synthetic, weights
    from oracle import oracle
    pts, center = synthetic.make_batch(4, hi - lo, 1024, first_object=lo)
    rng = [np.random.Generator(np.random.PCG64(1000 + b)) for b in range(lo, hi)]
    prior = np.concatenate([r.standard_normal((K, 9), dtype=np.float32) for r in rng])
    z = np.stack([np.concatenate([r.standard_normal((2 * T, 9), dtype=np.float32) for _ in range(K)], 1)
                  for r in rng], 0)                                  # (b, 2T, K*9) -> rows of this shard
    z = z.reshape(hi - lo, 2 * T, K, 9).transpose(1, 0, 2, 3).reshape(2 * T, (hi - lo) * K, 9)
    pose, _, feat, _ = oracle.pred_func(weights.synthetic_state_dict("score"), pts, center, K, T, "pc", prior,
                                        z[0::2], z[1::2])
    energy = oracle.get_energy(weights.synthetic_state_dict("energy"), pts, center, pose, 1e-5)
    agg = oracle.aggregate_pose(pose, energy, clustering=0)
    return {"pred_pose": pose, "pts_feat": feat, "energy": energy, "aggregated": agg}


def _gloo_worker(rank, world, port, out_dir, total):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from genpose2_amd import shard, weights
    # every agent's packed buffers (encoder + heads for score/energy, ScaleNet): rank 0 owns the
    # weights, the others start from different ones and receive rank 0's by broadcast (the RCCL step)
    ok = True
    for kind in ("score", "energy", "scale"):
        sd_mine = weights.synthetic_state_dict(kind, seed=0 if rank == 0 else 99)
        mine = shard.packed_host_tensors(kind, sd_mine)
        # the host layer tables (split-f16 exponents of the weight VALUES) travel with the buffers
        tabs = shard.broadcast_packed(mine, shard.packed_host_tables(kind, sd_mine), src=0)
        sd_ref = weights.synthetic_state_dict(kind, seed=0)
        ref = shard.packed_host_tensors(kind, sd_ref)
        ref_tabs = shard.packed_host_tables(kind, sd_ref)
        ok &= len(mine) == len(ref) and all(torch.equal(a, b) for a, b in zip(mine, ref))
        ok &= len(tabs) == len(ref_tabs) and all(np.array_equal(a, b) for a, b in zip(tabs, ref_tabs))
        if rank != 0 and kind != "scale":
            # the seeds differ in at least one exponent, or this check would prove nothing
            ok &= not all(np.array_equal(a, b) for a, b in zip(shard.packed_host_tables(kind, sd_mine), ref_tabs))
    lo, hi = shard.shard_range(total, world, rank)
    K, T = 4, 5
    if hi > lo:
        out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _shard_reference(lo, hi, K, T).items()}
    else:
        out = {"pred_pose": torch.zeros(0, K, 9), "pts_feat": torch.zeros(0, 1024), "energy": torch.zeros(0, K, 2),
               "aggregated": torch.zeros(0, 4, 4)}
    out["length"] = None
    g = shard.gather_outputs(out, total)                 # on every rank
    g0 = shard.gather_outputs(out, total, dst=0)         # on rank 0 only
    ok &= (g0 is None) == (rank != 0) and g["length"] is None
    if rank == 0:
        for k in ("pred_pose", "pts_feat", "energy", "aggregated"):
            np.save(os.path.join(out_dir, f"{k}.npy"), g[k].numpy())
            ok &= torch.equal(g[k], g0[k])
    np.save(os.path.join(out_dir, f"ok_{rank}.npy"), np.array(ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,total", [(2, 5), (3, 2)])
def test_gloo_sharded_broadcast_and_gather(tmp_path, world, total):
    """world_size 2 and 3 (gloo): broadcast of every agent's packed buffers, per-rank shards (uneven,
    and an empty shard when ranks outnumber objects), gather of the per-object outputs in object
    order on every rank and on rank 0 -- equal to the per-shard computations concatenated."""
    import torch.multiprocessing as mp
    from genpose2_amd import shard
    port = 29500 + (os.getpid() + world) % 1000
    mp.spawn(_gloo_worker, args=(world, port, str(tmp_path), total), nprocs=world, join=True)
    assert all(np.load(tmp_path / f"ok_{r}.npy") for r in range(world))
    parts = [_shard_reference(*shard.shard_range(total, world, r), 4, 5) for r in range(world)
             if shard.shard_range(total, world, r)[1] > shard.shard_range(total, world, r)[0]]
    for k in ("pred_pose", "pts_feat", "energy", "aggregated"):
        np.testing.assert_array_equal(np.load(tmp_path / f"{k}.npy"), np.concatenate([p[k] for p in parts]))


@pytest.mark.parametrize("t_eval", [None, 40])
def test_rk45_controller_failed_solve_matches_scipy(t_eval):
    """A solve that fails ("required step size is less than spacing between numbers", status -1):
    y' = -y^2 has the solution 1/(t - 0.3), singular inside (1e-5, 0.55). The controller stops where
    solve_ivp stops, with the same nfev, times and collected outputs (the t_eval points before the
    failure), which is what cond_ode_sampler's res.y[:, -1] then reads."""
    import warnings
    from scipy.integrate import solve_ivp
    from genpose2_amd.ode import NumpyRk45, rk45_drive

    def f_np(t, y):
        return -y * y

    y0 = np.array([1.0 / (0.55 - 0.3), 2.0 / (0.55 - 0.3)])
    te = None if t_eval is None else np.linspace(0.55, 1e-5, t_eval)
    ref = solve_ivp(f_np, (0.55, 1e-5), y0, method="RK45", rtol=1e-5, atol=1e-5, t_eval=te)
    assert ref.status == -1
    be = NumpyRk45(f_np, y0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts, nfev, status = rk45_drive(be, 0.55, 1e-5, t_eval=te)
    assert status == -1 and nfev == ref.nfev
    np.testing.assert_array_equal(ts, ref.t)
    ys = np.stack(be.ys, 1) if te is None else np.stack([v for _, v in be.dense_rows], 1)
    np.testing.assert_array_equal(ys, ref.y)


@pytest.mark.parametrize("kind", ["score", "energy", "scale"])
def test_manifest_matches_reference_checkpoint_layout(kind):
    """The weight manifest (keys, shapes, dtypes) equals the model_state_dict the reference's own
    save_ckpt writes (golden_ckpt_layout.json, generated by make_golden.py ckpt)."""
    import json
    from conftest import GOLDEN
    from genpose2_amd import weights
    with open(os.path.join(GOLDEN, "golden_ckpt_layout.json")) as f:
        lay = json.load(f)[kind]
    assert lay["top_level_keys"] == ["clock", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    sd = weights.synthetic_state_dict(kind)
    assert sorted(sd) == sorted(lay["model_state_dict"])
    for k, (shape, dt) in lay["model_state_dict"].items():
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == dt, k


@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_checkpoint_reference_format(tmp_path, prefix):
    """weights.load_checkpoint (PoseNet.load_ckpt's loader) reads a save_ckpt-format file with
    torch.load(weights_only=True), strips DataParallel's "module." prefix, and packs to exactly the
    buffers the synthetic weights pack to; a missing file raises ValueError like the reference."""
    from conftest import write_reference_checkpoint
    from genpose2_amd import pack, weights
    for kind in ("score", "scale"):
        path = write_reference_checkpoint(str(tmp_path / f"{kind}.pth"), kind, prefix=prefix)
        sd = weights.load_checkpoint(path)
        weights.check_keys(sd, kind)
        ref = weights.synthetic_state_dict(kind)
        for k in ref:
            np.testing.assert_array_equal(sd[k], ref[k])
        if kind == "score":
            a, b = pack.pack_heads(sd), pack.pack_heads(ref)
            assert all(np.array_equal(a[k], b[k]) for k in a)
            np.testing.assert_array_equal(pack.pack_encoder(sd)[0], pack.pack_encoder(ref)[0])
    with pytest.raises(ValueError):
        weights.load_checkpoint(str(tmp_path / "missing.pth"))


def test_fus_manifest_matches_reference_layout():
    """The fused encoder's manifest equals the reference Pointnet2ClsMSGFus(384) state dict (keys and
    shapes; golden_fus_layout.json, written by tests/golden/make_golden_fus.py)."""
    import json
    from conftest import GOLDEN
    from genpose2_amd import weights
    with open(os.path.join(GOLDEN, "golden_fus_layout.json")) as f:
        lay = json.load(f)
    mine = {k[len("pts_encoder."):]: list(s) for k, s, _ in weights.fus_encoder_manifest()}
    assert mine == lay


def _pack_host(kind_id, sd):
    """gp_weights_pack_host over a state dict (host arrays); returns (buffer, fields, enc_table)."""
    import ctypes
    from genpose2_amd import _lib
    lib = _lib.load()
    keys = [k for k, v in sd.items() if v.dtype == np.float32]
    arrs = [np.ascontiguousarray(sd[k], np.float32) for k in keys]
    names = (ctypes.c_char_p * len(keys))(*[k.encode() for k in keys])
    data = (ctypes.c_void_p * len(keys))(*[a.ctypes.data for a in arrs])
    numel = np.array([a.size for a in arrs], np.int64)
    fields = np.zeros(25, np.int64)
    table = np.zeros(120, np.int64)
    need = ctypes.c_size_t(0)
    args = (kind_id, len(keys), ctypes.cast(names, ctypes.c_void_p), ctypes.cast(data, ctypes.c_void_p),
            numel.ctypes.data)
    _lib.check(lib.gp_weights_pack_host(*args, None, 0, ctypes.byref(need), fields.ctypes.data_as(_lib.c_int64_p),
                                        table.ctypes.data_as(_lib.c_int64_p)), "pack_host size")
    buf = np.zeros(need.value, np.float32)
    _lib.check(lib.gp_weights_pack_host(*args, buf.ctypes.data, buf.size, ctypes.byref(need),
                                        fields.ctypes.data_as(_lib.c_int64_p), table.ctypes.data_as(_lib.c_int64_p)),
               "pack_host")
    return buf, fields, table


@pytest.mark.parametrize("kind,kind_id", [("score", 0), ("energy", 1), ("scale", 2)])
def test_weights_pack_host_matches_pack_py(kind, kind_id):
    """The C++ packer behind gp_weights_pack (the non-Python load path) writes byte-identical layouts to
    genpose2_amd/pack.py: folded + fragment-packed encoder and its table, every head field (split-f16
    planes and activation bounds included), ScaleNet copies; a "module." prefix is accepted."""
    from genpose2_amd import pack, weights
    sd = weights.synthetic_state_dict(kind)
    sd_mod = {("module." + k if i % 2 else k): v for i, (k, v) in enumerate(sd.items())}
    buf, fields, table = _pack_host(kind_id, sd_mod)
    if kind == "scale":
        ref = pack.pack_scale(sd)
        for i, k in enumerate(pack.SCALE_FIELDS):
            v = ref[k].reshape(-1)
            np.testing.assert_array_equal(buf[fields[17 + i]:fields[17 + i] + v.size], v)
        assert fields[0] == -1
        return
    ebuf, etab = pack.pack_encoder(sd)
    np.testing.assert_array_equal(table.reshape(5, 2, 3, 4), etab)
    assert fields[0] == 0
    np.testing.assert_array_equal(buf[:ebuf.size].view(np.uint32), ebuf.view(np.uint32))
    ref = pack.pack_heads(sd)
    for i, k in enumerate(pack.HEAD_FIELDS):
        v = ref[k].reshape(-1).view(np.uint32)
        np.testing.assert_array_equal(buf[fields[1 + i]:fields[1 + i] + v.size].view(np.uint32), v, err_msg=k)


def test_weights_pack_host_reports_missing_key():
    from genpose2_amd import _lib, weights
    sd = weights.synthetic_state_dict("score")
    del sd["pose_score_net.pose_encoder.2.bias"]
    with pytest.raises(_lib.GenPoseHipError, match="pose_encoder.2.bias"):
        _pack_host(0, sd)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("genpose_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_launcher_plan():
    """bench.py --gpus N: in-process for N=1 or inside a launcher whose WORLD_SIZE is N; a torchrun CHILD
    with N ranks otherwise; a loud failure when N GPUs are missing or WORLD_SIZE disagrees."""
    b = _bench_module()
    assert b.launch_command(["--gpus", "1"], 1, {}, 0) is None
    assert b.launch_command(["--gpus", "8"], 8, {"WORLD_SIZE": "8"}, 8) is None
    cmd = b.launch_command(["--gpus", "4", "--steps", "3"], 4, {}, 8)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert "--master-addr=127.0.0.1" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    with pytest.raises(SystemExit, match="only 1 HIP device"):
        b.launch_command(["--gpus", "2"], 2, {}, 1)
    with pytest.raises(SystemExit, match="WORLD_SIZE=1"):
        b.launch_command(["--gpus", "2"], 2, {"WORLD_SIZE": "1"}, 8)


def test_bench_gpus2_without_gpus_fails_loudly():
    """On a host with fewer GPUs than --gpus the bench exits non-zero instead of printing n_gpus: 1."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode != 0 and ("HIP device" in p.stderr or "cannot count" in p.stderr), p.stderr[-2000:]
    assert '"n_gpus"' not in p.stdout


def test_bench_has_full_and_dump_options(monkeypatch, capsys):
    """bench.py takes --full (everything beside the headline figure) and --dump-outputs DIR."""
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text


def test_bench_counts_gpus_without_hip(monkeypatch, tmp_path):
    """bench.py --gpus N counts the node's GPUs before the launcher starts, without any HIP call: amdsmi,
    else the KFD topology (nodes with a non-zero gfx_target_version); with neither it exits non-zero and
    never falls back to torch.cuda.device_count() (hipGetDeviceCount in the parent of the ranks)."""
    b = _bench_module()

    def hip_touched(*a, **k):
        raise AssertionError("HIP touched before the launcher")
    for fn in ("device_count", "is_available", "init", "_lazy_init", "set_device", "current_device"):
        monkeypatch.setattr(torch.cuda, fn, hip_touched)
    monkeypatch.setitem(sys.modules, "amdsmi", None)          # import amdsmi -> ImportError
    # a fake KFD topology: one CPU node, two GPU nodes
    for i, ver in enumerate((0, 90500, 90500)):
        d = tmp_path / "nodes" / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text(f"cpu_cores_count 4\ngfx_target_version {ver}\nsimd_count 0\n")
    monkeypatch.setattr(b, "KFD_NODES", str(tmp_path / "nodes" / "*" / "properties"))
    assert b.count_gpus({}) == 2
    assert b.count_gpus({"HIP_VISIBLE_DEVICES": "0"}) == 1
    monkeypatch.setattr(b, "KFD_NODES", str(tmp_path / "absent" / "*" / "properties"))
    assert b.count_gpus({}) is None
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert "cannot count" in str(e.value.code)


def test_bench_rocprof_source_matches_config(tmp_path, monkeypatch):
    """The roofline's rocprof figure comes from a summary of the same config (row count, tile) and kernel
    instantiation, newest round first, then reverse lexical order -- never another config's file or an
    mtime order."""
    b = _bench_module()
    monkeypatch.setattr(b, "REPO", str(tmp_path))
    hdr = "Name,Calls,TotalDurationNs,AverageNs,Percentage,MinNs,MaxNs,StdDev\n"

    def csv(path, kernel, avg):
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(hdr + f'"{kernel}(PCArgs, int, PCStep, PCStep)",501,1,{avg},50,1,1,0\n')
    k4, k1 = "void pc_step_kernel<4, 8, 3>", "void pc_step_kernel<1, 8, 0>"
    csv(tmp_path / "profiles" / "r3" / "config4_r3f_kernel_stats.csv", k4, 23890)
    csv(tmp_path / "profiles" / "r4" / "config4_a_kernel_stats.csv", k4, 30000)
    csv(tmp_path / "profiles" / "r4" / "config4_b_kernel_stats.csv", k4, 31000)
    csv(tmp_path / "profiles" / "r4" / "config5_a_kernel_stats.csv", k4, 60000)
    csv(tmp_path / "profiles" / "r4" / "config4_pointwise_a_kernel_stats.csv", k4, 32000)
    csv(tmp_path / "profiles" / "r10" / "config4_z_kernel_stats.csv", k1, 70000)
    assert b.load_rocprof(k4, 4)["avg_launch_us"] == 31.0           # r4 beats r3; b after a
    assert b.load_rocprof(k4, 4)["source"].endswith("r4/config4_b_kernel_stats.csv")
    assert b.load_rocprof(k1, 4)["avg_launch_us"] == 70.0           # r10 > r4 numerically
    assert b.load_rocprof(k4, 5)["avg_launch_us"] == 60.0
    assert b.load_rocprof(k4, 4, "pointwise")["avg_launch_us"] == 32.0
    assert b.load_rocprof(k4, 2) is None


def test_bench_launcher_starts_world2_gloo():
    """The launcher path end to end on CPU: bench.py --gpus 2 --launch-probe starts 2 ranks under torchrun
    (gloo), which all-reduce their ranks; rank 0 prints n_gpus 2."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--launch-probe"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line == {"launch_probe": True, "n_gpus": 2, "rank_sum": 1}


def test_c_pc_step_table_matches_sde_table():
    """gp_pc_step_table (the C host's table) against genpose2_amd/sde.py (torch, the reference's own
    arithmetic): t and dt bit-identical for every T in 2..1500; sqrt(dt) within 1 ulp and sigma, g within 3
    ulp (torch's CPU pow and sqrt are Sleef's 1-ulp vector routines, the C table's are correctly rounded;
    sigma = 0.01 * pow scales pow's 1-ulp difference into up to 2 ulp of sigma, and g rounds once more)."""
    import ctypes
    from genpose2_amd import _lib, sde
    lib = _lib.load()
    worst, n_diff, n = {1: 0, 2: 0, 4: 0}, 0, 0
    for T in list(range(2, 1501)) + [2000, 5000]:
        tab = np.zeros((T, 5), np.float32)
        _lib.check(lib.gp_pc_step_table(T, ctypes.c_float(1e-5), tab.ctypes.data_as(ctypes.c_void_p)))
        ref = sde.pc_step_table(T)
        for c in (0, 3):
            np.testing.assert_array_equal(tab[:, c], ref[:, c], err_msg=f"T={T} column {c}")
        for c in (1, 2, 4):
            ulp = np.abs(tab[:, c].view(np.int32).astype(np.int64) - ref[:, c].view(np.int32).astype(np.int64))
            worst[c] = max(worst[c], int(ulp.max()))
            n_diff += int((ulp > 0).sum())
        n += 3 * T
    assert worst[1] <= 3 and worst[2] <= 3 and worst[4] <= 1, worst
    print(f"sigma/g/sqrt(dt) entries differing: {n_diff} of {n}, worst ulp {worst}")
    assert lib.gp_pc_step_table(1, ctypes.c_float(1e-5), None) != 0


def test_energy_per_object_t_draws_like_reference():
    """PoseNet.per_object_energy_t consumes torch's default generator exactly as posenet_agent.py:677-685
    does (randint(int(T_min * 1e5), int(T_max * 1e5), (bs, 1)).type_as(float32 features) / 1e5)."""
    import torch
    from genpose2_amd.agent import PoseNet
    for bs in (1, 7, 64):
        torch.manual_seed(bs)
        ref = torch.randint(int(1e-5 * 1e5), int(1e-4 * 1e5), (bs, 1)).type_as(torch.zeros(1)) / 1e5
        torch.manual_seed(bs)
        got = PoseNet.per_object_energy_t(bs)
        assert got.dtype == torch.float32 and torch.equal(got, ref.view(bs))


def _vregs(op):
    """VGPR/AGPR indices named by one assembler operand (v7, v[4:7], a[0:3]); empty for others."""
    m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", op)
    if m:
        return {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.fullmatch(r"([va])(\d+)", op)
    return {(m.group(1), int(m.group(2)))} if m else set()


def test_no_permlane_swap_in_mfma_hazard_window():
    """the head trunks' v_permlane16/32_swap row reductions once overwrote registers that in-flight
    MFMAs still read (the swap writes BOTH of its operands), which only instruction scheduling kept apart.
    Disassembles every head kernel (PC step, score/energy eval, ODE stages) of the built library and checks that
    no swap's SOURCE operand -- the register the compiler's hazard recognizer may treat as read-only; its vdst
    gets the ISA's wait states (s_nop) like any VALU def -- is the result (vdst, which is also SrcC for the trunks'
    chained accumulators) of a v_mfma issued within the previous 11 wait states: a VALU write to an in-flight MFMA's
    vdst needs NumPasses + 2 wait states (8 passes for 16x16x4 f32, fewer for 16x16x32 f16: the compiler's own
    s_nop 8 + 1 before such writes; a separate SrcC, SrcA and SrcB are read at issue -- the compiler rewrites
    them on the next cycle), s_nop N counting N+1. Validated with the ROCm 7.2 clang that builds the library (hipcc --version)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    build = os.path.join(REPO, "genpose2_amd", "csrc", "build")
    if not all(os.path.exists(os.path.join(build, f)) for f in ("gp_score.o", "gp_ode.o")):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "genpose2_amd", "csrc")], check=True)
    window, checked = 11, 0
    for src in ("gp_score.o", "gp_ode.o"):
        tmp = os.path.join(build, src + ".fatbin")
        co = os.path.join(build, src + ".gfx950.co")
        subprocess.run([f"{llvm}/llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}", os.path.join(build, src),
                        os.devnull], check=True)
        subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={tmp}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        asm = subprocess.run([f"{llvm}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True,
                             check=True).stdout
        os.remove(tmp)
        os.remove(co)
        kernel, recent = None, []   # recent: (wait states since issue, regs) of MFMAs
        for line in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                kernel, recent = m.group(1), []
                continue
            code = line.split("//")[0].strip()
            if not code or kernel is None:
                continue
            parts = code.replace(",", " ").split()
            op, args = parts[0], parts[1:]
            if not re.search(r"head_eval|pc_step|ode_stage", kernel):
                continue
            step = int(args[0]) + 1 if op == "s_nop" and args else 1
            if op.startswith("v_permlane") and "swap" in op:
                written = _vregs(args[1])
                for _, regs in recent:
                    assert not (written & regs), (kernel, code)
                checked += 1
            recent = [(w + step, r) for w, r in recent if w + step < window]
            if op.startswith("v_mfma"):
                regs = _vregs(args[0])   # vdst
                recent.append((0, regs))
    assert checked > 50, checked   # the trunks' row reductions were found


def _exchange_worker(rank, world, port, out_dir, per):
    import torch.distributed as dist
    from genpose2_amd import shard
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        gb = shard.GlobalBatch.of(world * 3)
        assert (gb.lo, gb.hi, gb.per_max, gb.rank, gb.world) == (3 * rank, 3 * rank + 3, 3, rank, world)
        n = per * world
        part = torch.full((2 * n,), -1.0)
        ex = shard.PartialsExchange(part, n, gb)
        for step in range(3):   # the sampler fills this rank's chunk of slot step & 1, then calls the exchange
            base = (step & 1) * n
            part[base + rank * per:base + (rank + 1) * per] = torch.arange(per, dtype=torch.float32) + 100 * rank + step
            assert ex._call(None, step, part[base:].data_ptr(), n, None) == 0, ex.error
            want = torch.cat([torch.arange(per, dtype=torch.float32) + 100 * r + step for r in range(world)])
            assert torch.equal(part[base:base + n], want)
        assert ex._call(None, 0, part.data_ptr() + 4, n, None) == -1 and ex.error is not None   # wrong slot
        # the ODE's form: one slot of fp64 partials, exchanged after every attempt
        p64 = torch.full((n,), -1.0, dtype=torch.float64)
        ex64 = shard.PartialsExchange(p64, n, gb)
        for attempt in range(3):
            p64[rank * per:(rank + 1) * per] = torch.arange(per, dtype=torch.float64) / 3 + 100 * rank + attempt
            assert ex64._call(None, attempt, p64.data_ptr(), n, None) == 0, ex64.error
            want = torch.cat([torch.arange(per, dtype=torch.float64) / 3 + 100 * r + attempt for r in range(world)])
            assert torch.equal(p64, want)
        with pytest.raises(ValueError):
            shard.PartialsExchange(torch.zeros(3 * n), n, gb)
        # the whole batch's rows from uneven shards (7 objects x 4 rows over `world` ranks), in object order
        gb7 = shard.GlobalBatch.of(7)
        full = torch.arange(7 * 4 * 9, dtype=torch.float64).view(7 * 4, 9) * 0.5
        got = shard.gather_shard_rows(full[gb7.lo * 4:gb7.hi * 4].clone(), gb7, 4)
        assert torch.equal(got, full)
        with pytest.raises(ValueError):
            shard.gather_shard_rows(full[:3], gb7, 4)
        np.save(os.path.join(out_dir, f"ok_{rank}.npy"), np.array(True))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_global_batch_partials_exchange_gloo(tmp_path, world):
    """Global-batch sampling's host side (shard.GlobalBatch, shard.PartialsExchange, shard.gather_shard_rows)
    over gloo: every rank's chunk of the slot a scoring launch (PC: two fp32 slots) or an RK45 attempt (ODE:
    one fp64 slot) wrote reaches every rank in shard order, an unexpected slot pointer is reported as a failure
    (the C caller turns it into an error) instead of raising into C, and the ODE's initial-step vectors are
    gathered from uneven shards in object order."""
    import torch.multiprocessing as mp
    port = 29700 + (os.getpid() + world) % 1000
    mp.spawn(_exchange_worker, args=(world, port, str(tmp_path), 5), nprocs=world, join=True)
    assert all(np.load(tmp_path / f"ok_{r}.npy") for r in range(world))


def test_global_batch_rejects_empty_shards():
    from genpose2_amd import shard
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{29690 + os.getpid() % 300}", rank=0, world_size=1)
    try:
        assert shard.GlobalBatch.of(4).per_max == 4
        with pytest.raises(ValueError):
            shard.GlobalBatch.of(0)
    finally:
        dist.destroy_process_group()
