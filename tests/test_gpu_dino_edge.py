"""The DINOv3 backbone on the device off the fixture shapes (tests/golden/dino_edge_inputs.py): the tile boundaries of
dino_attention_kernel and dino_patch_embed_kernel, Hp > Wp, inputs that stress the softmax, a batch larger than one
natural chunk (which also runs the 256-row linear_split_kernel<4, ., 8> instances), and gp_dino_rope_table's values.
The references are tests/dino_ref.py in float64 on the CPU, computed when a test asks and shared by both arithmetics;
the bar is test_gpu_dino.py's: FACTOR x the float32 CPU run's own error, per layer and statistic."""
import ctypes

import numpy as np
import pytest
import torch

import dino_edge_inputs as de
import dino_inputs as di
import dino_ref
from test_gpu_dino import ARITHS, DEV, FACTOR, backbone, run

pytestmark = pytest.mark.gpu

_sharp = []


def edge_backbone(kind):
    """The shared backbone, or a second one over the sharpened state dict (built once)."""
    if kind == "plain":
        return backbone()
    if not _sharp:
        from genpose2_amd.dino import DinoBackbone
        _sharp.append(DinoBackbone(de.state_dict("sharp"), torch.device(DEV)))
    return _sharp[0]


def bar_failures(tag, outs, ref, layers):
    """Prints device error / float32 CPU error for every layer and statistic; -> those above FACTOR."""
    failures = []
    for i, l in enumerate(layers):
        got = outs[i].cpu().numpy()
        assert got.shape == ref["ref64"][i].shape and np.all(np.isfinite(got)), (tag, l)
        st = di.error_stats(got, ref["ref64"][i])
        for j, s in enumerate(di.STATS):
            y = float(ref["stats32"][i][j])
            print(f"dino edge {tag} layer {l} {s}: device {st[s]:.3e}  fp32 torch {y:.3e}  ratio {st[s] / y:.2f}")
            if not st[s] <= FACTOR * y:
                failures.append((l, s, st[s], FACTOR * y))
    return failures


# ------------------------------------------------------------------ 1. the edges against float64
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(de.CASES))
def test_backbone_matches_float64_at_the_edges(name, arith):
    """Measured on MI355X, device error over the float32 torch run's error (range over cases, layers and
    statistics): the table is in DESIGN.md "DINOv3 backbone off the fixture shapes"."""
    layers, kind = de.CASES[name][4], de.CASES[name][6]
    ref = de.reference(name)
    out = run(de.case_input(name), arith, n=layers, bb=edge_backbone(kind))
    failures = bar_failures(f"case {name} {arith}", out, ref, layers)
    assert not failures, failures


@pytest.mark.parametrize("arith", ARITHS)
def test_one_patch_embed_row_block_is_bit_identical(arith):
    """m64 with B = 4 is patch-embed m = 64, exactly one 64-row block with no clamped row; B = 5 adds a block of 16."""
    x = de.case_input("m64")
    five = run(x, arith, n=de.LAYERS)
    four = run(x[:4], arith, n=de.LAYERS)
    for a, b in zip(four, five):
        assert a.shape[0] == 4 and torch.equal(a, b[:4])


def _raw_forward(bb, x, layers, outs, arith, ws, ws_off, ws_bytes, grid=None):
    from genpose2_amd.dino import ARITH
    B, _, H, W = x.shape
    hp, wp = (H // 16, W // 16) if grid is None else grid
    wts = bb._weights(bb.rope_table(hp, wp) if grid is None else bb.rope_table(4, 6), hp, wp)
    lay = (ctypes.c_int * len(layers))(*layers)
    ptrs = (ctypes.c_void_p * len(layers))(*[o.data_ptr() + 256 * 4 for o in outs])
    rc = bb.lib.gp_dino_forward(ctypes.byref(wts), x.data_ptr(), B, H, W, len(layers), lay, ptrs, ARITH[arith],
                                ws.data_ptr() + ws_off, ws_bytes, None)
    torch.cuda.synchronize()
    return rc


def test_a_query_tile_of_one_row_stores_nothing_else():
    """strip_h (65 tokens): the second query tile holds one real row and 63 clamped ones; guard bands of 256 floats
    round every output and the workspace's padding keep their fill."""
    bb = backbone()
    x = torch.as_tensor(de.case_input("strip_h")).to(DEV)
    B, _, H, W = x.shape
    np_ = (H // 16) * (W // 16)
    need, pad = int(bb.lib.gp_dino_workspace_size(B, H, W)), 1 << 16
    for arith in ARITHS:
        want = run(x, arith, n=de.LAYERS)
        ws = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        outs = [torch.full((B * np_ * 384 + 2 * 256,), 7.0, dtype=torch.float32, device=DEV) for _ in de.LAYERS]
        rc = _raw_forward(bb, x, de.LAYERS, outs, arith, ws, pad, need)
        assert rc == 0, bb.lib.gp_last_error()
        assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + need:] == 0xA5).all())
        for o, w in zip(outs, want):
            assert bool((o[:256] == 7.0).all()) and bool((o[-256:] == 7.0).all())
            assert torch.equal(o[256:-256].view_as(w), w)


def test_more_than_the_most_patches_is_refused():
    """33 x 32 patches: ValueError from get_intermediate_layers, a non-zero code from gp_dino_forward, and outputs
    that keep their sentinel (buffers are sized for the refused shape all the same)."""
    bb = backbone()
    H, W = 16 * 33, 16 * 32
    x = torch.zeros((1, 3, H, W), device=DEV)
    calls = bb.calls
    with pytest.raises(ValueError, match="at most 1024 patches"):
        bb.get_intermediate_layers(x, n=[0])
    assert bb.calls == calls and int(bb.lib.gp_dino_workspace_size(1, H, W)) == 0
    ws_bytes = int(bb.lib.gp_dino_workspace_size(1, 512, 512)) * 33 // 32 + 4096
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    outs = [torch.full((33 * 32 * 384 + 2 * 256,), 7.0, dtype=torch.float32, device=DEV) for _ in range(2)]
    for arith in ARITHS:
        rc = _raw_forward(bb, x, (0, 2), outs, arith, ws, 0, ws_bytes, grid=(33, 32))
        assert rc != 0 and b"exceed 1024" in bb.lib.gp_last_error()
        assert all(bool((o == 7.0).all()) for o in outs) and bool((ws == 0xA5).all())


# ------------------------------------------------------------------ 2. a batch larger than one natural chunk
@pytest.mark.parametrize("arith", ARITHS)
def test_batch_of_one_image_more_than_a_chunk(arith):
    """B = 3109 images of 16 x 32 (7 tokens): the first chunk holds 3108 images = 21,756 token rows (so every split
    GEMM with npad % 256 == 0 runs its 256-row instance), the second one image. No max_workspace_bytes."""
    bb = backbone()
    lib = bb.lib
    H, W, cap, B = de.CHUNK_H, de.CHUNK_W, de.CHUNK_CAP, de.CHUNK_B
    assert bb.max_workspace_bytes is None
    size = int(lib.gp_dino_workspace_size(B, H, W))
    assert size == int(lib.gp_dino_workspace_size(cap, H, W)) > int(lib.gp_dino_workspace_size(cap - 1, H, W))
    xh = de.chunk_input()
    x = torch.tensor(xh).to(DEV)         # a copy: the shared input stays read-only
    try:
        full = run(x, arith, n=(2,))[0]
        assert bb._ws.numel() == size and tuple(full.shape) == (B, 2, 384)
        head, tail = run(x[:cap], arith, n=(2,))[0], run(x[cap:], arith, n=(2,))[0]
        assert torch.equal(full, torch.cat([head, tail]))
        for i in de.CHUNK_PROBES:
            assert torch.equal(run(x[i:i + 1], arith, n=(2,))[0][0], full[i]), i
    finally:
        bb._ws = None           # 0.64 GB: not kept for the rest of the session
        torch.cuda.empty_cache()
    probes = list(de.CHUNK_PROBES)
    ref = chunk_reference()
    failures = bar_failures(f"chunk probes {arith}", [full[probes]], ref, (2,))
    assert not failures, failures


_chunk_ref = []


def chunk_reference():
    if not _chunk_ref:
        _chunk_ref.append(de.yardstick(de.state_dict("plain"), de.chunk_input()[list(de.CHUNK_PROBES)], (2,)))
    return _chunk_ref[0]


# ------------------------------------------------------------------ 3. the RoPE table
@pytest.mark.parametrize("periods", ["default", "scaled"])
@pytest.mark.parametrize("hp,wp", [(1, 1), (1, 59), (60, 1), (41, 3), (32, 32)])
def test_rope_table_matches_float64(hp, wp, periods):
    """Row p of the device table = [cos h | cos w | sin h | sin w] of patch p: the host evaluates in float64 and
    rounds once, so the tolerance is one float32 rounding of a value <= 1 (2^-25) plus 1e-12 for the two float64
    evaluations of an angle of at most 2 pi."""
    from genpose2_amd import _lib
    lib = _lib.load()
    if periods == "default":
        per, per_p = None, None
    else:
        default = 100.0 ** (np.arange(16, dtype=np.float64) / 16.0)
        per = np.ascontiguousarray((default * 1.37).astype(np.float32))
        per_p = per.ctypes.data_as(ctypes.c_void_p)
    tab = torch.full((hp * wp + 4, 64), 9.0, dtype=torch.float32, device=DEV)       # 4 guard rows
    rc = lib.gp_dino_rope_table(per_p, hp, wp, ctypes.c_void_p(tab.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.gp_last_error()
    cos, sin = dino_ref.rope_cos_sin(hp, wp, None if per is None else torch.from_numpy(per.astype(np.float64)),
                                     torch.float64)
    want = torch.cat([cos[:, :32], sin[:, :32]], dim=1)
    got = tab.cpu().double()
    assert bool((got[hp * wp:] == 9.0).all())
    err = float((got[:hp * wp] - want).abs().max())
    print(f"rope table {hp} x {wp} {periods}: max |device - float64| {err:.3e}")
    assert err <= 2.0 ** -25 + 1e-12
    if hp == 1:
        assert bool((got[:wp, :16] == 1).all()) and bool((got[:wp, 32:48] == 0).all())     # h coordinate 0
    if wp == 1:
        assert bool((got[:hp, 16:32] == 1).all()) and bool((got[:hp, 48:] == 0).all())     # w coordinate 0
