"""The --dino pointwise image branch on the device off its one shape (tests/golden/img_edge_inputs.py): gp_img_encoder2 /
gp_img_encoder3 through the C ABI at grids of 4 .. 20 and widths of 64 .. 384, across the edge chunk of 256 objects,
with guard bands round every output and an exactly sized workspace; gp_gather_patch_points bit for bit; the host's
gp_img_geo_table. The references are tests/img_ref.py in float64 on the CPU, computed once per case and shared by the
four forms; the bar of the exact-fp32 forms is 4 x the float32 CPU oracle's own error (never a device figure), that of
the split-f16 forms the 1e-5 test_img_encoder_vs_reference_golden holds both arithmetics to."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import img_edge_inputs as ie
import img_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
FILL = 0xA5
MARGIN = 4.0             # the MFMA kernels sum in another order and chunking than torch's CPU GEMM
SPLIT_BOUND = 1e-5
FORMS_AGREE = 2e-6       # test_img_encoder_implicit_im2col_vs_column_buffer's figure
# form -> (entry, split-f16 planes given)
FORMS = {"split2": ("gp_img_encoder2", True), "split3": ("gp_img_encoder3", True),
         "f32_2": ("gp_img_encoder2", False), "f32_3": ("gp_img_encoder3", False)}


def lib():
    from genpose2_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def packed(d, grid):
    """The device buffers of the C entry for the (d, grid) state dict, packed here: the fp32 weights as stored, the
    position table, the split-f16 planes channel-major and position-major (as pack_img_encoder forms them)."""
    from genpose2_amd import img_encoder
    from genpose2_amd.fus_encoder import pack_split_linear
    sd = {k: np.array(v) for k, v in ie.state_dict(d, grid, ie.WEIGHT_SEED).items()}    # writable copies
    g = lambda k: np.ascontiguousarray(sd[f"img_encoder.{k}"], dtype=np.float32)  # noqa: E731
    conv = g("edge_guide.0.weight")
    host = {"la_w1": g("layer_attn.0.weight"), "la_b1": g("layer_attn.0.bias"),
            "la_w2": g("layer_attn.2.weight").reshape(-1), "geo_table": img_encoder.geo_table(sd, grid=grid),
            "conv_w": conv, "conv_b": g("edge_guide.0.bias"), "la_w1_h": pack_split_linear(g("layer_attn.0.weight")),
            "conv_w_h": pack_split_linear(conv.reshape(conv.shape[0], -1)),
            "conv_w_hp": pack_split_linear(np.ascontiguousarray(conv.transpose(0, 2, 3, 1)).reshape(conv.shape[0], -1))}
    assert host["geo_table"].shape == (grid * grid, grid * grid)
    t = {k: torch.tensor(v).to(DEV) for k, v in host.items()}
    t["scalars"] = tuple(float(v) for v in img_encoder.pack_img_scalars(sd))
    return t


def workspace_bytes(form, B, n, d):
    entry, split = FORMS[form]
    if entry == "gp_img_encoder2":
        return int(lib().gp_img_encoder_workspace_size(B, n, d))
    return int(lib().gp_img_encoder3_workspace_size(B, n, d, int(split)))


class Arena:
    """out, layer_w, edge and the workspace as slices of one buffer, 4 KB guard bands before, between and after them
    (every slice starts 256-byte aligned; its round-up belongs to the guard). Outputs start as NaN, the workspace as
    0xFF bytes (NaN too: an element read before it is written would show in the outputs), guards as 0xA5."""

    def __init__(self, sizes):
        self.spans, off = {}, GUARD
        for k, nbytes in sizes.items():
            self.spans[k] = (off, off + nbytes)
            off = (off + nbytes + 255) // 256 * 256 + GUARD
        self.buf = torch.full((off,), FILL, dtype=torch.uint8, device=DEV)
        for k, (a, b) in self.spans.items():
            self.buf[a:b] = 0xFF
        self.start = self.buf.clone()

    def ptr(self, k):
        return self.buf.data_ptr() + self.spans[k][0]

    def floats(self, k, shape):
        a, b = self.spans[k]
        return self.buf[a:b].view(torch.float32).view(shape).cpu().numpy()

    def guards_intact(self):
        edges = [0] + [v for a, b in self.spans.values() for v in (a, b)] + [self.buf.numel()]
        return all(bool((self.buf[edges[i]:edges[i + 1]] == FILL).all()) for i in range(0, len(edges), 2))

    def untouched(self):
        return bool(torch.equal(self.buf, self.start))


def call_encoder(form, pk, ls, B, n, d, ws_bytes=None, lw=True, edge=True, arena_shape=None):
    """One call of the form's entry over device layers ls -> (rc, arena). arena_shape: (B, n, d) the buffers are sized
    for when the call's own shape is one the entry refuses."""
    entry, split = FORMS[form]
    aB, an, ad = arena_shape or (B, n, d)
    need = workspace_bytes(form, aB, an, ad)
    ar = Arena({"out": 4 * aB * an * ad, "layer_w": 4 * aB * an * 3, "edge": 4 * aB * (ad // 4), "ws": need})
    assert pk["la_w1"].data_ptr() % 256 == 0 and ar.buf.data_ptr() % 256 == 0
    b2, gg, eg = pk["scalars"]
    conv_h = pk["conv_w_h" if entry == "gp_img_encoder2" else "conv_w_hp"]
    rc = getattr(lib(), entry)(
        ls[0].data_ptr(), ls[1].data_ptr(), ls[2].data_ptr(), B, n, d, pk["la_w1"].data_ptr(), pk["la_b1"].data_ptr(),
        pk["la_w2"].data_ptr(), b2, pk["geo_table"].data_ptr(), pk["conv_w"].data_ptr(), pk["conv_b"].data_ptr(), gg, eg,
        pk["la_w1_h"].data_ptr() if split else None, conv_h.data_ptr() if split else None, ar.ptr("out"),
        ar.ptr("layer_w") if lw else None, ar.ptr("edge") if edge else None, ar.ptr("ws"),
        need if ws_bytes is None else ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ar


def run_form(form, name, ls=None, objects=None):
    """The case through one form -> {"final", "layer_w", "edge"} (numpy). objects: a slice of the batch to run."""
    _, g, d, _ = ie.CASES[name]
    hs = ie.layers(name) if ls is None else ls
    if objects is not None:
        hs = [v[objects] for v in hs]
    B, n = hs[0].shape[0], g * g
    dev = [torch.tensor(v).to(DEV) for v in hs]
    rc, ar = call_encoder(form, packed(d, g), dev, B, n, d)
    assert rc == 0, (name, form, lib().gp_last_error())
    assert ar.guards_intact(), (name, form, "a guard band changed")
    got = {"final": ar.floats("out", (B, n, d)), "layer_w": ar.floats("layer_w", (B, n, 3)),
           "edge": ar.floats("edge", (B, d // 4))}
    for k, v in got.items():
        assert np.all(np.isfinite(v)), (name, form, k, "not every element was written")
    return got


def bound(name, form, k):
    eps = ie.reference(name)["eps"][k]
    if not FORMS[form][1]:
        return MARGIN * eps
    return max(SPLIT_BOUND, MARGIN * eps) if name == "sharp" else SPLIT_BOUND


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in ie.OUTPUTS)


# ------------------------------------------------------------------ 1. the whole encoder, four forms per case
@pytest.mark.parametrize("name", list(ie.CASES))
def test_encoder_matches_float64_at_the_edges(name):
    """Measured on MI355X, err / eps (eps = the fp32 CPU oracle's error against float64; range over the ten cases):

        form     final        layer_w      edge
        split2   0.63 - 1.66  0.60 - 1.00  0.33 - 1.77
        split3   0.63 - 1.66  0.60 - 1.00  0.47 - 1.37
        f32_2    0.74 - 2.14  0.68 - 1.37  0.42 - 1.37
        f32_3    the bits of f32_2

    (largest: g12_wide final 2.14; the split forms' largest error is 4.2e-7 against their 1e-5.) The chunk-boundary
    objects on their own: at most 0.77; their B = 2 re-run is bitwise equal in every form and output; split3 against
    split2 at most 2.4e-7. Before imgenc_pool_kernel summed in 16 partial sums the edge weights stood at 4.33 (g12)
    and 6.22 (g20) in the exact forms: one running fp32 sum over np pixels. The same_layers and zero_obj invariants
    are held to 4 eps in all four forms (measured 1.00 eps and 0). Per case and form: DESIGN.md "Image encoder off
    its one shape"."""
    r = ie.reference(name)
    ref, eps = r["ref"], r["eps"]
    B = ie.CASES[name][0]
    got, failures = {}, []
    for form in FORMS:
        got[form] = run_form(form, name)
        for k in ie.OUTPUTS:
            err = ie.rel(got[form][k], ref[k])
            print(f"img edge {name} {form} {k}: err {err:.3e}  eps {eps[k]:.3e}  err/eps {err / eps[k]:.2f}  "
                  f"bound {bound(name, form, k):.3e}")
            if not err <= bound(name, form, k):
                failures.append((form, k, err, bound(name, form, k)))
    # between the forms: NULL planes run the same kernels through either entry; with planes the implicit im2col sums
    # the same products in another order
    if not same_bits(got["f32_2"], got["f32_3"]):
        failures.append("exact fp32: entries 2 and 3 differ in bits")
    for k in ie.OUTPUTS:
        e = ie.rel(got["split3"][k], got["split2"][k])
        print(f"img edge {name} split3 vs split2 {k}: {e:.3e}")
        if not e <= FORMS_AGREE:
            failures.append(("split3 vs split2", k, e))
    for form in FORMS:
        g, peak = got[form], {k: float(np.abs(ref[k]).max()) for k in ie.OUTPUTS}
        if name == "same_layers":
            e = float(np.abs(g["layer_w"].astype(np.float64) - 1.0 / 3.0).max()) / peak["layer_w"]
            print(f"img edge {name} {form}: |layer_w - 1/3| / max {e:.3e}")
            if not e <= MARGIN * eps["layer_w"]:          # every form: three equal rows give softmax(1, 1, 1)
                failures.append((form, "layer_w != 1/3", e, MARGIN * eps["layer_w"]))
        if name == "zero_obj":
            sd = ie.case_state_dict(name)
            if not np.all(g["final"][1] == 0):
                failures.append((form, "the zero object's rows are not 0"))
            want = np.maximum(sd["img_encoder.edge_guide.0.bias"].astype(np.float64), 0.0)
            e = float(np.abs(g["edge"][1] - want).max()) / peak["edge"]
            print(f"img edge {name} {form}: |edge[1] - relu(conv bias)| / max {e:.3e}")
            if not e <= MARGIN * eps["edge"]:             # every form: a zero im2col row leaves the bias
                failures.append((form, "edge[1] != relu(bias)", e, MARGIN * eps["edge"]))
            full = run_form(form, name, ls=ie.raw_layers(name))        # object 1 not zeroed
            if np.all(full["final"][1] == 0) or not all(
                    np.array_equal(full[k][[0, 2]].view(np.int32), g[k][[0, 2]].view(np.int32)) for k in ie.OUTPUTS):
                failures.append((form, "the zero object's neighbours changed"))
        if name in ie.CHUNK_PROBES:
            for i in ie.CHUNK_PROBES[name]:     # on their own: a wrong chunk offset cannot hide in a maximum over B
                for k in ie.OUTPUTS:
                    e = float(np.abs(g[k][i] - ref[k][i]).max()) / peak[k]
                    print(f"img edge {name} {form} object {i} {k}: err/eps {e / eps[k]:.2f}")
                    if not e <= bound(name, form, k):
                        failures.append((form, "object", i, k, e, bound(name, form, k)))
            # the last two objects (the one that closes a chunk, the one alone in the next) again as a B = 2 call
            pair = run_form(form, name, objects=slice(B - 2, B))
            equal = {k: bool(np.array_equal(pair[k].view(np.int32), g[k][B - 2:].view(np.int32))) for k in ie.OUTPUTS}
            print(f"img edge {name} {form}: B = 2 re-run of objects {B - 2}, {B - 1} bitwise equal: {equal}")
            if not all(equal.values()):
                failures.append((form, "re-run of the last two objects differs in bits", equal))
    assert not failures, failures


def test_optional_outputs_do_not_change_the_features():
    """g12: layer_w = NULL and edge_out = NULL (the edge weights then live in the workspace) give the same bits."""
    _, g, d, _ = ie.CASES["g12"]
    hs = ie.layers("g12")
    dev = [torch.tensor(v).to(DEV) for v in hs]
    B, n = hs[0].shape[0], g * g
    for form in FORMS:
        want = run_form(form, "g12")["final"]
        rc, ar = call_encoder(form, packed(d, g), dev, B, n, d, lw=False, edge=False)
        assert rc == 0 and ar.guards_intact(), (form, lib().gp_last_error())
        for k in ("layer_w", "edge"):
            a, b = ar.spans[k]
            assert bool((ar.buf[a:b] == 0xFF).all()), (form, k)
        assert np.array_equal(ar.floats("out", (B, n, d)).view(np.int32), want.view(np.int32)), form


def test_refused_shapes_launch_nothing():
    """np = 32 (no square), np = 36 (square, not a multiple of 16), d = 96, a workspace one byte short for either
    entry: an error code, and every byte of the outputs, the workspace and the guards as it was. B = 0 is no error
    and writes nothing."""
    _, g, d, _ = ie.CASES["g8"]
    dev = [torch.tensor(v).to(DEV) for v in ie.layers("g8")]
    B, n = 2, g * g
    pk = packed(d, g)
    for form in FORMS:
        for shape, msg in (((B, 32, d), b"square"), ((B, 36, d), b"square"), ((B, n, 96), b"multiple of 64")):
            rc, ar = call_encoder(form, pk, dev, *shape, arena_shape=(B, n, d))
            assert rc != 0 and msg in lib().gp_last_error(), (form, shape, lib().gp_last_error())
            assert ar.untouched(), (form, shape)
        need = workspace_bytes(form, B, n, d)
        rc, ar = call_encoder(form, pk, dev, B, n, d, ws_bytes=need - 1)
        assert rc != 0 and b"workspace too small" in lib().gp_last_error(), (form, lib().gp_last_error())
        assert ar.untouched(), form
        rc, ar = call_encoder(form, pk, dev, 0, n, d, arena_shape=(B, n, d))
        assert rc == 0 and ar.untouched(), form
        rc, ar = call_encoder(form, pk, dev, B, n, d)          # the same buffers at the exact size: accepted
        assert rc == 0 and ar.guards_intact() and not ar.untouched(), form


# ------------------------------------------------------------------ 2. the patch -> point gather
def call_gather(feat, xs, ys, B, n_p, d, N, patch, grid, feat_offset=0):
    ar = Arena({"out": 4 * max(xs.shape[0] * xs.shape[1] * feat.shape[2], 4)})
    rc = lib().gp_gather_patch_points(feat.data_ptr() + feat_offset, B, n_p, d, xs.data_ptr(), ys.data_ptr(), N, patch,
                                      grid, ar.ptr("out"), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ar


@pytest.mark.parametrize("i", range(len(ie.GATHER_CASES)))
def test_gather_is_bit_exact(i):
    B, n_p, grid, patch, d, N = ie.GATHER_CASES[i]
    feat, xs, ys = ie.gather_inputs(i)
    want = img_ref.gather_ref(feat, xs, ys, patch, grid)
    dev = [torch.tensor(v).to(DEV) for v in (feat, xs, ys)]
    rc, ar = call_gather(*dev, B, n_p, d, N, patch, grid)
    assert rc == 0, lib().gp_last_error()
    assert ar.guards_intact()
    assert np.array_equal(ar.floats("out", (B, N, d)).view(np.int32), want.view(np.int32))


def test_gather_refusals():
    """d = 6, a feat pointer 4 bytes off its alignment, grid = 0: refused, nothing written; B = 0 or N = 0: no error,
    nothing written."""
    B, n_p, grid, patch, d, N = ie.GATHER_CASES[1]
    dev = [torch.tensor(v).to(DEV) for v in ie.gather_inputs(1)]
    for kw, args in (({}, (B, n_p, 6, N, patch, grid)), ({"feat_offset": 4}, (B, n_p - 1, d, N, patch, grid)),
                     ({}, (B, n_p, d, N, patch, 0))):
        rc, ar = call_gather(*dev, *args, **kw)
        assert rc != 0 and b"gather_patch_points" in lib().gp_last_error(), (args, lib().gp_last_error())
        assert ar.untouched(), args
    for args in ((0, n_p, d, N, patch, grid), (B, n_p, d, 0, patch, grid)):
        rc, ar = call_gather(*dev, *args)
        assert rc == 0 and ar.untouched(), args


# ------------------------------------------------------------------ 3. the host's position table
@pytest.mark.parametrize("grid", [2, 4, 12, 16, 20])
def test_geo_table_on_the_host(grid):
    """gp_img_geo_table (host code, host pointers). An embedding whose rows are (idx, 0, 0, ..) gives the clamped
    index itself: the mapping alone. With random rows every entry is within edim 2^-24 sum |e| of the float64 row
    sum, the bound of a sequential fp32 sum (derived, not measured); img_encoder.geo_table, the table production
    uploads, meets the same bound and indexes identically."""
    from genpose2_amd import img_encoder
    n = grid * grid
    rng = np.random.Generator(np.random.PCG64(4400 + grid))
    for edim in (1, 24, 96):
        for rows in ((2 * (grid - 1)) ** 2, (2 * grid - 1) ** 2, 1):
            idx = img_ref.table_index(grid, rows)
            assert idx.min() == 0 and idx.max() == rows - 1

            def table(E):
                out = np.full(n * n + 64, 9.0, np.float32)
                rc = lib().gp_img_geo_table(E.ctypes.data, rows, edim, grid, out.ctypes.data)
                assert rc == 0, lib().gp_last_error()
                assert np.all(out[n * n:] == 9.0)
                return out[:n * n].reshape(n, n)
            E = np.zeros((rows, edim), np.float32)
            E[:, 0] = np.arange(rows)
            assert np.array_equal(table(E), idx.astype(np.float32)), (grid, edim, rows)
            assert np.array_equal(img_encoder.geo_table({"img_encoder.rel_pos_emb.weight": E}, grid=grid), table(E))
            E = rng.standard_normal((rows, edim)).astype(np.float32)
            want = img_ref.geo_table64(E, grid)
            tol = (edim * 2.0 ** -24 * np.abs(E.astype(np.float64)).sum(-1))[idx]
            for got in (table(E), img_encoder.geo_table({"img_encoder.rel_pos_emb.weight": E}, grid=grid)):
                assert got.dtype == np.float32 and got.shape == (n, n)
                assert np.all(np.abs(got - want) <= tol), (grid, edim, rows, float(np.abs(got - want).max()))
    E = np.zeros((4, 4), np.float32)
    out = np.full(16, 9.0, np.float32)
    assert lib().gp_img_geo_table(E.ctypes.data, 4, 4, 1, out.ctypes.data) != 0 and np.all(out == 9.0)   # grid < 2
