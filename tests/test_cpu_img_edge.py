"""The image encoder's edge cases without a device (tests/golden/img_edge_inputs.py): the case table names the tile,
wave and chunk boundaries it says it does, the float32 yardstick of every case is positive and small, "sharp" is
sharp, the float64 restatement (tests/img_ref.py) shows that the cases can see the mistakes they are there for, and
the gather restatement is the oracle's. No HIP compute calls."""
import numpy as np
import pytest

import img_edge_inputs as ie
import img_ref
from oracle import oracle

MIN_MULTIPLE = 100.0
EPS_MAX, EPS_MAX_SHARP = 2.5e-6, 5e-5      # 4 eps stays inside the existing image tests' 1e-5
# the case meant for each mistake: partial tiles / a softmax tail (g12, g20), clamped table indices in numbers (g20),
# a second edge chunk (chunk); the rest show on the smallest grid
VARIANT_CASES = (("table_transposed", "g12"), ("g_first_channels", "g4"), ("softmax_tail_dropped", "g12"),
                 ("softmax_tail_dropped", "g20"), ("conv_wrap", "g4"), ("im2col_row_wrap", "g12"), ("edge_div4", "g4"),
                 ("chunk_edge_offset", "chunk"), ("chunk_edge_offset", "chunk2"), ("index_wrap", "g20"))


def test_case_table_names_the_edges():
    assert set(ie.PROPERTIES) == set(ie.CASES) and set(ie.CHUNK_PROBES) <= set(ie.CASES)
    assert (ie.IE_EDGE_CHUNK, ie.GEMM_TILE, ie.WAVE) == (256, 64, 64)
    for name, (b, g, d, scale) in ie.CASES.items():
        assert ie.case_properties(name) == ie.PROPERTIES[name], (name, ie.case_properties(name))
        assert (g * g) % 16 == 0 and d % 64 == 0 and b >= 1 and 0 < scale <= 1, name     # what the C entry accepts
    p = ie.PROPERTIES
    # narrower than a wave and than a tile, one k-group, one output tile of the conv, d < 256
    assert (p["g4"]["np"], p["g4"]["kgroups"], p["g4"]["co"], p["g4"]["tiles"]) == (16, 1, 16, 1)
    assert ie.CASES["g4"][2] < 256
    # exactly one wave and one tile
    assert (p["g8"]["np"], p["g8"]["tile_rem"], p["g8"]["wave_rem"], p["g8"]["tiles"]) == (64, 0, 0, 1)
    # 144 = 2 * 64 + 16 and 400 = 6 * 64 + 16: a partial tile row and column, a 16-key softmax tail, and a partial
    # 32-wide transpose tile (144 = 4 * 32 + 16, 400 = 12 * 32 + 16)
    for name in ("g12", "g12_wide", "g20", "sharp"):
        assert p[name]["tile_rem"] == 16 and p[name]["wave_rem"] == 16 and p[name]["np"] % 32 == 16, name
    assert (p["g12"]["tiles"], p["g20"]["tiles"]) == (3, 7) and p["g20"]["np"] > 256
    assert ie.CASES["g12_wide"][0] == 1 and ie.CASES["g12_wide"][2] == 384 and p["g12_wide"]["d_mod256"] == 128
    # g20's embedding table has 1444 rows for 39^2 = 1521 indices
    e = ie.case_state_dict("g20")["img_encoder.rel_pos_emb.weight"]
    assert e.shape == (1444, 16) and 39 * 39 == 1521
    raw = img_ref.table_index(20, 1 << 30)
    assert raw.max() == 1520 and int((raw > 1443).sum()) == p["g20"]["clamped"] == 1198 and raw.min() == 0
    for name, (_, g, _, _) in ie.CASES.items():     # the restatement clamps exactly those entries, on every grid
        rows = (2 * (g - 1)) ** 2
        assert int((img_ref.table_index(g, rows) != img_ref.table_index(g, 1 << 30)).sum()) == p[name]["clamped"] > 0
    # one object past a chunk; two chunks and one object
    assert (p["chunk"]["chunks"], p["chunk"]["last_chunk"], ie.CASES["chunk"][0]) == (2, 1, 257)
    assert (p["chunk2"]["chunks"], p["chunk2"]["last_chunk"], ie.CASES["chunk2"][0]) == (3, 1, 513)
    assert ie.CHUNK_PROBES == {"chunk": (255, 256), "chunk2": (255, 256, 511, 512)}
    assert all(p[n]["chunks"] == 1 for n in ie.CASES if n not in ie.CHUNK_PROBES)
    # sharp is g12 at another scale and seed: the same weights
    assert ie.CASES["sharp"][1:3] == ie.CASES["g12"][1:3] and ie.case_state_dict("sharp") is ie.case_state_dict("g12")


def test_weights_have_the_reference_shapes():
    for d, g in ((64, 4), (128, 8), (384, 12), (64, 20)):
        sd = ie.state_dict(d, g, ie.WEIGHT_SEED)
        shapes = {k[len("img_encoder."):]: v.shape for k, v in sd.items()}
        assert shapes == {"layer_attn.0.weight": (d // 2, d), "layer_attn.0.bias": (d // 2,),
                          "layer_attn.2.weight": (1, d // 2), "layer_attn.2.bias": (1,),
                          "rel_pos_emb.weight": ((2 * (g - 1)) ** 2, d // 4), "edge_guide.0.weight": (d // 4, d, 3, 3),
                          "edge_guide.0.bias": (d // 4,), "geo_weight": (), "edge_weight": ()}
        assert all(v.dtype == np.float32 for v in sd.values())
        assert float(sd["img_encoder.geo_weight"]) > 0 and float(sd["img_encoder.edge_weight"]) > 0
        bias = sd["img_encoder.edge_guide.0.bias"]
        assert bias.min() < 0 < bias.max()                # relu(conv bias) is no identity (zero_obj)
        centre = sd["img_encoder.rel_pos_emb.weight"][2 * g * (g - 1)].astype(np.float64).sum()
        assert abs(centre - ie.CENTRE_SUM) < 1e-5
        assert img_ref.table_index(g, (2 * (g - 1)) ** 2)[5, 5] == 2 * g * (g - 1)
    assert ie.state_dict(64, 4, ie.WEIGHT_SEED, emb_rows=49)["img_encoder.rel_pos_emb.weight"].shape == (49, 16)
    a, b = ie.state_dict(64, 4, 1), ie.state_dict(64, 4, 2)
    assert not np.array_equal(a["img_encoder.layer_attn.0.weight"], b["img_encoder.layer_attn.0.weight"])
    assert np.array_equal(a["img_encoder.edge_guide.0.weight"], ie._state_dict(64, 4, 1)["img_encoder.edge_guide.0.weight"])


def test_inputs_are_seeded_and_distinct():
    seen = []
    for name, (b, g, d, scale) in ie.CASES.items():
        ls = ie.layers(name)
        assert len(ls) == 3 and all(v.shape == (b, g * g, d) and v.dtype == np.float32 for v in ls), name
        assert all(np.array_equal(x, y) for x, y in zip(ls, ie.raw_layers(name))) or name in ("zero_obj", "same_layers")
        first = ls[0].reshape(-1)[:64]
        assert not any(np.array_equal(first, s) for s in seen), name
        seen.append(first)
        assert 3.0 * scale < np.abs(ls[0]).max() < 6.0 * scale, name
    z = ie.layers("zero_obj")
    assert all(np.all(v[1] == 0) and np.all(np.abs(v[0]).max() > 0) and np.abs(v[2]).max() > 0 for v in z)
    s = ie.layers("same_layers")
    assert s[0] is s[1] is s[2]
    g = ie.layers("g4")
    assert not np.array_equal(g[0], g[1]) and not np.array_equal(g[1], g[2])


@pytest.mark.parametrize("name", list(ie.CASES))
def test_yardstick_is_positive_and_small(name):
    """eps(case, output): oracle.img_encoder_forward (fp32 torch, CPU) against the float64 restatement, relative to
    max |ref| of the output. Measured: 6e-8 .. 3.7e-7 on every case but sharp (final 5.3e-7, layer_w 5.8e-7)."""
    r = ie.reference(name)
    b, g, d, _ = ie.CASES[name]
    ref = r["ref"]
    assert ref["final"].shape == (b, g * g, d) and ref["layer_w"].shape == (b, g * g, 3) and ref["edge"].shape == (b, d // 4)
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in ref.values())
    print(f"img edge case {name}: eps {r['eps']}, max |final| {np.abs(ref['final']).max():.2f}, mean row max of the "
          f"attention {ref['attn_max'].mean():.3f}")
    for k in ie.OUTPUTS:
        assert 0 < r["eps"][k] <= (EPS_MAX_SHARP if name == "sharp" else EPS_MAX), (name, k, r["eps"][k])
    assert np.allclose(ref["layer_w"].sum(-1), 1.0, atol=1e-14)
    if name == "same_layers":
        assert np.abs(ref["layer_w"] - 1.0 / 3.0).max() < 1e-15
    if name == "zero_obj":
        sd = ie.case_state_dict(name)
        assert np.all(ref["final"][1] == 0)
        assert np.array_equal(ref["edge"][1], np.maximum(sd["img_encoder.edge_guide.0.bias"].astype(np.float64), 0))


def test_sharp_is_sharp_and_g12_is_not():
    """Float64, the mean over rows of the largest attention probability: >= 0.9 for sharp, <= 0.5 for g12 (the same
    weights at 0.3 of the input scale). Measured 1.000 and 0.342."""
    sharp, plain = ie.reference("sharp")["ref"]["attn_max"], ie.reference("g12")["ref"]["attn_max"]
    print(f"mean row max of the geometric attention: sharp {sharp.mean():.4f}, g12 {plain.mean():.4f}")
    assert sharp.mean() >= 0.9
    assert plain.mean() <= 0.5


@pytest.mark.parametrize("variant,name", VARIANT_CASES)
def test_cases_see_the_mistakes(variant, name):
    """Each variant of img_ref moves the float64 final features or edge weights of the case meant for it by at least
    100 eps. Measured multiples of eps (final / edge): table_transposed g12 2e5 / 0, g_first_channels g4 5e5 / 0,
    softmax_tail_dropped g12 9e5 / 0 and g20 8e5 / 0, conv_wrap g4 1e5 / 2e6, im2col_row_wrap g12 3e4 / 5e5,
    edge_div4 g4 3e5 / 0, chunk_edge_offset chunk 9e4 / 1e6, index_wrap g20 4e3 / 0."""
    r = ie.reference(name)
    out = img_ref.img_encoder_forward64(ie.case_state_dict(name), ie.layers(name), ie.CASES[name][1], variant=variant)
    moved = {k: ie.rel(out[k], r["ref"][k]) / r["eps"][k] for k in ("final", "edge")}
    print(f"img edge case {name} variant {variant}: moves final by {moved['final']:.0f} eps, edge by {moved['edge']:.0f} eps")
    assert max(moved.values()) >= MIN_MULTIPLE, moved
    if name in ie.CHUNK_PROBES:         # the first chunk is untouched: only a per-object look at the second sees it
        assert np.array_equal(out["final"][:256], r["ref"]["final"][:256])
        assert ie.rel(out["final"][256], r["ref"]["final"][256]) >= MIN_MULTIPLE * r["eps"]["final"]


def test_identity_variants_are_identities():
    """Where a variant cannot change anything: no softmax tail at np <= 64, no second chunk at B <= 256."""
    for name, variant in (("g4", "softmax_tail_dropped"), ("g8", "softmax_tail_dropped"), ("g12", "chunk_edge_offset")):
        out = img_ref.img_encoder_forward64(ie.case_state_dict(name), ie.layers(name), ie.CASES[name][1], variant=variant)
        assert np.array_equal(out["final"], ie.reference(name)["ref"]["final"]), (name, variant)


def test_geo_table_restatement():
    """geo_table64 indexes as oracle.img_geo_bias and as genpose2_amd.img_encoder.geo_table (float32 row sums)."""
    from genpose2_amd import img_encoder
    for d, g, rows in ((64, 4, None), (64, 20, None), (128, 8, (2 * 8 - 1) ** 2), (64, 12, 1)):
        sd = {k: np.array(v) for k, v in ie.state_dict(d, g, ie.WEIGHT_SEED, rows).items()}    # writable copies
        t64 = img_ref.geo_table64(sd["img_encoder.rel_pos_emb.weight"], g)
        assert t64.shape == (g * g, g * g) and t64.dtype == np.float64
        for t32 in (oracle.img_geo_bias(sd, grid=g), img_encoder.geo_table(sd, grid=g)):
            assert t32.dtype == np.float32 and np.abs(t32 - t64).max() < 2e-6
        if rows is None:
            assert abs(t64[3, 3] - ie.CENTRE_SUM) < 1e-5 and not np.allclose(t64, t64.T)


def test_gather_cases_and_restatement():
    ds, ns, grids, patches = set(), set(), set(), set()
    seen = set()
    for i, (b, n_p, grid, patch, d, n) in enumerate(ie.GATHER_CASES):
        ds.add(d), ns.add(n), grids.add((n_p, grid)), patches.add(patch)
        feat, xs, ys = ie.gather_inputs(i)
        assert feat.shape == (b, n_p, d) and xs.shape == ys.shape == (b, n) and xs.dtype == ys.dtype == np.int32
        for v in (xs, ys):
            assert -3 * patch <= v.min() and v.max() < (grid + 3) * patch
        pairs = set(zip(xs.reshape(-1).tolist(), ys.reshape(-1).tolist()))
        sp = set(ie.gather_specials(grid, patch))
        if b * n >= len(sp):
            assert sp <= pairs, i
            vals = set(xs.reshape(-1).tolist()) | set(ys.reshape(-1).tolist())
            assert {-1, -patch, -patch - 1} <= vals
        seen |= {s for s in range(len(ie.gather_specials(grid, patch))) if ie.gather_specials(grid, patch)[s] in pairs}
        got = img_ref.gather_ref(feat, xs, ys, patch, grid)
        assert got.shape == (b, n, d)
        if patch == 14 and grid == 16:
            assert np.array_equal(got, oracle.gather_patch_points(feat, xs, ys))
        # an in-range xs with ys = -1 is the previous row's last patch (one clamp of the combined index)
        one = img_ref.gather_ref(feat[:1], np.array([[2 * patch]]), np.array([[-1]]), patch, grid)
        assert np.array_equal(one[0, 0], feat[0, min(2 * grid - 1, n_p - 1)])
        one = img_ref.gather_ref(feat[:1], np.array([[-1]]), np.array([[grid * patch]]), patch, grid)
        assert np.array_equal(one[0, 0], feat[0, 0])                 # -grid + grid = 0: floor, not truncation
    assert ds == {4, 64, 260, 384, 1024} and ns == {1, 3, 4, 5, 1023} and patches == {1, 14, 16}
    assert grids == {(16, 4), (256, 16), (400, 20), (100, 16)}
    assert seen == set(range(13))       # every special pair is run by some case
