"""The DINOv3 backbone's edge cases without a device (tests/golden/dino_edge_inputs.py): the case table names the
tile boundaries it says it does, the float32 yardstick of every case is positive, and the float64 restatement
(tests/dino_ref.py) shows that the cases can see the mistakes they are there for. No HIP compute calls."""
import numpy as np
import pytest
import torch

import dino_edge_inputs as de
import dino_ref

# the cases the variant check runs on: a key chunk of 1 with Hp > Wp, a third chunk of 1, fixture (a) transposed
VARIANT_CASES = ("strip_h", "n129", "tall")
MIN_MULTIPLE = 100.0


def test_case_table_names_the_edges():
    assert set(de.PROPERTIES) == set(de.CASES)
    for name, (b, h, w, _, layers, _, _) in de.CASES.items():
        assert h % 16 == 0 and w % 16 == 0, name
        hp, wp = h // 16, w // 16
        want = de.PROPERTIES[name]
        got = dict(n=hp * wp + 5, n_mod64=(hp * wp + 5) % 64, m=b * hp * wp, m_mod64=(b * hp * wp) % 64, tall=hp > wp)
        assert got == want, (name, got)
        assert hp * wp <= 1024
        if name != "max":
            assert b * hp * wp * 384 >= de.MIN_VALUES and layers == (0, 2, 11), name
    p = de.PROPERTIES
    # attention: no tail at 64 and 128 tokens; a chunk and a query tile of one row at 65 and 129; a 5-row tail at
    # the limit
    assert (p["strip_w"]["n"], p["n128"]["n"]) == (64, 128)
    assert (p["strip_h"]["n"], p["n129"]["n"], p["max"]["n"]) == (65, 129, 1029) and p["one_patch"]["n"] == 6
    assert (-p["strip_h"]["n"]) % 16 == 15 and (-p["n129"]["n"]) % 16 == 15        # 15 masked pad keys
    # patch embedding: fewer rows than a block, one more than two blocks, whole blocks; m64's B = 4 is one block
    assert p["m129"]["m"] == 2 * 64 + 1 and p["max"]["m"] % 64 == 0 and 4 * 16 == 64 and p["m64"]["m"] == 80
    assert p["strip_h"]["tall"] and p["tall"]["tall"] and de.CASES["strip_h"][2] == 16
    assert de.CASES["max"][4] == (0, 2) and 1 * 1024 * 384 == 393216
    # part 2: one image more than a natural chunk
    assert de.CHUNK_N == (de.CHUNK_H // 16) * (de.CHUNK_W // 16) + 5 == 7
    assert de.CHUNK_CAP == 3108 and de.CHUNK_B == 3109 and de.CHUNK_CAP * de.CHUNK_N == 21756 > 10752


def test_inputs_are_what_the_table_says():
    x = de.case_input("n129")
    assert x.dtype == np.float32 and x.shape == (2, 3, 64, 496) and -2.1 <= x.min() < -2.0 and 2.5 < x.max() <= 2.6
    assert np.array_equal(de.case_input("n129"), x)                                   # seeded
    assert not np.array_equal(de.case_input("n128")[:, :, :48, :496], x[:, :, :48])   # a seed per case
    assert np.all(de.case_input("n129_const") == np.float32(0.7))
    assert np.array_equal(de.case_input("n129_big"), x * np.float32(100.0))
    assert np.array_equal(de.case_input("n129_sharp"), x)
    plain, sharp = de.state_dict("plain"), de.state_dict("sharp")
    assert set(plain) == set(sharp)
    changed = [k for k in plain if not np.array_equal(plain[k], sharp[k])]
    assert sorted(changed) == sorted(f"blocks.{i}.attn.qkv.{t}" for i in range(12) for t in ("weight", "bias"))
    for k in changed:
        assert np.array_equal(sharp[k][:384], plain[k][:384] * np.float32(6.0))
        assert np.array_equal(sharp[k][384:], plain[k][384:])


@pytest.mark.parametrize("name", list(de.CASES))
def test_yardstick_is_positive(name):
    ref = de.reference(name)
    b, h, w, _, layers, _, _ = de.CASES[name]
    assert ref["stats32"].shape == (len(layers), 3)
    for r in ref["ref64"]:
        assert r.shape == (b, (h // 16) * (w // 16), 384) and r.dtype == np.float64 and np.all(np.isfinite(r))
    print(f"dino edge case {name}: |ref| <= {max(np.abs(r).max() for r in ref['ref64']):.2f}, fp32 run error "
          f"[max p99.9 mean] per layer {ref['stats32'].tolist()}")
    assert np.all(ref["stats32"] > 0)
    assert np.all(ref["stats32"][:, 0] < 1e-4)          # a float32 run, not a different model


def _identity(name, variant):
    """The combinations in which a variant cannot change anything."""
    _, h, w, *_ = de.CASES[name]
    hp, wp = h // 16, w // 16
    if variant == "zero_key_tail":
        return (hp * wp + 5) % 16 == 0
    return variant == "swap_hw" and hp == wp == 1   # one patch: both coordinates are 0. (On a square or a 1-wide grid
    # the swap is no identity: patch (i, j) gets the angles of (j, i), and the h angles move to the w dims.)


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_cases_see_the_mistakes(name):
    """Each switched-off variant of dino_ref moves the float64 output of layer 2 by at least 100 x the float32 run's
    max error (the largest over the case's layers). Measured multiples (this CPU): DESIGN.md "DINOv3 backbone off
    the fixture shapes"."""
    ref = de.reference(name)
    emax = float(ref["stats32"][:, 0].max())
    i2 = de.CASES[name][4].index(2)
    sd, x = de.state_dict(de.CASES[name][6]), de.case_input(name)
    low = []
    with torch.no_grad():
        for v in dino_ref.VARIANTS:
            out = dino_ref.forward(sd, x, (2,), torch.float64, variant=v)[0].numpy()
            moved = float(np.abs(out - ref["ref64"][i2]).max())
            if _identity(name, v):
                assert moved == 0.0, (name, v)
                continue
            print(f"dino edge case {name} variant {v}: moves layer 2 by {moved:.3e} = {moved / emax:.0f} x the fp32 "
                  f"run's max error {emax:.2e}")
            if not moved >= MIN_MULTIPLE * emax:
                low.append((v, moved / emax))
    assert not low, low


def test_identity_variants_are_identities():
    """swap_hw on a single patch and zero_key_tail at n % 16 == 0 change nothing (the exemptions of the check above);
    on a 1-wide or a square grid swap_hw is NOT the identity."""
    sd = de.state_dict("plain")
    with torch.no_grad():
        x = de.case_input("one_patch")[:2]          # 1 x 1 patches
        a = dino_ref.forward(sd, x, (0,), torch.float64)[0]
        assert torch.equal(dino_ref.forward(sd, x, (0,), torch.float64, variant="swap_hw")[0], a)
        assert not torch.equal(dino_ref.forward(sd, x, (0,), torch.float64, variant="zero_key_tail")[0], a)
        x = de.case_input("m64")[:1]                # 4 x 4 patches
        a = dino_ref.forward(sd, x, (0,), torch.float64)[0]
        assert not torch.equal(dino_ref.forward(sd, x, (0,), torch.float64, variant="swap_hw")[0], a)
        x = de.case_input("strip_w")[:1]            # 64 tokens
        a = dino_ref.forward(sd, x, (0,), torch.float64)[0]
        assert torch.equal(dino_ref.forward(sd, x, (0,), torch.float64, variant="zero_key_tail")[0], a)
        assert not torch.equal(dino_ref.forward(sd, x, (0,), torch.float64, variant="swap_hw")[0], a)


def test_rope_restatement_layout():
    """rope_cos_sin's columns are [h(16) | w(16)] tiled twice, so [cos[:, :32] | sin[:, :32]] is the device table's
    [cos h | cos w | sin h | sin w]; a single row or column sits at coordinate 0 (angle 0)."""
    cos, sin = dino_ref.rope_cos_sin(60, 1, None, torch.float64)
    assert torch.equal(cos[:, :32], cos[:, 32:]) and torch.equal(sin[:, :32], sin[:, 32:])
    assert torch.all(cos[:, 16:32] == 1) and torch.all(sin[:, 16:32] == 0)           # wp = 1: the w angles are 0
    assert float(sin[:, :16].abs().max()) > 0.5
    ch = 2.0 * (torch.arange(60, dtype=torch.float64) + 0.5) / 60 - 1.0
    assert torch.allclose(cos[:, 0], torch.cos(2 * np.pi * ch), atol=1e-14, rtol=0)   # period 0 is 1
    cos, sin = dino_ref.rope_cos_sin(1, 1, None, torch.float64)
    assert torch.all(cos == 1) and torch.all(sin == 0)
