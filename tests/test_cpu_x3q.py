"""Host side of the hybrid f16 + FP8 form of the PC step's GEMMs (gp_head.h X3Q): the e4m3 encoder, the packed
plane layout, and the C++ packer's bytes."""
import numpy as np
import pytest

from genpose2_amd import pack, weights


def test_e4m3_codes_round_trip_and_ties():
    codes = np.array([c for c in range(256) if (c & 0x7f) != 0x7f and c != 0x80], np.uint8)   # no NaN, no -0
    assert np.array_equal(pack.e4m3_bits(pack.e4m3_value(codes)), codes)
    # ties go to the even code; half the smallest subnormal goes to zero; 448 is the largest value
    got = pack.e4m3_value(pack.e4m3_bits(np.array([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 255.0, 448.0, -0.40625])))
    assert got.tolist() == [16.0, 20.0, 0.0, 2.0 ** -8, 256.0, 448.0, -0.40625]


def test_q8_planes_layout_and_range():
    """Plane p of pe2_q / h1p_q is the e4m3 code of f16 plane p of W * 2^e times 2^Q8_PLANE_EXPONENTS[p], at
    [T][group][plane][half][lane][byte]; every plane stays inside e4m3's range without saturating."""
    from genpose2_amd import arch
    sd = weights.synthetic_state_dict("score")
    heads = pack.pack_heads(sd)
    p = weights.head_params(sd)
    for key, W in (("pe2_q", p["pe2_w"]), ("h1p_q", p["h1_pose"].reshape(3 * arch.HEAD_HID, arch.POSE_HID))):
        e = pack.split_exponent(W)
        n_out, k_in = W.shape
        q = heads[key].view(np.uint8).reshape(n_out // 16, k_in // 128, 3, 2, 4, 16, 16)   # [T][g][p][half][q][i][b]
        assert q.size == 3 * W.size
        # -> [p][T][i][g][half][b][q] with k = 128 g + 8-byte chunk cc, element j: byte 16 half + b = 8 cc + j
        full = q.transpose(2, 0, 5, 1, 3, 6, 4).reshape(3, n_out // 16, 16, k_in // 128, 4, 2, 4, 4)   # [..][cc][h16][j4][q]
        full = full.transpose(0, 1, 2, 3, 4, 5, 7, 6).reshape(3, n_out, k_in)                          # k = ..16 h16 + 4 q + j4
        r = (W.astype(np.float32) * np.float32(2.0 ** e)).astype(np.float32)
        for pl, ex in enumerate(pack.Q8_PLANE_EXPONENTS):
            h = r.astype(np.float16)
            v = h.astype(np.float64) * 2.0 ** ex
            assert np.abs(v).max() <= 256.0, (key, pl)
            assert np.array_equal(full[pl], pack.e4m3_bits(v)), (key, pl)
            r = (r - h.astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("kind,kind_id", [("score", 0), ("energy", 1)])
def test_weights_pack_host_appends_q8_planes(kind, kind_id):
    """The C++ packer appends pack.py's pe2_q | h1p_q bytes after the 16 reported head fields."""
    from test_cpu_host import _pack_host
    sd = weights.synthetic_state_dict(kind)
    buf, fields, _ = _pack_host(kind_id, sd)
    ref = pack.pack_heads(sd)
    tail = np.concatenate([ref[k].reshape(-1).view(np.uint32) for k in pack.HEAD_Q8_FIELDS])
    hsc = int(fields[16])
    assert buf.size == hsc + 8 + tail.size
    np.testing.assert_array_equal(buf[hsc + 8:].view(np.uint32), tail)
