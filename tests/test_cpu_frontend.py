"""CPU-only tests of the RGB-D front end: the C ABI's new symbols, the host crop-box arithmetic, argument checks,
and self-checks of the numpy restatement (tests/frontend_ref.py). No HIP compute calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import frontend_ref as ref

NEW = ("gp_frame_mask_stats", "gp_frame_crop_boxes", "gp_frame_objects_workspace_size", "gp_frame_objects",
       "gp_frame_roi_rgb")


def _lib():
    from genpose2_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_and_exported():
    from genpose2_amd import _lib
    hdr = open(os.path.join(REPO, "include", "genpose_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared
    assert set(NEW) <= set(_lib.EXPORTED)
    assert set(NEW) <= set(_lib.exported_symbols())
    assert _lib.load().gp_abi_version() == 7
    assert "#define GP_ABI_VERSION 7" in hdr


H, W = 120, 160
# rmin, rmax, cmin, cmax of hand-made objects in a 120 x 160 frame
BOX_CASES = {
    "interior": (50, 79, 60, 89),
    "top": (0, 10, 70, 90),
    "left": (50, 70, 0, 12),
    "bottom": (100, 119, 60, 85),
    "right": (40, 60, 140, 159),
    "bottom_right": (95, 119, 130, 159),
    "window_limited_by_h_minus_40": (5, 115, 20, 140),   # 121-pixel box: window 160 -> min(80, 120) = 80
    "single_pixel": (33, 33, 47, 47),
    "single_pixel_corner": (0, 0, 0, 0),
}


def _c_crop_boxes(stats, h, w):
    from genpose2_amd import frontend
    return frontend.crop_boxes(stats, h, w)


@pytest.mark.parametrize("case", sorted(BOX_CASES))
def test_crop_boxes_match_restatement(case):
    rmin, rmax, cmin, cmax = BOX_CASES[case]
    stats = np.tile(np.array([0, H, -1, W, -1], np.int32), (256, 1))
    stats[7] = ((rmax - rmin + 1) * (cmax - cmin + 1), rmin, rmax, cmin, cmax)
    stats[255] = (H * W, 0, H - 1, 0, W - 1)          # background: never an object
    ids, boxes = _c_crop_boxes(stats, H, W)
    rids, rboxes = ref.crop_boxes(stats, H, W)
    assert ids.tolist() == rids == [7]
    assert boxes.dtype == np.float32 and boxes.tolist() == [list(rboxes[0])]
    cx, cy, scale = boxes[0]
    assert 0 < scale <= min(H, W) - 40 and scale % 1 == 0
    # the window lies inside the image
    assert cx - scale / 2 >= 0 and cx + scale / 2 <= W and cy - scale / 2 >= 0 and cy + scale / 2 <= H


def test_crop_boxes_expected_values():
    """Worked by hand from the rules, independent of the restatement."""
    stats = np.tile(np.array([0, H, -1, W, -1], np.int32), (256, 1))
    stats[0] = (1, 50, 79, 60, 89)      # window 40 around (64, 74): rows 44..84, columns 54..94
    stats[9] = (1, 95, 119, 130, 159)   # window 40 around (107, 144), shifted to rows 80..120, columns 120..160
    stats[3] = (1, 5, 115, 20, 140)     # window 80 around (60, 80): rows 20..100, columns 40..120
    ids, boxes = _c_crop_boxes(stats, H, W)
    assert ids.tolist() == [0, 3, 9]
    assert boxes.tolist() == [[74.0, 64.0, 40.0], [80.0, 60.0, 80.0], [140.0, 100.0, 40.0]]


def test_crop_boxes_all_ids_ascending_without_background():
    stats = np.tile(np.array([1, 50, 60, 50, 60], np.int32), (256, 1))
    ids, boxes = _c_crop_boxes(stats, H, W)
    assert ids.tolist() == list(range(255)) and boxes.shape == (255, 3)
    stats[:, 0] = 0
    ids, boxes = _c_crop_boxes(stats, H, W)
    assert len(ids) == 0 and boxes.shape == (0, 3)


def test_argument_checks_return_invalid_without_a_device():
    lib = _lib()
    buf = np.zeros(256 * 5, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)

    def objects(h=120, w=160, b=1, s=56, n=128, pts=p, xs=p, ys=p, cnt=p, ws=p, wsb=1 << 30):
        return lib.gp_frame_objects(p, p, h, w, p, p, b, s, n, 1.0, 1.0, 0.0, 0.0, 4.0, 0, pts, xs, ys, cnt, ws, wsb,
                                    None)

    assert objects(n=2049) == -1 and b"n_pts" in lib.gp_last_error()
    assert objects(n=0) == -1
    assert objects(s=13) == -1 and b"img_size" in lib.gp_last_error()
    assert objects(b=-1) == -1
    for out in ("pts", "xs", "ys", "cnt"):
        assert objects(**{out: None}) == -1 and b"null output" in lib.gp_last_error()
    assert objects(ws=None) == -1
    assert objects(wsb=56 * 56 * 4 - 1) == -1 and b"workspace" in lib.gp_last_error()
    assert objects(h=0) == -1
    assert lib.gp_frame_roi_rgb(p, 120, 160, p, 1, 56, None, None) == -1 and b"null output" in lib.gp_last_error()
    assert lib.gp_frame_roi_rgb(p, 120, 160, p, -1, 56, p, None) == -1
    assert lib.gp_frame_roi_rgb(p, 120, 160, p, 1, 12, p, None) == -1
    assert lib.gp_frame_mask_stats(p, 120, 160, None, None) == -1
    assert lib.gp_frame_mask_stats(None, 120, 160, p, None) == -1
    assert lib.gp_frame_crop_boxes(p, 120, 160, p, p, None) == -1
    assert lib.gp_frame_crop_boxes(p, 40, 160, p, p, p) == -1
    assert lib.gp_frame_objects_workspace_size(2, 224) == 2 * 224 * 224 * 4
    assert lib.gp_frame_objects_workspace_size(0, 224) == 0


def test_python_argument_checks_need_no_device():
    from genpose2_amd import frontend
    z = np.zeros((120, 160), np.uint8)
    K = dict(fx=100.0, fy=100.0, cx=80.0, cy=60.0, width=160, height=120)
    with pytest.raises(ValueError, match="HIP device"):
        frontend.frame_objects(z.astype(np.float32), np.zeros((120, 160, 3), np.uint8), z, K, device="cpu")
    intr = frontend._intrinsics({"camera": {"intrinsics": K}})
    assert intr == {k: float(v) for k, v in K.items()}
    assert frontend.scaled_intrinsics(dict(K, width=320, height=240), 120, 160) == (50.0, 50.0, 40.0, 30.0)


# ---------------------------------------------------------------------------- the restatement's own rules
def _tiny_frame(extra_ids=()):
    rng = np.random.default_rng(3)
    h, w = 100, 120
    mask = np.full((h, w), 255, np.uint8)
    mask[30:60, 40:75] = 5                       # c > n_pts at S = 56
    for k, v in enumerate(extra_ids):
        mask[2 + 9 * k:9 + 9 * k, 3:12] = v
    depth = (1.0 + 0.01 * np.arange(w)[None, :] + 0.003 * np.arange(h)[:, None]).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0
    return depth, mask


def _K(h, w):
    return np.float32(150.0), np.float32(150.0), np.float32(w / 2), np.float32(h / 2)


def test_restatement_tiling_rule():
    assert ref.sample_ids(10, 25, 5, 0).tolist() == [j % 10 for j in range(25)]
    depth, mask = _tiny_frame()
    h, w = mask.shape
    box = ref.crop_boxes(ref.mask_stats(mask), h, w)[1][0]
    big = ref.per_object(depth, mask, 5, box, _K(h, w), 28, 2048, 4.0, 0)
    c = big[3]
    assert 10 <= c < 2048
    assert np.array_equal(big[0][c:2 * c], big[0][:c]) and np.array_equal(big[1][:2048 - c], big[1][c:])
    # row-major crop order: (row, column) strictly increasing over the first c entries
    lin = big[1][:c].astype(np.int64) * 28 + big[2][:c]
    assert np.all(np.diff(lin) > 0)


def test_restatement_selection_is_distinct_and_ordered_by_key():
    c, n = 5000, 128
    sel = ref.sample_ids(c, n, 5, 11)
    assert len(set(sel.tolist())) == n and sel.max() < c
    keys = ref.sample_keys(c, 5, 11)
    comp = (keys.astype(np.uint64) << np.uint64(32)) | np.arange(c, dtype=np.uint64)
    assert np.array_equal(np.sort(comp)[:n], comp[sel])
    assert not np.array_equal(sel, ref.sample_ids(c, n, 5, 12))      # the seed matters
    assert not np.array_equal(sel, ref.sample_ids(c, n, 6, 11))      # and the id
    assert sorted(ref.sample_ids(n, n, 5, 11).tolist()) == list(range(n))   # c == n_pts: a permutation


def test_restatement_sample_independent_of_other_objects():
    K = dict(fx=150.0, fy=150.0, cx=60.0, cy=50.0, width=120, height=100)
    color = np.zeros((100, 120, 3), np.uint8)
    depth, m1 = _tiny_frame()
    a = ref.frame_objects(depth, color, m1, K, 56, 128, 4.0, 4)
    _, m2 = _tiny_frame(extra_ids=(9, 2, 77))
    b = ref.frame_objects(depth, color, m2, K, 56, 128, 4.0, 4)
    _, m3 = _tiny_frame(extra_ids=(77, 9, 2))     # the same ids on other pixels
    c = ref.frame_objects(depth, color, m3, K, 56, 128, 4.0, 4)
    assert a["ids"].tolist() == [5] and b["ids"].tolist() == [2, 5, 9, 77] == c["ids"].tolist()
    assert a["count"][0] > 128
    for other in (b, c):
        for k in ("pts", "roi_xs", "roi_ys"):
            assert np.array_equal(a[k][0], other[k][1]), k
    with pytest.raises(ValueError, match="object 4"):
        m4 = m1.copy()
        m4[0, 0:2] = 4
        ref.frame_objects(depth, color, m4, K, 56, 128, 4.0, 4)


def test_restatement_bilinear_crop_identity_and_border():
    """scale = S maps crop pixels onto source pixels half a pixel apart from the centre's fraction: with an
    integer centre the crop is a copy; outside the image it is 0."""
    rng = np.random.default_rng(0)
    color = rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)
    val = ref.roi_rgb_levels(color, (30.0, 20.0, 28.0), 28)           # columns 16..43, rows 6..33
    assert np.array_equal(val, color[6:34, 16:44].astype(np.float64))
    val = ref.roi_rgb_levels(color, (60.0, 50.0, 28.0), 28)           # columns 46..73, rows 36..63
    assert np.array_equal(val[:24, :24], color[36:60, 46:70]) and not val[24:].any() and not val[:, 24:].any()
    val = ref.roi_rgb_levels(color, (30.5, 20.0, 28.0), 28)           # half-pixel shift: the mean of two columns
    assert np.array_equal(val, 0.5 * (color[6:34, 16:44].astype(np.float64) + color[6:34, 17:45]))
