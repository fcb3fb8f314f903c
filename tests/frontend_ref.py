"""numpy restatement of the RGB-D front end's rules (DESIGN.md "RGB-D front end"): the checker of
genpose2_amd/frontend.py and csrc/gp_frontend.hip, written from the rules, never the product."""
import numpy as np

from oracle.oracle import philox4x32_10

BACKGROUND = 255
SAMPLE_TAG = 0x53414D50
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def mask_stats(mask):
    """(256,5) int32 {count, rmin, rmax, cmin, cmax} per mask value; an absent value has {0, h, -1, w, -1}."""
    h, w = mask.shape
    out = np.tile(np.array([0, h, -1, w, -1], np.int32), (256, 1))
    for v in np.unique(mask):
        r, c = np.nonzero(mask == v)
        out[v] = (len(r), r.min(), r.max(), c.min(), c.max())
    return out


def crop_box(rmin, rmax, cmin, cmax, h, w):
    """The square window (multiples of 40 pixels, at most min(h, w) - 40, shifted back inside the image) of the
    pixel box, then centre (x, y) and scale."""
    win = (max(rmax - rmin, cmax - cmin) // 40 + 1) * 40
    win = min(win, h - 40, w - 40)
    cr, cc = (rmin + rmax) // 2, (cmin + cmax) // 2
    r0, r1, c0, c1 = cr - win // 2, cr + win // 2, cc - win // 2, cc + win // 2
    if r0 < 0:
        r0, r1 = 0, r1 - r0
    if c0 < 0:
        c0, c1 = 0, c1 - c0
    if r1 > h:
        r0, r1 = r0 - (r1 - h), h
    if c1 > w:
        c0, c1 = c0 - (c1 - w), w
    return 0.5 * (c0 + c1), 0.5 * (r0 + r1), float(min(max(r1 - r0, c1 - c0), max(h, w)))


def crop_boxes(stats, h, w):
    """ids (ascending, background left out) and their (centre x, centre y, scale)."""
    ids = [v for v in range(256) if v != BACKGROUND and stats[v, 0] > 0]
    return ids, [crop_box(int(stats[v, 1]), int(stats[v, 2]), int(stats[v, 3]), int(stats[v, 4]), h, w) for v in ids]


def source_coords(S, scale, centre):
    """The source position of crop index 0..S-1 along one axis, float64."""
    return (np.arange(S, dtype=np.float64) - S / 2) * scale / S + centre


def nearest(S, scale, centre):
    return np.floor(source_coords(S, scale, centre) + 0.5).astype(np.int64)


def sample_keys(c, obj_id, seed):
    e = np.arange(c, dtype=np.uint64)
    ctr = np.stack([e, np.full_like(e, obj_id), np.zeros_like(e), np.full_like(e, SAMPLE_TAG)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64), (c, 2))
    return philox4x32_10(ctr, key)[:, 0]


def sample_ids(c, n_pts, obj_id, seed):
    """Positions in V of the n_pts sampled elements."""
    if c < n_pts:
        return np.arange(n_pts) % c
    keys = sample_keys(c, obj_id, seed)
    return np.lexsort((np.arange(c), keys))[:n_pts]


def per_object(depth, mask, obj_id, box, K, S, n_pts, max_depth, seed):
    """-> pts (n_pts,3) float32, roi_xs, roi_ys (n_pts) int32, c, and whether a nearest source index fell
    outside the image. K = (fx, fy, cx, cy) float32, already scaled."""
    h, w = mask.shape
    bx, by, sc = box
    rows, cols = nearest(S, sc, by), nearest(S, sc, bx)
    rin, cin = (rows >= 0) & (rows < h), (cols >= 0) & (cols < w)
    inside = rin[:, None] & cin[None, :]
    rr, cc = np.clip(rows, 0, h - 1), np.clip(cols, 0, w - 1)
    d = np.where(inside, depth[rr][:, cc], np.float32(0))
    m = np.where(inside, mask[rr][:, cc] == obj_id, False)
    d = np.where(d > np.float32(max_depth), np.float32(0), d)
    valid = m & (d > 0)
    xs, ys = np.argwhere(valid).T          # crop row, crop column, row-major
    c = len(xs)
    if c < 10:
        raise ValueError(f"object {obj_id}: {c} valid points")
    sel = sample_ids(c, n_pts, obj_id, seed)
    xs, ys = xs[sel], ys[sel]
    fx, fy, cx, cy = (np.float32(v) for v in K)
    dd = d[xs, ys].astype(np.float32)
    x = (cols[ys].astype(np.float32) - cx) * dd / fx
    y = (rows[xs].astype(np.float32) - cy) * dd / fy
    assert x.dtype == np.float32 and y.dtype == np.float32
    pts = np.stack([x, y, dd], -1)
    return pts, xs.astype(np.int32), ys.astype(np.int32), c, bool((~rin).any() or (~cin).any())


def roi_rgb_levels(color, box, S):
    """The bilinear crop before rounding, float64 (S,S,3); taps outside the image are 0."""
    h, w, _ = color.shape
    bx, by, sc = box
    u, v = source_coords(S, sc, bx), source_coords(S, sc, by)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    ax, ay = u - x0, v - y0
    pad = np.zeros((h + 2, w + 2, 3), np.float64)     # one zero pixel around: index + 1
    pad[1:-1, 1:-1] = color
    xi, yi = np.clip(x0 + 1, 0, w), np.clip(y0 + 1, 0, h)
    # positions further than one pixel outside read zeros only
    xz, yz = (x0 < -1) | (x0 > w - 1), (y0 < -1) | (y0 > h - 1)
    tap = lambda dy, dx: pad[np.clip(yi + dy, 0, h + 1)][:, np.clip(xi + dx, 0, w + 1)]   # noqa: E731
    wx0, wx1 = (1 - ax)[None, :, None], ax[None, :, None]
    wy0, wy1 = (1 - ay)[:, None, None], ay[:, None, None]
    val = wy0 * (wx0 * tap(0, 0) + wx1 * tap(0, 1)) + wy1 * (wx0 * tap(1, 0) + wx1 * tap(1, 1))
    val[yz] = 0
    val[:, xz] = 0
    return val


def roi_rgb(color, box, S):
    """-> (normalised (3,S,S) float64, uint8 levels (S,S,3), distance of the value to its rounding boundary)."""
    val = roi_rgb_levels(color, box, S)
    q = np.clip(np.floor(val + 0.5), 0, 255)
    frac = val + 0.5 - np.floor(val + 0.5)
    dist = np.minimum(frac, 1 - frac)
    norm = (q / 255.0 - np.array(MEAN)) / np.array(STD)
    return norm.transpose(2, 0, 1), q.astype(np.uint8), dist


def scaled_intrinsics(fx, fy, cx, cy, width, height, W, H):
    """float32 intrinsics times W / width and H / height, in float32."""
    sx, sy = np.float32(W / width), np.float32(H / height)
    return np.float32(fx) * sx, np.float32(fy) * sy, np.float32(cx) * sx, np.float32(cy) * sy


def frame_objects(depth, color, mask, intrinsics, img_size=224, n_pts=1024, max_depth=4.0, seed=0):
    h, w = mask.shape
    K = scaled_intrinsics(*(intrinsics[k] for k in ("fx", "fy", "cx", "cy", "width", "height")), w, h)
    ids, boxes = crop_boxes(mask_stats(mask), h, w)
    out = {"ids": np.array(ids, np.int32), "boxes": boxes, "pts": [], "roi_xs": [], "roi_ys": [], "count": [],
           "outside": []}
    for obj_id, box in zip(ids, boxes):
        pts, xs, ys, c, outside = per_object(depth, mask, obj_id, box, K, img_size, n_pts, max_depth, seed)
        for k, v in zip(("pts", "roi_xs", "roi_ys", "count", "outside"), (pts, xs, ys, c, outside)):
            out[k].append(v)
    for k in ("pts", "roi_xs", "roi_ys"):
        out[k] = np.stack(out[k]) if ids else np.zeros((0, n_pts) + ((3,) if k == "pts" else ()))
    out["count"] = np.array(out["count"], np.int32)
    out["pts_center"] = out["pts"].astype(np.float64).mean(1) if ids else np.zeros((0, 3))
    return out
