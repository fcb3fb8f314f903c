"""ImgEncoder.forward (networks/img_encoder/img_encoder.py:48-100, eval) and the patch -> point gather of
GFObjectPose.extract_pts_feature (networks/posenet.py:146-192) restated in plain float64 numpy, with the semantics
oracle.img_encoder_forward states in float32 torch: the yardstick of the image encoder's edge tests. ``variant=``
switches on one deliberate mistake, so that the CPU test can show that a case sees it."""
from __future__ import annotations

import numpy as np

PREFIX = "img_encoder"
# the mistakes: position table transposed; G from the first 3d/4 channels; the softmax's keys past the last whole
# 64 dropped; the conv's padding wrapped round the map; a flat im2col that wraps rows (only the pixel index is
# checked); edge[c // 4] for edge[c % co] in the final mix; the second edge chunk written at the first one's offset;
# the table index wrapped (mod rows) instead of clamped
VARIANTS = ("table_transposed", "g_first_channels", "softmax_tail_dropped", "conv_wrap", "im2col_row_wrap",
            "edge_div4", "chunk_edge_offset", "index_wrap")
EDGE_CHUNK = 256


def table_index(grid: int, num_emb: int, wrap: bool = False) -> np.ndarray:
    """(np, np) int: [i][j] = clamp((c_j - c_i + g - 1) . (2 g - 1, 1), 0, num_emb - 1), c_p = (p // g, p % g)."""
    p = np.arange(grid * grid)
    r0 = p[None, :] // grid - p[:, None] // grid + grid - 1
    r1 = p[None, :] % grid - p[:, None] % grid + grid - 1
    idx = r0 * (2 * (grid - 1) + 1) + r1
    return idx % num_emb if wrap else np.clip(idx, 0, num_emb - 1)


def geo_table64(E, grid: int, variant=None) -> np.ndarray:
    """rel_pos_emb(rel_pos_idx).sum(-1) in float64: (np, np)."""
    E = np.asarray(E, np.float64)
    t = E.sum(axis=-1)[table_index(grid, E.shape[0], wrap=variant == "index_wrap")]
    return t.T.copy() if variant == "table_transposed" else t


def _conv3x3(fused, w, bias, grid, variant):
    """relu-less Conv2d(d, co, 3, padding=1) over spatial_feat = fused^T viewed (d, g, g): -> (B, np, co)."""
    B, n, d = fused.shape
    g = grid
    out = np.broadcast_to(bias, (B, n, w.shape[0])).copy()
    if variant == "im2col_row_wrap":
        for ky in range(3):
            for kx in range(3):
                off = (ky - 1) * g + (kx - 1)
                src = np.arange(n) + off
                ok = (src >= 0) & (src < n)
                nb = np.where(ok[None, :, None], fused[:, np.clip(src, 0, n - 1)], 0.0)
                out += nb @ w[:, :, ky, kx].T
        return out
    m = fused.reshape(B, g, g, d)
    pad = np.pad(m, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="wrap" if variant == "conv_wrap" else "constant")
    for ky in range(3):
        for kx in range(3):
            out += (pad[:, ky:ky + g, kx:kx + g] @ w[:, :, ky, kx].T).reshape(B, n, -1)
    return out


def img_encoder_forward64(sd, layers, grid: int, variant=None, prefix: str = PREFIX) -> dict:
    """Three (B, np, d) layers -> {"final" (B, np, d), "layer_w" (B, np, 3), "edge" (B, d/4), "fused" (B, np, d)}."""
    assert variant is None or variant in VARIANTS, variant
    t = lambda k: np.asarray(sd[f"{prefix}.{k}"], np.float64)  # noqa: E731
    f = np.stack([np.asarray(v, np.float64) for v in layers], 1)                       # (B, 3, np, d)
    B, _, n, d = f.shape
    assert n == grid * grid
    co = d // 4
    # layer attention: Linear -> ReLU -> Linear(., 1), softmax over the three layers, weighted sum
    h = np.maximum(f @ t("layer_attn.0.weight").T + t("layer_attn.0.bias"), 0.0)
    s = h @ t("layer_attn.2.weight").reshape(-1) + t("layer_attn.2.bias").reshape(-1)[0]   # (B, 3, np)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    fused = (f * w[..., None]).sum(axis=1)                                             # (B, np, d)
    # geometric attention: G G^T x the position table, softmax over the keys, times fused
    G = fused[:, :, :d - co] if variant == "g_first_channels" else fused[:, :, co:]
    logits = (G @ G.transpose(0, 2, 1)) * geo_table64(t("rel_pos_emb.weight"), grid, variant)
    if variant == "softmax_tail_dropped" and n > 64 and n % 64:
        logits[:, :, n // 64 * 64:] = -np.inf
    p = np.exp(logits - logits.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    geo = p @ fused
    # edge branch: conv -> ReLU -> mean over the pixels
    edge = np.maximum(_conv3x3(fused, t("edge_guide.0.weight"), t("edge_guide.0.bias"), grid, variant), 0.0).mean(axis=1)
    if variant == "chunk_edge_offset" and B > EDGE_CHUNK:
        edge = edge.copy()
        edge[EDGE_CHUNK:] = edge[np.arange(EDGE_CHUNK, B) % EDGE_CHUNK]
    c = np.arange(d)
    ec = edge[:, c // 4] if variant == "edge_div4" else edge[:, c % co]
    gw, ew = max(float(t("geo_weight").reshape(-1)[0]), 0.0), max(float(t("edge_weight").reshape(-1)[0]), 0.0)
    final = fused + gw * geo + ew * (fused * ec[:, None, :])
    return {"final": final, "layer_w": np.ascontiguousarray(w.transpose(0, 2, 1)), "edge": edge, "fused": fused,
            "attn_max": p.max(axis=-1)}


def gather_ref(feat, xs, ys, patch: int, grid: int) -> np.ndarray:
    """feat[b][clamp(floor(xs / patch) * grid + floor(ys / patch), 0, np - 1)]: floor division of each coordinate,
    ONE clamp of the combined index (an in-range xs with ys = -1 lands on the previous row's last patch)."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    pos = np.floor_divide(xs, patch) * grid + np.floor_divide(ys, patch)
    pos = np.minimum(np.maximum(pos, 0), feat.shape[1] - 1)
    return np.take_along_axis(np.asarray(feat), pos[..., None], 1)
