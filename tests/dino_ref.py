"""From-scratch torch restatement of DINOv3 ViT-S+/16 ``get_intermediate_layers(x, n, reshape=False, norm=True,
return_class_token=False)`` over the ORIGINAL key format (weights.DINO_TOP_KEYS / DINO_BLOCK_KEYS), for the
backbone's fixtures and tests. Dtype-generic (float32 and float64), any torch device; written from the published
architecture, independent of genpose2_amd/dino.py's packing (no folding, no interleaving).

The ``variant`` switches exist only to prove that a fixture can see a mistake: "no_rope" (q, k not rotated),
"swap_hw" (the h and w angle halves exchanged), "no_mask" (qkv.bias_mask ignored), "rope_prefix" (the 5 prefix
tokens rotated too, with the first patches' angles), "zero_key_tail" ((-n) % 16 all-zero key / value rows appended
after RoPE and left unmasked in the softmax: an attention kernel that pads its last 16-key tile and loses the mask).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

D, HEADS, HEAD_DIM, PATCH, PREFIX, BLOCKS, EPS = 384, 6, 64, 16, 5, 12, 1e-5
VARIANTS = ("no_rope", "swap_hw", "no_mask", "rope_prefix", "zero_key_tail")


def rope_cos_sin(hp: int, wp: int, periods: Optional[torch.Tensor], dtype, device="cpu", swap_hw: bool = False
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hp * wp, 64) cos and sin: patch centres (i + 0.5) / hp mapped to [-1, 1], angles 2 pi coord / periods laid
    out [h(16) | w(16)] and tiled twice."""
    if periods is None:
        periods = 100.0 ** (torch.arange(HEAD_DIM // 4, dtype=torch.float64) * 4.0 / HEAD_DIM)
    periods = periods.to(device=device, dtype=dtype)
    ch = 2.0 * ((torch.arange(hp, dtype=dtype, device=device) + 0.5) / hp) - 1.0
    cw = 2.0 * ((torch.arange(wp, dtype=dtype, device=device) + 0.5) / wp) - 1.0
    gh, gw = torch.meshgrid(ch, cw, indexing="ij")
    coords = torch.stack([gw, gh] if swap_hw else [gh, gw], dim=-1).reshape(hp * wp, 2)
    ang = 2.0 * math.pi * coords[:, :, None] / periods[None, None, :]
    ang = ang.reshape(hp * wp, HEAD_DIM // 2).repeat(1, 2)
    return torch.cos(ang), torch.sin(ang)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def forward(sd: Dict[str, np.ndarray], x, layers: Sequence[int] = (2, 6, 11), dtype=torch.float32, device="cpu",
            variant: Optional[str] = None, rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """x (B, 3, H, W) -> [norm(hidden state after block l)[:, 5:] for l in layers], each (B, H/16 * W/16, 384).
    ``rope``: (cos, sin) used instead of rope_cos_sin (cross-checks against another implementation's table)."""
    assert variant is None or variant in VARIANTS, variant
    # values: numpy arrays, or tensors (already on the device: no copy per call)
    g = lambda k: (sd[k] if isinstance(sd[k], torch.Tensor) else torch.as_tensor(np.asarray(sd[k]))).to(  # noqa: E731
        device=device, dtype=dtype)
    x = torch.as_tensor(x).to(device=device, dtype=dtype)
    B, _, H, W = x.shape
    hp, wp = H // PATCH, W // PATCH
    tok = F.conv2d(x, g("patch_embed.proj.weight"), g("patch_embed.proj.bias"), stride=PATCH)   # (B, D, hp, wp)
    tok = tok.flatten(2).transpose(1, 2)                                                      # row-major patches
    h = torch.cat([g("cls_token").reshape(1, 1, D).expand(B, -1, -1),
                   g("storage_tokens").reshape(1, PREFIX - 1, D).expand(B, -1, -1), tok], dim=1)
    n = h.shape[1]
    if rope is None:
        periods = g("rope_embed.periods") if "rope_embed.periods" in sd else None
        cos, sin = rope_cos_sin(hp, wp, periods, dtype, device, swap_hw=variant == "swap_hw")
    else:
        cos, sin = (t.to(device=device, dtype=dtype) for t in rope)

    def rot(t):   # (B, heads, n, 64)
        if variant == "no_rope":
            return t
        if variant == "rope_prefix":
            c = torch.cat([cos[:PREFIX], cos], dim=0)
            s = torch.cat([sin[:PREFIX], sin], dim=0)
            return t * c + rotate_half(t) * s
        pre, pat = t[:, :, :PREFIX], t[:, :, PREFIX:]
        return torch.cat([pre, pat * cos + rotate_half(pat) * sin], dim=2)

    outs = {}
    for i in range(max(layers) + 1):
        p = f"blocks.{i}."
        y = F.layer_norm(h, (D,), g(p + "norm1.weight"), g(p + "norm1.bias"), EPS)
        bias = g(p + "attn.qkv.bias")
        if p + "attn.qkv.bias_mask" in sd and variant != "no_mask":
            bias = bias * g(p + "attn.qkv.bias_mask")
        qkv = F.linear(y, g(p + "attn.qkv.weight"), bias).reshape(B, n, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
        q, k, v = rot(qkv[0]), rot(qkv[1]), qkv[2]
        if variant == "zero_key_tail" and (-n) % 16:
            pad = k.new_zeros(k.shape[:2] + ((-n) % 16, HEAD_DIM))
            k, v = torch.cat([k, pad], dim=2), torch.cat([v, pad], dim=2)
        att = torch.softmax(q @ k.transpose(-1, -2) * (HEAD_DIM ** -0.5), dim=-1) @ v       # (B, heads, n, 64)
        att = att.transpose(1, 2).reshape(B, n, D)
        h = h + g(p + "ls1.gamma") * F.linear(att, g(p + "attn.proj.weight"), g(p + "attn.proj.bias"))
        y = F.layer_norm(h, (D,), g(p + "norm2.weight"), g(p + "norm2.bias"), EPS)
        hid = F.silu(F.linear(y, g(p + "mlp.w1.weight"), g(p + "mlp.w1.bias"))) * \
            F.linear(y, g(p + "mlp.w2.weight"), g(p + "mlp.w2.bias"))
        h = h + g(p + "ls2.gamma") * F.linear(hid, g(p + "mlp.w3.weight"), g(p + "mlp.w3.bias"))
        if i in layers:
            outs[i] = F.layer_norm(h, (D,), g("norm.weight"), g("norm.bias"), EPS)[:, PREFIX:]
    return [outs[i] for i in layers]


# ------------------------------------------------------------------ the transformers cross-check
def hf_state_dict(sd: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
    """The original keys mapped onto transformers' DINOv3ViTModel (key_bias=False: it has no k_proj.bias, which
    equals the masked bias of the original)."""
    t = lambda k: torch.as_tensor(np.asarray(sd[k]), dtype=torch.float64)  # noqa: E731
    out = {"embeddings.cls_token": t("cls_token").reshape(1, 1, D),
           "embeddings.mask_token": t("mask_token").reshape(1, 1, D),
           "embeddings.register_tokens": t("storage_tokens").reshape(1, PREFIX - 1, D),
           "embeddings.patch_embeddings.weight": t("patch_embed.proj.weight"),
           "embeddings.patch_embeddings.bias": t("patch_embed.proj.bias"),
           "norm.weight": t("norm.weight"), "norm.bias": t("norm.bias")}
    for i in range(BLOCKS):
        p, o = f"blocks.{i}.", f"model.layer.{i}."
        w, b = t(p + "attn.qkv.weight"), t(p + "attn.qkv.bias")
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
            out[f"{o}attention.{nm}.weight"] = w[j * D:(j + 1) * D]
            if nm != "k_proj":
                out[f"{o}attention.{nm}.bias"] = b[j * D:(j + 1) * D]
        out[o + "attention.o_proj.weight"], out[o + "attention.o_proj.bias"] = t(p + "attn.proj.weight"), t(p + "attn.proj.bias")
        out[o + "layer_scale1.lambda1"], out[o + "layer_scale2.lambda1"] = t(p + "ls1.gamma"), t(p + "ls2.gamma")
        for nm in ("norm1", "norm2"):
            out[f"{o}{nm}.weight"], out[f"{o}{nm}.bias"] = t(f"{p}{nm}.weight"), t(f"{p}{nm}.bias")
        for src, dst in (("w1", "gate_proj"), ("w2", "up_proj"), ("w3", "down_proj")):
            out[f"{o}mlp.{dst}.weight"], out[f"{o}mlp.{dst}.bias"] = t(f"{p}mlp.{src}.weight"), t(f"{p}mlp.{src}.bias")
    return out


def hf_cross_check(sd: Dict[str, np.ndarray], x: np.ndarray, layers: Sequence[int] = (2, 6, 11)):
    """transformers' DINOv3ViTModel in float64 with the mapped weights against forward() in float64.
    transformers evaluates its RoPE table in float32 whatever the model's dtype, so the comparison has two parts:
    -> (max |difference| of the outputs with forward() given THAT table, max |difference| of the two tables)."""
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    cfg = DINOv3ViTConfig(hidden_size=D, intermediate_size=1536, num_attention_heads=HEADS, num_hidden_layers=BLOCKS,
                          num_register_tokens=PREFIX - 1, use_gated_mlp=True, hidden_act="silu", key_bias=False,
                          layerscale_value=1.0, patch_size=PATCH, image_size=int(x.shape[-1]))
    model = DINOv3ViTModel(cfg).double().eval()
    missing, unexpected = model.load_state_dict(hf_state_dict(sd), strict=False)
    assert not unexpected and all("inv_freq" in k for k in missing), (missing, unexpected)
    xt = torch.as_tensor(x, dtype=torch.float64)
    with torch.no_grad():
        hs = model(xt, output_hidden_states=True).hidden_states
        theirs = [model.norm(hs[l + 1])[:, PREFIX:] for l in layers]
        cos, sin = model.rope_embeddings(xt)
        cos, sin = cos.reshape(-1, HEAD_DIM), sin.reshape(-1, HEAD_DIM)
        sd_np = dict(sd)
        sd_np.pop("rope_embed.periods", None)   # transformers computes its periods
        ours = forward(sd_np, xt, layers, torch.float64, rope=(cos, sin))
        mine = rope_cos_sin(x.shape[-2] // PATCH, x.shape[-1] // PATCH, None, torch.float64)
    out_diff = max(float((a - b).abs().max()) for a, b in zip(ours, theirs))
    tab_diff = max(float((mine[0] - cos).abs().max()), float((mine[1] - sin).abs().max()))
    return out_diff, tab_diff
