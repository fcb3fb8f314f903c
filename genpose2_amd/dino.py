"""The frozen DINOv3 ViT-S+/16 backbone of ``--dino pointwise`` (posenet.py:56-62, 138-144) on device.

``DinoBackbone(sd, device).get_intermediate_layers(roi_rgb, n=[2, 6, 11], reshape=False, norm=True,
return_class_token=False)`` is the call GFObjectPose makes; ``sd`` holds the backbone in its original key
format (weights.DINO_TOP_KEYS / DINO_BLOCK_KEYS), without the checkpoint's ``dino.`` prefix. Everything runs in
``gp_dino_forward`` (csrc/gp_dino.hip); this module packs the weights and moves pointers.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, arch, weights
from ._lib import check, vp
from .device import require_device_tensor, stream_handle
from .fus_encoder import pack_split_linear

ARITH = {"split_f16": 0, "f32": 1}
_LINEARS = ("qkv", "proj", "w12", "w3")


def interleave_gate_up(gate: np.ndarray, up: np.ndarray) -> np.ndarray:
    """[w1 | w2] in 16-row tiles: rows 32t..32t+15 = gate rows 16t.., rows 32t+16..32t+31 = up rows 16t.. (the
    order gp_linear_split's SwiGLU epilogue pairs); works for the (1536, 384) weights and the (1536,) biases."""
    g = gate.reshape((gate.shape[0] // 16, 16) + gate.shape[1:])
    u = up.reshape(g.shape)
    return np.stack([g, u], axis=1).reshape((2 * gate.shape[0],) + gate.shape[1:])


def pack_dino(sd: weights.StateDict) -> Dict[str, np.ndarray]:
    """The arrays gp_dino_weights points to. LayerScale is folded into proj and w3 (W' = gamma W, b' = gamma b, in
    float64, rounded once), the qkv bias is multiplied by its mask when the state dict has one (a non-finite
    mask is a load error), w1 | w2 are interleaved; every linear also gets its split-f16 planes (``*.wh``).
    ``rope_periods``: the stored periods (float32), or absent."""
    weights.check_keys(sd, "dino")
    f64 = lambda k: np.asarray(sd[k], np.float64)  # noqa: E731
    out: Dict[str, np.ndarray] = {
        "patch.w": f64(weights.dino_key("patch_w")).reshape(arch.DINO_DIM, -1),
        "patch.b": f64(weights.dino_key("patch_b")),
        "cls": f64(weights.dino_key("cls_token")).reshape(-1),
        "storage": f64(weights.dino_key("storage_tokens")).reshape(arch.DINO_STORAGE, arch.DINO_DIM),
        "norm.w": f64(weights.dino_key("norm_w")), "norm.b": f64(weights.dino_key("norm_b")),
    }
    if weights.dino_key("rope_periods") in sd:
        per = f64(weights.dino_key("rope_periods"))
        if not (np.all(np.isfinite(per)) and np.all(per > 0)):
            raise ValueError("rope_embed.periods must be positive and finite")
        out["rope_periods"] = per
    for i in range(arch.DINO_BLOCKS):
        g = lambda role: f64(weights.dino_key(role, i))  # noqa: E731
        p = f"b{i}."
        for nm in ("ln1", "ln2"):
            out[f"{p}{nm}.w"], out[f"{p}{nm}.b"] = g(f"{nm}_w"), g(f"{nm}_b")
        qb = g("qkv_b")
        if weights.dino_key("qkv_mask", i) in sd:
            mask = g("qkv_mask")
            if not np.all(np.isfinite(mask)):
                raise ValueError(f"blocks.{i}.attn.qkv.bias_mask is not finite")
            qb = qb * mask
        out[f"{p}qkv.w"], out[f"{p}qkv.b"] = g("qkv_w"), qb
        ls1, ls2 = g("ls1"), g("ls2")
        out[f"{p}proj.w"], out[f"{p}proj.b"] = ls1[:, None] * g("proj_w"), ls1 * g("proj_b")
        out[f"{p}w12.w"] = interleave_gate_up(g("gate_w"), g("up_w"))
        out[f"{p}w12.b"] = interleave_gate_up(g("gate_b"), g("up_b"))
        out[f"{p}w3.w"], out[f"{p}w3.b"] = ls2[:, None] * g("down_w"), ls2 * g("down_b")
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}
    for i in range(arch.DINO_BLOCKS):
        for nm in _LINEARS:
            out[f"b{i}.{nm}.wh"] = pack_split_linear(out[f"b{i}.{nm}.w"])
    return out


class DinoBackbone:
    """dinov3_vits16plus on device. ``get_intermediate_layers`` as the reference calls it; ``calls`` counts its
    invocations."""

    def __init__(self, sd: weights.StateDict, device: torch.device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        packed = pack_dino(sd)
        self.periods = packed.pop("rope_periods", None)
        self.t = {k: torch.from_numpy(v).to(self.device) for k, v in packed.items()}
        self._rope: Dict[Tuple[int, int], torch.Tensor] = {}
        self._ws: Optional[torch.Tensor] = None
        self.max_workspace_bytes: Optional[int] = None   # tests: a smaller workspace forces smaller chunks
        self.calls = 0
        self.set_arith(os.environ.get("GENPOSE2_ENC_ARITH", "split_f16"))

    def set_arith(self, arith: str) -> None:
        """Arithmetic of the linears: "split_f16" (gp_linear_split's three f16 MFMA products) or "f32" (exact
        fp32 MFMA), the selection ImgEncoderModel uses."""
        if arith not in ARITH:
            raise ValueError(f"unknown backbone arithmetic {arith!r} (split_f16 | f32)")
        self.arith = arith

    def same_weights(self, other: "DinoBackbone") -> bool:
        """Byte-identical packed weights and periods (compared once at load by the pipeline)."""
        if self.t.keys() != other.t.keys():
            return False
        if (self.periods is None) != (other.periods is None) or \
                (self.periods is not None and not np.array_equal(self.periods, other.periods)):
            return False
        return all(torch.equal(v, other.t[k].to(v.device)) for k, v in self.t.items())

    def rope_table(self, hp: int, wp: int) -> torch.Tensor:
        """cos / sin of the (hp, wp) patch grid, built once per shape (gp_dino_rope_table)."""
        tab = self._rope.get((hp, wp))
        if tab is None:
            tab = torch.empty((hp * wp, 64), dtype=torch.float32, device=self.device)
            per = None if self.periods is None else np.ascontiguousarray(self.periods, np.float32)
            check(self.lib.gp_dino_rope_table(None if per is None else per.ctypes.data_as(ctypes.c_void_p), hp, wp,
                                              vp(tab), ctypes.c_void_p(stream_handle(self.device))), "dino_rope_table")
            self._rope[(hp, wp)] = tab
        return tab

    def _weights(self, rope: torch.Tensor, hp: int, wp: int) -> _lib.DinoWeights:
        t = self.t
        w = _lib.DinoWeights()
        w.patch_w, w.patch_b = t["patch.w"].data_ptr(), t["patch.b"].data_ptr()
        w.cls_token, w.storage_tokens = t["cls"].data_ptr(), t["storage"].data_ptr()
        w.norm_w, w.norm_b = t["norm.w"].data_ptr(), t["norm.b"].data_ptr()
        w.rope, w.rope_hp, w.rope_wp = rope.data_ptr(), hp, wp
        for i in range(arch.DINO_BLOCKS):
            blk, p = w.blocks[i], f"b{i}."
            for nm in ("ln1", "ln2"):
                setattr(blk, f"{nm}_w", t[f"{p}{nm}.w"].data_ptr())
                setattr(blk, f"{nm}_b", t[f"{p}{nm}.b"].data_ptr())
            for nm in _LINEARS:
                setattr(blk, f"{nm}_w", t[f"{p}{nm}.w"].data_ptr())
                setattr(blk, f"{nm}_b", t[f"{p}{nm}.b"].data_ptr())
                setattr(blk, f"{nm}_h", t[f"{p}{nm}.wh"].data_ptr())
        return w

    def workspace(self, b: int, h: int, w: int) -> torch.Tensor:
        need = int(self.lib.gp_dino_workspace_size(b, h, w))
        if self.max_workspace_bytes is not None:
            need = min(need, max(int(self.max_workspace_bytes), int(self.lib.gp_dino_workspace_size(1, h, w))))
        if self._ws is None or self._ws.numel() != need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    @torch.no_grad()
    def get_intermediate_layers(self, x: torch.Tensor, n: Sequence[int] = arch.IMG_LAYERS, reshape: bool = False,
                                norm: bool = True, return_class_token: bool = False):
        """x (B, 3, H, W) float32 on the device -> a tuple of (B, H/16 * W/16, 384) tensors, one per layer of n."""
        if reshape or not norm or return_class_token:
            raise NotImplementedError("the device backbone is built for reshape=False, norm=True, "
                                      "return_class_token=False (the call of posenet.py:138-144)")
        if isinstance(n, int):
            raise NotImplementedError("n must list the blocks to take (an int n, 'the last n blocks', is not built)")
        layers = [int(v) for v in n]
        if not layers or any(v < 0 or v >= arch.DINO_BLOCKS for v in layers):
            raise NotImplementedError(f"layers {layers}: block indices 0..{arch.DINO_BLOCKS - 1}")
        x = require_device_tensor(x, "roi_rgb")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"roi_rgb must be (B, 3, H, W), got {tuple(x.shape)}")
        B, _, H, W = (int(v) for v in x.shape)
        P = arch.DINO_PATCH
        if B < 1 or H % P or W % P or H < P or W < P or (H // P) * (W // P) > arch.DINO_MAX_PATCHES:
            raise ValueError(f"roi_rgb {tuple(x.shape)}: B >= 1, H and W multiples of {P}, at most "
                             f"{arch.DINO_MAX_PATCHES} patches")
        hp, wp = H // P, W // P
        rope = self.rope_table(hp, wp)
        ws = self.workspace(B, H, W)
        outs = [torch.empty((B, hp * wp, arch.DINO_DIM), dtype=torch.float32, device=self.device) for _ in layers]
        wts = self._weights(rope, hp, wp)
        lay = (ctypes.c_int * len(layers))(*layers)
        ptrs = (ctypes.c_void_p * len(layers))(*[o.data_ptr() for o in outs])
        check(self.lib.gp_dino_forward(ctypes.byref(wts), vp(x), B, H, W, len(layers), lay, ptrs, ARITH[self.arith],
                                       vp(ws), ws.numel(), ctypes.c_void_p(stream_handle(self.device))),
              "dino_forward")
        self.calls += 1
        return tuple(outs)
