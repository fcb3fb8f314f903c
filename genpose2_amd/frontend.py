"""RGB-D front end: one camera frame -> the per-object batch the pose networks read (the counterpart of
datasets/datasets_infer.py ``InferDataset``; rules in DESIGN.md "RGB-D front end").

Everything per pixel runs on the device (csrc/gp_frontend.hip). The host reads device memory twice per frame:
the 256 x 5 mask statistics (the number of objects sizes the outputs) and the per-object counts of valid
points (fewer than 10 is an error, as in the reference).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Mapping, Union

import numpy as np
import torch

from . import _lib
from . import device as dev
from ._lib import check

MAX_PTS = 2048
MIN_VALID_POINTS = 10
_KEYS = ("fx", "fy", "cx", "cy", "width", "height")


def _vp(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _intrinsics(intrinsics) -> Dict[str, float]:
    """fx, fy, cx, cy, width, height from a mapping or an object with those attributes; the reference's
    meta dictionary (meta["camera"]["intrinsics"]) is accepted too."""
    if isinstance(intrinsics, Mapping) and "camera" in intrinsics:
        intrinsics = intrinsics["camera"]["intrinsics"]
    elif hasattr(intrinsics, "camera"):
        intrinsics = intrinsics.camera.intrinsics
    if isinstance(intrinsics, Mapping):
        return {k: float(intrinsics[k]) for k in _KEYS}
    return {k: float(getattr(intrinsics, k)) for k in _KEYS}


def _image(x, name: str, dtype: torch.dtype, shape_tail, device: torch.device) -> torch.Tensor:
    t = torch.as_tensor(x)
    if t.dtype != dtype:
        if dtype == torch.uint8:
            raise TypeError(f"{name} must be uint8 (got {t.dtype})")
        t = t.to(dtype)
    t = t.to(device).contiguous()
    if t.dim() != 2 + len(shape_tail) or tuple(t.shape[2:]) != tuple(shape_tail):
        raise ValueError(f"{name} must be (H, W{''.join(', %d' % s for s in shape_tail)}), got {tuple(t.shape)}")
    return t


def mask_stats(mask: torch.Tensor) -> torch.Tensor:
    """gp_frame_mask_stats: (H,W) uint8 on the device -> (256,5) int32 {count, rmin, rmax, cmin, cmax}."""
    h, w = mask.shape
    stats = torch.empty((256, 5), dtype=torch.int32, device=mask.device)
    check(_lib.load().gp_frame_mask_stats(_vp(mask), h, w, _vp(stats), ctypes.c_void_p(dev.stream_handle(mask.device))),
          "frame_mask_stats")
    return stats


def crop_boxes(stats_host: np.ndarray, h: int, w: int):
    """gp_frame_crop_boxes (host): -> ids (B) int32, boxes (B,3) float32 (centre x, centre y, scale)."""
    stats_host = np.ascontiguousarray(stats_host, np.int32)
    if stats_host.shape != (256, 5):
        raise ValueError(f"stats must be (256, 5), got {stats_host.shape}")
    ids = np.zeros(255, np.int32)
    boxes = np.zeros((255, 3), np.float32)
    n = ctypes.c_int(0)
    check(_lib.load().gp_frame_crop_boxes(stats_host.ctypes.data_as(ctypes.c_void_p), h, w,
                                          ids.ctypes.data_as(ctypes.c_void_p), boxes.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.cast(ctypes.byref(n), ctypes.c_void_p)), "frame_crop_boxes")
    return ids[:n.value].copy(), boxes[:n.value].copy()


def scaled_intrinsics(intr: Dict[str, float], h: int, w: int):
    """The float32 intrinsics times W / width and H / height, in float32 (datasets_infer.py:70-80)."""
    sx, sy = np.float32(w / intr["width"]), np.float32(h / intr["height"])
    return (float(np.float32(intr["fx"]) * sx), float(np.float32(intr["fy"]) * sy),
            float(np.float32(intr["cx"]) * sx), float(np.float32(intr["cy"]) * sy))


def check_img_size(img_size) -> int:
    """The crop size rule: a positive multiple of 14 (the reference's 224: 16 x 16 windows of 14 pixels for the
    patch -> point gather) or of 16 (256: what the DINOv3 backbone of --dino pointwise needs, 16 x 16 patches)."""
    S = int(img_size)
    if S < 14 or (S % 14 != 0 and S % 16 != 0):
        raise ValueError(f"img_size must be a positive multiple of 14 or of 16, got {img_size}")
    return S


@torch.no_grad()
def frame_objects(depth, color, mask, intrinsics, img_size: int = 224, n_pts: int = 1024, max_depth: float = 4.0,
                  seed: int = 0, device: Union[str, torch.device] = "cuda") -> Dict[str, torch.Tensor]:
    """One frame -> the batch of ``InferDataset.get_objects()``: pts = pts_color = pcl_in (B,n_pts,3), roi_rgb
    (B,3,S,S), roi_xs / roi_ys (B,n_pts) int32 (crop row / column), zero_mean_pts, pts_center (B,3), plus ids (B)
    and count (B). Usable as ``data`` of ``PoseNet.pred_func`` and ``batch`` of ``EvaluationPipeline.run``.

    depth (H,W) float32 metres, color (H,W,3) uint8, mask (H,W) uint8 (255 = background, any other value an object
    id): numpy arrays or tensors, on the host or the device; none is modified. Raises ValueError naming the id
    of an object with fewer than 10 valid points."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the front end runs on a HIP device (got {device}); there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    S, n_pts = check_img_size(img_size), int(n_pts)
    if not 1 <= n_pts <= MAX_PTS:
        raise ValueError(f"n_pts must be in 1..{MAX_PTS}, got {n_pts}")
    mask = _image(mask, "mask", torch.uint8, (), device)
    h, w = mask.shape
    depth = _image(depth, "depth", torch.float32, (), device)
    color = _image(color, "color", torch.uint8, (3,), device)
    if tuple(depth.shape) != (h, w) or tuple(color.shape[:2]) != (h, w):
        raise ValueError("depth, mask and color must have the same height and width")
    fx, fy, cx, cy = scaled_intrinsics(_intrinsics(intrinsics), h, w)

    lib = _lib.load()
    with torch.cuda.device(device):
        st = ctypes.c_void_p(dev.stream_handle(device))
        ids_h, boxes_h = crop_boxes(mask_stats(mask).cpu().numpy(), h, w)       # host read 1
        B = len(ids_h)
        ids = torch.from_numpy(ids_h).to(device)
        boxes = torch.from_numpy(boxes_h).to(device)
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        pts = torch.empty((B, n_pts, 3), **f32)
        xs, ys = torch.empty((B, n_pts), **i32), torch.empty((B, n_pts), **i32)
        count = torch.empty((B,), **i32)
        roi_rgb = torch.empty((B, 3, S, S), **f32)
        if B == 0:   # a frame of background only: an empty batch, nothing to launch
            return {"pts": pts, "pts_color": pts, "pcl_in": pts, "roi_rgb": roi_rgb, "roi_xs": xs, "roi_ys": ys,
                    "zero_mean_pts": pts.clone(), "pts_center": torch.empty((0, 3), **f32), "ids": ids,
                    "count": count}
        ws_bytes = int(lib.gp_frame_objects_workspace_size(B, S))
        ws = torch.empty((ws_bytes // 4,), **i32)
        check(lib.gp_frame_objects(_vp(depth), _vp(mask), h, w, _vp(ids), _vp(boxes), B, S, n_pts, fx, fy, cx, cy,
                                   float(max_depth), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _vp(pts),
                                   _vp(xs), _vp(ys), _vp(count), _vp(ws), ws_bytes, st), "frame_objects")
        check(lib.gp_frame_roi_rgb(_vp(color), h, w, _vp(boxes), B, S, _vp(roi_rgb), st), "frame_roi_rgb")
        center = dev.points_mean(pts)
        zero_mean = pts - center.unsqueeze(1)
        count_h = count.cpu().numpy()                                            # host read 2
    few = [(int(i), int(c)) for i, c in zip(ids_h, count_h) if c < MIN_VALID_POINTS]
    if few:
        raise ValueError("not enough points for pose estimation: " +
                         ", ".join(f"object id {i} has {c} valid points" for i, c in few) +
                         f" (at least {MIN_VALID_POINTS} are needed)")
    return {"pts": pts, "pts_color": pts, "pcl_in": pts, "roi_rgb": roi_rgb, "roi_xs": xs, "roi_ys": ys,
            "zero_mean_pts": zero_mean, "pts_center": center, "ids": ids, "count": count}


class InferDataset:
    """The reference's ``InferDataset(data, img_size=224, device='cuda', n_pts=1024)``: ``data`` holds ``depth``,
    ``color``, ``mask`` and ``meta`` (the camera intrinsics: the reference's meta dictionary, a mapping with fx,
    fy, cx, cy, width, height, or an object with those attributes). ``get_objects()`` is ``frame_objects``; ``seed``
    (an attribute, 0 by default) keys the point sample."""

    def __init__(self, data: dict, img_size: int = 224, device="cuda", n_pts: int = 1024):
        self._depth, self._color, self._mask, self._meta = data["depth"], data["color"], data["mask"], data["meta"]
        self._img_size, self._device, self._n_pts = img_size, device, n_pts
        self.seed = 0
        self.max_depth = 4.0

    def get_objects(self) -> Dict[str, torch.Tensor]:
        return frame_objects(self._depth, self._color, self._mask, self._meta, img_size=self._img_size,
                             n_pts=self._n_pts, max_depth=self.max_depth, seed=self.seed, device=self._device)
