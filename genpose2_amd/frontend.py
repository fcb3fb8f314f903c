"""RGB-D front end: one camera frame -> the per-object batch the pose networks read (the counterpart of
datasets/datasets_infer.py ``InferDataset``; rules in DESIGN.md "RGB-D front end").

Everything per pixel runs on the device (csrc/gp_frontend.hip). The host reads device memory twice per frame:
the 256 x 5 mask statistics (the number of objects sizes the outputs) and the per-object counts of valid
points (fewer than 10 is an error, as in the reference).

``frames_objects`` / ``InferFrames`` take F frames of one size per call and give the objects of all of them as one
batch, with the same two host reads and one launch of each kernel whatever F (DESIGN.md "Several frames per call").
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


def _frames(x, name: str, dtype: torch.dtype, shape_tail) -> torch.Tensor:
    """A stacked (F,H,W,...) array or tensor, or a sequence of F per-frame ones, as one tensor where it lives;
    raises on frames of different sizes. Reads shapes only: no device is touched."""
    if isinstance(x, (list, tuple)):
        frames = [torch.as_tensor(a) for a in x]
        if not frames:
            raise ValueError(f"{name}: at least one frame is needed")
        if len({tuple(t.shape) for t in frames}) != 1:
            raise ValueError(f"{name}: the frames differ in size ({sorted({tuple(t.shape) for t in frames})}): "
                             f"one size per call")
        if len({t.device for t in frames}) != 1:
            frames = [t.cpu() for t in frames]
        t = torch.stack(frames)
    else:
        t = torch.as_tensor(x)
    if t.dtype != dtype and dtype == torch.uint8:
        raise TypeError(f"{name} must be uint8 (got {t.dtype})")
    if t.dim() != 3 + len(shape_tail) or tuple(t.shape[3:]) != tuple(shape_tail) or t.shape[0] < 1:
        raise ValueError(f"{name} must be (F, H, W{''.join(', %d' % s for s in shape_tail)}), got {tuple(t.shape)}")
    return t


def _per_frame(x, single, F: int, what: str) -> list:
    """One value for all frames, or a sequence of 1 or F of them -> a list of F."""
    xs = [x] if single(x) else list(x)
    if len(xs) not in (1, F):
        raise ValueError(f"{len(xs)} {what} for {F} frames: give one for all frames or one per frame")
    return xs * F if len(xs) == 1 else xs


def frames_mask_stats(mask: torch.Tensor) -> torch.Tensor:
    """gp_frames_mask_stats: (F,H,W) uint8 on the device -> (F,256,5) int32, ``mask_stats`` of every frame."""
    f, h, w = mask.shape
    stats = torch.empty((f, 256, 5), dtype=torch.int32, device=mask.device)
    check(_lib.load().gp_frames_mask_stats(_vp(mask), f, h, w, _vp(stats),
                                           ctypes.c_void_p(dev.stream_handle(mask.device))), "frames_mask_stats")
    return stats


@torch.no_grad()
def frames_objects(depth, color, mask, intrinsics, img_size: int = 224, n_pts: int = 1024, max_depth: float = 4.0,
                   seed=0, device: Union[str, torch.device] = "cuda") -> Dict[str, torch.Tensor]:
    """F frames of one size -> one batch of all their B = sum B_f objects, ordered by (frame, id): the keys of
    ``frame_objects`` with the bits it gives frame by frame, plus ``frame`` (B) int32 on the device and
    ``frame_offsets``, a host list of F + 1 ints (frame f's objects are rows frame_offsets[f]:frame_offsets[f+1]).

    depth (F,H,W), color (F,H,W,3), mask (F,H,W): stacked arrays or tensors, or sequences of F per-frame ones, on
    the host or the device; none is modified. ``intrinsics``: one camera for all frames or a sequence of F;
    ``seed``: an int for all frames or a sequence of F. One launch of each kernel and two device -> host reads
    (the (F,256,5) statistics, the B counts) per call, whatever F. A frame of background only contributes no rows.
    Raises ValueError for frames of different sizes, for a number of intrinsics or seeds that is neither 1 nor F,
    and naming every object ("frame f, object id i has c valid points") with fewer than 10 valid points."""
    mask = _frames(mask, "mask", torch.uint8, ())
    depth = _frames(depth, "depth", torch.float32, ())
    color = _frames(color, "color", torch.uint8, (3,))
    F, h, w = mask.shape
    if tuple(depth.shape) != (F, h, w) or tuple(color.shape[:3]) != (F, h, w):
        raise ValueError("depth, mask and color must have the same number of frames, height and width")
    cameras = _per_frame(intrinsics, lambda x: not isinstance(x, (list, tuple)), F, "intrinsics")
    seeds = _per_frame(seed, lambda x: isinstance(x, (int, np.integer)), F, "seeds")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the front end runs on a HIP device (got {device}); there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    S, n_pts = check_img_size(img_size), int(n_pts)
    if not 1 <= n_pts <= MAX_PTS:
        raise ValueError(f"n_pts must be in 1..{MAX_PTS}, got {n_pts}")
    if F > 65535:
        raise ValueError(f"at most 65535 frames per call, got {F}")
    intr_h = np.array([scaled_intrinsics(_intrinsics(c), h, w) for c in cameras], np.float32)
    if not (intr_h[:, :2] != 0).all():
        raise ValueError("zero focal length")
    seeds_h = np.array([[int(s) & 0xFFFFFFFF, (int(s) >> 32) & 0xFFFFFFFF] for s in seeds], np.uint32)
    mask = mask.to(device).contiguous()
    depth = depth.to(device, torch.float32).contiguous()
    color = color.to(device).contiguous()

    lib = _lib.load()
    with torch.cuda.device(device):
        st = ctypes.c_void_p(dev.stream_handle(device))
        stats_h = frames_mask_stats(mask).cpu().numpy()                          # host read 1
        per_frame = [crop_boxes(stats_h[f], h, w) for f in range(F)]
        offsets = [0]
        for ids_f, _ in per_frame:
            offsets.append(offsets[-1] + len(ids_f))
        B = offsets[-1]
        if B > 65535:
            raise ValueError(f"at most 65535 objects per call, got {B}")
        ids_h = np.concatenate([p[0] for p in per_frame]).astype(np.int32)
        frame_h = np.repeat(np.arange(F, dtype=np.int32), np.diff(offsets))
        # one upload: frame (B) | ids (B) | boxes (B,3) | intrinsics (F,4) | seeds (F,2), four bytes each
        packed = torch.from_numpy(np.concatenate(
            [frame_h, ids_h, np.concatenate([p[1] for p in per_frame]).astype(np.float32).ravel().view(np.int32),
             intr_h.ravel().view(np.int32), seeds_h.ravel().view(np.int32)])).to(device)
        frame, ids, boxes, intr, keys = torch.split(packed, [B, B, 3 * B, 4 * F, 2 * F])
        boxes, intr = boxes.view(torch.float32).view(B, 3), intr.view(torch.float32).view(F, 4)
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        pts = torch.empty((B, n_pts, 3), **f32)
        xs, ys = torch.empty((B, n_pts), **i32), torch.empty((B, n_pts), **i32)
        count = torch.empty((B,), **i32)
        roi_rgb = torch.empty((B, 3, S, S), **f32)
        if B == 0:   # background only in every frame: the empty batch, nothing to launch
            return {"pts": pts, "pts_color": pts, "pcl_in": pts, "roi_rgb": roi_rgb, "roi_xs": xs, "roi_ys": ys,
                    "zero_mean_pts": pts.clone(), "pts_center": torch.empty((0, 3), **f32), "ids": ids,
                    "count": count, "frame": frame, "frame_offsets": offsets}
        ws_bytes = int(lib.gp_frame_objects_workspace_size(B, S))
        ws = torch.empty((ws_bytes // 4,), **i32)
        check(lib.gp_frames_objects(_vp(depth), _vp(mask), F, h, w, _vp(frame), _vp(ids), _vp(boxes), B, S, n_pts,
                                    _vp(intr), float(max_depth), _vp(keys), _vp(pts), _vp(xs), _vp(ys), _vp(count),
                                    _vp(ws), ws_bytes, st), "frames_objects")
        check(lib.gp_frames_roi_rgb(_vp(color), F, h, w, _vp(frame), _vp(boxes), B, S, _vp(roi_rgb), st),
              "frames_roi_rgb")
        center = dev.points_mean(pts)
        zero_mean = pts - center.unsqueeze(1)
        count_h = count.cpu().numpy()                                            # host read 2
    few = [(int(f), int(i), int(c)) for f, i, c in zip(frame_h, ids_h, count_h) if c < MIN_VALID_POINTS]
    if few:
        raise ValueError("not enough points for pose estimation: " +
                         ", ".join(f"frame {f}, object id {i} has {c} valid points" for f, i, c in few) +
                         f" (at least {MIN_VALID_POINTS} are needed)")
    return {"pts": pts, "pts_color": pts, "pcl_in": pts, "roi_rgb": roi_rgb, "roi_xs": xs, "roi_ys": ys,
            "zero_mean_pts": zero_mean, "pts_center": center, "ids": ids, "count": count, "frame": frame,
            "frame_offsets": offsets}


class InferFrames:
    """``InferDataset`` for a sequence of F ``data`` dictionaries (``depth``, ``color``, ``mask``, ``meta``), all
    frames of one size. ``get_objects()`` is ``frames_objects``; ``seeds`` (an attribute: one per frame, 0 by
    default) key the point samples."""

    def __init__(self, datas, img_size: int = 224, device="cuda", n_pts: int = 1024):
        self._datas = list(datas)
        if not self._datas:
            raise ValueError("InferFrames needs at least one frame")
        self._img_size, self._device, self._n_pts = img_size, device, n_pts
        self.seeds = [0] * len(self._datas)
        self.max_depth = 4.0

    def __len__(self) -> int:
        return len(self._datas)

    def get_objects(self) -> Dict[str, torch.Tensor]:
        return frames_objects(*([d[k] for d in self._datas] for k in ("depth", "color", "mask")),
                              [d["meta"] for d in self._datas], img_size=self._img_size, n_pts=self._n_pts,
                              max_depth=self.max_depth, seed=self.seeds, device=self._device)


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
