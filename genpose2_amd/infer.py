"""Frame in, poses and sizes out: the counterpart of runners/infer.py ``GenPose2``.

``GenPose2.inference(data, prev_pose, tracking, tracking_T0)`` runs the front end (frontend.frame_objects) once
and the ``EvaluationPipeline`` stages on its batch: score sampling (warm-started from ``prev_pose``), energy
ranking with get_energy(T=None), aggregation, size. The reference calls ``get_objects()`` once per stage, so its
EnergyNet and size stage see a fresh random sample of the points; here every stage reads the same sample.
``GenPose2.inference_frames`` does the same for several frames in one call (frontend.frames_objects): one front
end, one pipeline run on the objects of all frames, the results split by frame.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import arch, device as dev
from .aggregate import MAX_MODES, PoseModes
from .config import GenPoseConfig
from .frontend import InferDataset, InferFrames
from .runner import EvaluationPipeline


def default_config(**kw) -> GenPoseConfig:
    """runners/infer.py:78-90: the ODE sampler from T0 = 0.55, 50 candidates, seed 0. ``dino`` stays 'none' by
    default; the reference's shipped configuration is ``default_config(dino="pointwise")`` with checkpoints that
    carry the DINOv3 backbone ("dino." keys, or ``PoseNet.load_dino``) and ``InferDataset(..., img_size=256)``:
    the backbone then runs on device on the frame's ``roi_rgb`` (genpose2_amd/dino.py)."""
    base = dict(sampler_mode=["ode"], T0=0.55, seed=0, eval_repeat_num=50, dino="none")
    base.update(kw)
    return GenPoseConfig(**base)


def pose_representation(pose: torch.Tensor) -> torch.Tensor:
    """(B,4,4) [R t; 0 1] -> (B,9) [R[:, :, 0] | R[:, :, 1] | t] (utils/misc.py get_pose_representation for
    rot_matrix, then the translation)."""
    return torch.cat([pose[:, :3, 0], pose[:, :3, 1], pose[:, :3, 3]], dim=-1)


class GenPose2:
    """``score_model_path`` / ``energy_model_path`` / ``scale_model_path``: reference checkpoints. A ``None``
    score or energy path keeps that agent's synthetic weights (as ``PoseNet`` does); without a scale path there
    is no ScaleNet and the size is the points' bounding box in the estimated frame."""

    def __init__(self, score_model_path: Optional[str], energy_model_path: Optional[str] = None,
                 scale_model_path: Optional[str] = None, cfg: Optional[GenPoseConfig] = None):
        cfg = default_config() if cfg is None else cfg
        self.cfg = cfg.copy(pretrained_score_model_path=score_model_path,
                            pretrained_energy_model_path=energy_model_path,
                            pretrained_scale_model_path=scale_model_path)
        self.cfg.validate()
        self.pipeline = EvaluationPipeline(self.cfg, with_energy=True, with_scale=scale_model_path is not None)
        for agent, path in ((self.score_agent, score_model_path), (self.energy_agent, energy_model_path),
                            (self.scale_agent, scale_model_path)):
            if agent is not None and path is not None:
                agent.load_ckpt(model_dir=path, model_path=True, load_model_only=True)

    score_agent = property(lambda self: self.pipeline.score_agent)
    energy_agent = property(lambda self: self.pipeline.energy_agent)
    scale_agent = property(lambda self: self.pipeline.scale_agent)

    @staticmethod
    def check_pointwise_size(h: int, w: int) -> None:
        """--dino pointwise: the ImgEncoder is built for 256 patches, so the backbone's input must be 16 x 16
        patches of 16 pixels."""
        h, w = int(h), int(w)
        if h % arch.DINO_PATCH or w % arch.DINO_PATCH or \
                (h // arch.DINO_PATCH) * (w // arch.DINO_PATCH) != arch.IMG_PATCHES:
            raise ValueError(f"dino='pointwise' needs roi_rgb of {arch.IMG_PATCHES} patches of {arch.DINO_PATCH} pixels "
                             f"(256 x 256), got {h} x {w}: build the frame with InferDataset(..., img_size=256) "
                             f"(or frame_objects(..., img_size=256))")

    @torch.no_grad()
    def inference(self, data: Union[InferDataset, Dict[str, torch.Tensor]], prev_pose=None, tracking: bool = False,
                  tracking_T0: float = 0.15) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (final_pose (B,4,4), final_length (B,3)), objects in ascending mask id (runners/infer.py:276-310).

        ``data``: an ``InferDataset`` (its ``get_objects()`` runs once) or a batch ``frame_objects`` returned.
        ``prev_pose`` (B,4,4) (or the reference's one-element list of it) warm-starts the sampler at
        [R[:, 0] | R[:, 1] | t - pts_center]; the start time is ``tracking_T0`` only when ``tracking`` is set as
        well, else cfg.T0 -- as the reference does."""
        return self._inference(data, prev_pose, tracking, tracking_T0)[:2]

    @torch.no_grad()
    def inference_modes(self, data: Union[InferDataset, Dict[str, torch.Tensor]], prev_pose=None,
                        tracking: bool = False, tracking_T0: float = 0.15, max_modes: int = 4,
                        follow_prev: bool = False) -> Tuple[torch.Tensor, torch.Tensor, PoseModes]:
        """``inference`` with the pose hypotheses -> (final_pose, final_length, ``aggregate.PoseModes``): up to
        ``max_modes`` (1..8) rotation clusters per object, from the aggregation's own launch.

        With ``follow_prev`` and a ``prev_pose``, each object's final rotation is that of the slot nearest to its
        previous rotation (``PoseModes.nearest``, picked on the device) and the size is estimated in that frame;
        the translation stays the aggregated one. Without it the first two results are ``inference``'s bits."""
        if not 1 <= int(max_modes) <= MAX_MODES:
            raise ValueError(f"max_modes must be 1..{MAX_MODES}, got {max_modes}")
        return self._inference(data, prev_pose, tracking, tracking_T0, int(max_modes), follow_prev)

    def _inference(self, data, prev_pose, tracking: bool, tracking_T0: float, max_modes: int = 0,
                   follow_prev: bool = False):
        """-> (final_pose, final_length, PoseModes or None): the body of ``inference`` and ``inference_modes``."""
        if self.cfg.dino == "pointwise" and hasattr(data, "get_objects") and hasattr(data, "_img_size"):
            self.check_pointwise_size(data._img_size, data._img_size)   # before the front end launches anything
        batch = data.get_objects() if hasattr(data, "get_objects") else data
        if self.cfg.dino == "pointwise" and batch.get("dino_layers") is None \
                and batch.get("point_rgb_feat") is None and batch.get("roi_rgb") is not None:
            self.check_pointwise_size(*batch["roi_rgb"].shape[-2:])
        pts = batch["pts"]
        B = int(pts.shape[0])
        if B == 0:
            return pts.new_zeros((0, 4, 4)), pts.new_zeros((0, 3)), \
                (PoseModes.empty(0, max_modes, pts.device) if max_modes else None)
        init_x = None
        if prev_pose is not None:
            if isinstance(prev_pose, (list, tuple)):
                if len(prev_pose) != 1:
                    raise ValueError("prev_pose as a list holds one (B,4,4) tensor: one frame per call")
                prev_pose = prev_pose[0]
            prev_pose = torch.as_tensor(prev_pose).to(pts.device, torch.float32)
            if tuple(prev_pose.shape) != (B, 4, 4):
                raise ValueError(f"prev_pose must be ({B},4,4), got {tuple(prev_pose.shape)}")
            init_x = pose_representation(prev_pose)
            init_x[:, -3:] -= batch["pts_center"]
        T0 = tracking_T0 if tracking and prev_pose is not None else None
        if max_modes:
            prev_rot = prev_pose[:, :3, :3].contiguous() if prev_pose is not None else None
            out = self.pipeline.run(batch, init_x=init_x, T0=T0, energy_T=None, max_modes=max_modes,
                                    prev_rot=prev_rot, follow_prev=follow_prev)
        else:
            out = self.pipeline.run(batch, init_x=init_x, T0=T0, energy_T=None)
        final_pose = out.aggregated
        length = out.length if out.length is not None else dev.bbox_length(pts, final_pose)
        return final_pose, length, out.modes

    @torch.no_grad()
    def inference_frames(self, data: Union[InferFrames, Dict[str, torch.Tensor]],
                         prev_pose: Optional[Sequence[torch.Tensor]] = None, tracking: bool = False,
                         tracking_T0: float = 0.15) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """``inference`` for F frames in one call -> a list of F pairs (final_pose (B_f,4,4), final_length (B_f,3)),
        each frame's objects in ascending mask id; a frame of background only gives empty tensors.

        ``data``: an ``InferFrames`` (its ``get_objects()`` runs once) or a batch ``frames_objects`` returned. The
        front end and ``pipeline.run`` run once on the B = sum B_f objects of all frames, and the results are split
        by the batch's ``frame_offsets``. ``prev_pose``: ``None`` or a sequence of F tensors (B_f,4,4), a warm start
        for every object (for none: ``None``); start time and crop-size check as in ``inference``.

        It runs under ``self.cfg``. With ``ode_coupling="object"`` (or ``pc_coupling="object"`` for the PC sampler)
        an object's candidates do not depend on which frames share the call; with the default ``"batch"`` coupling
        they do, exactly as they already depend on the other objects of one frame (the step controller's error norm
        and the Langevin step size are taken over the whole batch). Under either coupling an object's prior noise
        is its rows of the whole call's draw: to reproduce a frame's objects in a call of their own, give the score
        agent ``object_window = (B, frame_offsets[f])``."""
        batch, offsets, prev_pose = self._frames_batch(data, prev_pose)
        pose, length, _ = self._inference(batch, prev_pose, tracking, tracking_T0)
        return [(pose[lo:hi], length[lo:hi]) for lo, hi in zip(offsets[:-1], offsets[1:])]

    @torch.no_grad()
    def inference_frames_modes(self, data: Union[InferFrames, Dict[str, torch.Tensor]],
                               prev_pose: Optional[Sequence[torch.Tensor]] = None, tracking: bool = False,
                               tracking_T0: float = 0.15, max_modes: int = 4, follow_prev: bool = False
                               ) -> List[Tuple[torch.Tensor, torch.Tensor, PoseModes]]:
        """``inference_modes`` for F frames in one call, as ``inference_frames`` does it for ``inference``: a list
        of F triples (final_pose, final_length, PoseModes), the hypotheses split by ``frame_offsets`` too."""
        if not 1 <= int(max_modes) <= MAX_MODES:
            raise ValueError(f"max_modes must be 1..{MAX_MODES}, got {max_modes}")
        batch, offsets, prev_pose = self._frames_batch(data, prev_pose)
        pose, length, modes = self._inference(batch, prev_pose, tracking, tracking_T0, int(max_modes), follow_prev)
        return [(pose[lo:hi], length[lo:hi], m)
                for lo, hi, m in zip(offsets[:-1], offsets[1:], modes.split(offsets))]

    def _frames_batch(self, data, prev_pose):
        """-> (the batch of all frames, its frame offsets, prev_pose as one (B,4,4) tensor or None)."""
        if self.cfg.dino == "pointwise" and hasattr(data, "get_objects") and hasattr(data, "_img_size"):
            self.check_pointwise_size(data._img_size, data._img_size)   # before the front end launches anything
        batch = data.get_objects() if hasattr(data, "get_objects") else data
        if "frame_offsets" not in batch:
            raise ValueError("inference_frames takes an InferFrames or a batch of frames_objects (with frame_offsets)")
        offsets = [int(o) for o in batch["frame_offsets"]]
        F = len(offsets) - 1
        if prev_pose is not None:
            prev_pose = list(prev_pose)
            if len(prev_pose) != F:
                raise ValueError(f"prev_pose holds {len(prev_pose)} tensors for {F} frames: one (B_f,4,4) per frame")
            device = batch["pts"].device
            prev_pose = [torch.as_tensor(p).to(device, torch.float32) for p in prev_pose]
            for f, p in enumerate(prev_pose):
                if tuple(p.shape) != (offsets[f + 1] - offsets[f], 4, 4):
                    raise ValueError(f"prev_pose of frame {f} must be ({offsets[f + 1] - offsets[f]},4,4), "
                                     f"got {tuple(p.shape)}")
            prev_pose = torch.cat(prev_pose)
        return batch, offsets, prev_pose


def create_genpose2(score_model_path: Optional[str], energy_model_path: Optional[str] = None,
                    scale_model_path: Optional[str] = None, cfg: Optional[GenPoseConfig] = None) -> GenPose2:
    return GenPose2(score_model_path, energy_model_path, scale_model_path, cfg)
