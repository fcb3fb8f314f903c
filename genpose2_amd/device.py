"""Device-resident models: packed weights in HBM + thin calls into libgenpose_hip.so.

PyTorch is used only for device memory, the current HIP stream and host<->device copies; every
computation on the path is a call into the HIP library.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, arch, pack, weights
from ._lib import check


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device_tensor(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a HIP device (got {t.device}); the path has no CPU fallback")
    return t.to(dtype).contiguous()


class _Uploaded:
    def __init__(self, arrays: Dict[str, np.ndarray], device: torch.device):
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in arrays.items()}

    def ptr(self, k: str) -> int:
        return self.t[k].data_ptr()


class EncoderGeometry:
    """Geometry of one point batch in an encoder workspace (EncoderModel.geometry): valid until the producing
    model recomputes geometry in that workspace (its next geometry() or forward() without a geometry), which
    forward(geometry=...) detects through the producer's generation counter; ``event`` marks its completion on
    the producing stream. Refilling the points tensor in place also invalidates it (not detectable: the key is
    the tensor's address and shape). ``event0`` (or None) marks level 0's geometry alone: levels 1-3 were
    computed on a side stream after it, so a consumer can start level 0 before they are done."""

    def __init__(self, ws: torch.Tensor, event, key, producer=None, gen: int = 0, event0=None):
        self.ws, self.event, self.key = ws, event, key   # key: (points tensor address, (B, N))
        self.producer, self.gen = producer, gen
        self.event0 = event0


class EncoderModel:
    """Pointnet2ClsMSG(0), Light cfg, on device (gp_encoder_forward)."""

    def __init__(self, sd: weights.StateDict, device: torch.device):
        self.lib = _lib.load()
        self.device = device
        buf, offs = pack.pack_encoder(sd)
        self.wbuf = torch.from_numpy(buf).to(device)
        self._table = np.ascontiguousarray(offs, np.int64)     # [5][2][3][4] (gp_encoder_forward)
        self._ws: Optional[torch.Tensor] = None
        self._gen = 0   # bumped whenever this model writes geometry into its workspace
        # geometry(): levels 1-3 of the FPS chain and ball lists on a side stream, beside level 0's MLPs
        self.geometry_overlap = os.environ.get("GENPOSE2_GEOM_OVERLAP", "1") == "1"
        self._geo_stream: Optional[torch.cuda.Stream] = None
        # completion of the last side-stream geometry write into self._ws: every later write into the
        # workspace (geometry() again, forward() without a geometry) is ordered after it on its stream
        self._geo_event: Optional[torch.cuda.Event] = None
        self.set_arith(os.environ.get("GENPOSE2_ENC_ARITH", "split_f16"))

    @property
    def table(self) -> np.ndarray:
        """The host layer table [5][2][3][4] (offsets and split-f16 exponents derived from the weight
        values): part of the model's state beside ``wbuf``, so a weight broadcast carries it too."""
        return self._table

    def set_table(self, table: np.ndarray) -> None:
        table = np.ascontiguousarray(table, np.int64).reshape(self._table.shape)
        self._table = table
        self.set_arith(self.arith)

    def set_arith(self, arith: str) -> None:
        """GEMM arithmetic of SA levels 1-3 and GroupAll: "split_f16" (f16 hi/lo MFMA products with
        per-column activation scaling: sa_narrow_kernel, sa_split_kernel, tok_split_gemm_kernel)
        or "f32" (exact fp32 MFMA)."""
        if arith not in ("split_f16", "f32"):
            raise ValueError(f"unknown encoder arithmetic {arith!r} (split_f16 | f32)")
        t = self._table.copy()
        if arith == "f32":
            t[..., 2] = -1
        self.arith = arith
        self.offsets = np.ascontiguousarray(t.reshape(-1), np.int64)

    def workspace(self, b: int, n: int) -> torch.Tensor:
        need = int(self.lib.gp_encoder_workspace_size(b, n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _after_side_writes(self, cur) -> None:
        """Order the current stream after this model's outstanding side-stream geometry writes."""
        if self._geo_event is not None:
            cur.wait_event(self._geo_event)

    @staticmethod
    def _xyz(pts: torch.Tensor) -> torch.Tensor:
        pts = require_device_tensor(pts, "pts")
        if pts.dim() != 3 or pts.shape[2] < 3:
            raise ValueError("pts must be (B, N, 3+)")
        return pts if pts.shape[2] == 3 else pts[..., :3].contiguous()

    def geometry(self, pts: torch.Tensor) -> "EncoderGeometry":
        """FPS indices, centroids and ball lists of every level (gp_encoder_geometry) into this model's
        workspace, for this model and any other encoder of the same points (forward(geometry=...))."""
        key = (require_device_tensor(pts, "pts").data_ptr(), tuple(pts.shape[:2]))
        pts = self._xyz(pts)
        B, N, _ = pts.shape
        ws = self.workspace(B, N)
        self._gen += 1
        cur = torch.cuda.current_stream(self.device)
        self._after_side_writes(cur)
        if not self.geometry_overlap:
            check(self.lib.gp_encoder_geometry(ctypes.c_void_p(pts.data_ptr()), B, N, ctypes.c_void_p(ws.data_ptr()),
                                               ws.numel(), ctypes.c_void_p(cur.cuda_stream)), "encoder_geometry")
            ev = torch.cuda.Event()
            ev.record(cur)
            return EncoderGeometry(ws, ev, key, self, self._gen)
        # level 0 here; levels 1-3 (their FPS reads level 0's centroids) on the side stream after it
        check(self.lib.gp_encoder_geometry_levels(ctypes.c_void_p(pts.data_ptr()), B, N, ctypes.c_void_p(ws.data_ptr()),
                                                  ws.numel(), 0, 1, ctypes.c_void_p(cur.cuda_stream)),
              "encoder_geometry level 0")
        ev0 = torch.cuda.Event()
        ev0.record(cur)
        if self._geo_stream is None:
            self._geo_stream = torch.cuda.Stream(device=self.device)
        side = self._geo_stream
        side.wait_event(ev0)
        check(self.lib.gp_encoder_geometry_levels(ctypes.c_void_p(pts.data_ptr()), B, N, ctypes.c_void_p(ws.data_ptr()),
                                                  ws.numel(), 1, 4, ctypes.c_void_p(side.cuda_stream)),
              "encoder_geometry levels 1-3")
        ws.record_stream(side)
        pts.record_stream(side)
        ev = torch.cuda.Event()
        ev.record(side)
        self._geo_event = ev
        return EncoderGeometry(ws, ev, key, self, self._gen, event0=ev0)

    def forward(self, pts: torch.Tensor, return_workspace: bool = False,
                geometry: Optional["EncoderGeometry"] = None):
        """geometry: from geometry() on the same points (this model's or another encoder's); the call then
        runs only the per-level MLPs (gp_encoder_forward_geom), after the stream waits for it."""
        key = (require_device_tensor(pts, "pts").data_ptr(), tuple(pts.shape[:2]))
        pts = self._xyz(pts)
        B, N, _ = pts.shape
        feat = torch.empty((B, arch.PTS_FEAT_DIM), dtype=torch.float32, device=self.device)
        ws = self.workspace(B, N)
        self._after_side_writes(torch.cuda.current_stream(self.device))
        st = ctypes.c_void_p(stream_handle(self.device))
        if geometry is None:
            self._gen += 1   # the self-contained pass rewrites the geometry in this workspace
            check(self.lib.gp_encoder_forward(
                ctypes.c_void_p(self.wbuf.data_ptr()), self.offsets.ctypes.data_as(_lib.c_int64_p),
                ctypes.c_void_p(pts.data_ptr()), B, N, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                ctypes.c_void_p(feat.data_ptr()), st), "encoder_forward")
        else:
            if geometry.key != key:
                raise ValueError("encoder geometry was computed for other points")
            if geometry.producer is not None and geometry.producer._gen != geometry.gen:
                raise ValueError("encoder geometry is stale: its model encoded other points since")
            cur = torch.cuda.current_stream(self.device)
            # level 0 may start once its own geometry is there (event0), levels 1-4 after all of it
            spans = ((0, 1, geometry.event0), (1, 5, geometry.event)) if geometry.event0 is not None else \
                ((0, 5, geometry.event),)
            for first, last, ev in spans:
                cur.wait_event(ev)
                check(self.lib.gp_encoder_forward_geom_levels(
                    ctypes.c_void_p(self.wbuf.data_ptr()), self.offsets.ctypes.data_as(_lib.c_int64_p),
                    ctypes.c_void_p(pts.data_ptr()), B, N, ctypes.c_void_p(geometry.ws.data_ptr()),
                    ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(feat.data_ptr()), first, last, st),
                    "encoder_forward_geom")
            if geometry.ws is not ws:
                geometry.ws.record_stream(torch.cuda.current_stream(self.device))
        return (feat, ws) if return_workspace else feat

    def levels(self, b: int, n: int, ws: torch.Tensor):
        """Views of the per-level intermediates in the workspace (for parity tests)."""
        off = np.zeros(25, np.int64)
        check(self.lib.gp_encoder_workspace_layout(b, n, off.ctypes.data_as(_lib.c_int64_p)))
        out = []
        couts = [arch.level_out_channels(lv) for lv in range(5)]
        for lv in range(5):
            m = arch.NPOINTS[lv] if lv < 4 else 1
            d = {}
            if lv < 4:
                d["fps_idx"] = ws[off[lv * 5]:].view(torch.int32)[: b * m].view(b, m)
                d["new_xyz"] = ws[off[lv * 5 + 1]:].view(torch.float32)[: b * m * 3].view(b, m, 3)
                d["ball_idx"] = [ws[off[lv * 5 + 2 + i]:].view(torch.int32)[: b * m * ns].view(b, m, ns)
                                 for i, ns in enumerate(arch.NSAMPLES[lv])]
            if lv < 4:
                d["features"] = ws[off[lv * 5 + 4]:].view(torch.float32)[: b * m * couts[lv]].view(b, m, couts[lv])
            out.append(d)
        return out


PC_SMALL_DEFAULT = "auto"   # form of the PC step's three smallest products when GENPOSE2_PC_SMALL is unset


class HeadModel:
    """PoseScoreNet / PoseEnergyNet heads (Rx_Ry_and_T) on device."""

    def __init__(self, sd: weights.StateDict, device: torch.device):
        self.lib = _lib.load()
        self.device = device
        self.up = _Uploaded(pack.pack_heads(sd), device)
        # GENPOSE2_PC_SMALL=f16|fp8|auto, read once here: the form of the PC step's three smallest products
        # (set_pc_small)
        self.pc_small = os.environ.get("GENPOSE2_PC_SMALL") or PC_SMALL_DEFAULT
        if self.pc_small not in ("f16", "fp8", "auto"):
            raise ValueError(f"GENPOSE2_PC_SMALL={self.pc_small!r} (f16 | fp8 | auto)")
        self.set_arith(os.environ.get("GENPOSE2_HEAD_ARITH", "f16x3"))
        self._pc_ws: Optional[torch.Tensor] = None
        self._ode_obj_ws: Optional[torch.Tensor] = None
        self._like_obj_ws: Optional[torch.Tensor] = None
        self._gw = None                                    # (buffers, HeadGradWeights)

    def weights_changed(self) -> None:
        """Drop what was derived from the uploaded buffers' contents. Whoever rewrites ``up.t`` in place calls
        this (shard.broadcast_agent does): a collective's write does not show in a tensor's version counter, so
        nothing here could notice it."""
        self._gw = None

    @property
    def grad_weights(self) -> "_lib.HeadGradWeights":
        """The transposed pose-path weights of the energy gradient's reverse pass (pack.pack_heads_grad's bytes),
        made the first time an energy-gradient call needs them: the uploaded forward fragments re-tiled on the
        device (a copy, no arithmetic). Kept until weights_changed()."""
        if self._gw is None:
            src = [self.up.t[k] for k in ("pe0_w", "pe2_w", "h1p_w")]
            bufs = {}
            for name, t, n_out, k_in in zip(pack.HEAD_GRAD_FIELDS, src, (arch.POSE_HID, arch.POSE_HID, 3 * arch.HEAD_HID),
                                            (16, arch.POSE_HID, arch.POSE_HID)):
                # A fragments [T][g][q][i][j] -> W (n_out, k_in) -> fragments of W^T
                w = t.view(n_out // 16, k_in // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(n_out, k_in)
                bufs[name] = w.t().reshape(k_in // 16, 16, n_out // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)
            self._gw = (bufs, _lib.HeadGradWeights(**{k: v.data_ptr() for k, v in bufs.items()}))
        return self._gw[1]

    def set_arith(self, arith: str) -> None:
        """Per-candidate GEMM arithmetic of every head kernel (PC step, score/energy eval, ODE stages):
        "f16x3" (pose_encoder.2 and head layer 1's pose block on f16 MFMA with three planes per operand
        and six products: every bit of the fp32 operands, products to ~2^-33, fp32 accumulation;
        gp_head.h) or "f32" (exact fp32 MFMA, v_mfma_f32_16x16x4_f32)."""
        if arith not in ("f16x3", "f32"):
            raise ValueError(f"unknown head arithmetic {arith!r} (f16x3 | f32)")
        ptrs = {k: self.up.ptr(k) for k in pack.HEAD_FIELDS}
        if arith == "f32":
            ptrs.update(pe2_h=None, h1p_h=None, hsc=None)
        elif self.pc_small != "f16":   # _lib.HeadWeights.q8_flags: 1 score() follows, 2 every tile width
            ptrs.update({k: self.up.ptr(k) for k in pack.HEAD_Q8_FIELDS}, q8_flags=3 if self.pc_small == "fp8" else 1)
        self.arith = arith
        self.w = _lib.HeadWeights(**ptrs)

    def set_pc_small(self, form: str) -> None:
        """The PC step's products of plane order 2 (w_hi*a_lo, w_mid*a_mid, w_lo*a_hi) under "f16x3": "f16" (f16
        MFMA, the six-product form), "fp8" (OCP e4m3 planes on block-scaled FP8 MFMA, gp_head.h X3Q) or "auto"
        (the default: fp8 where the step runs 64-candidate tiles, from 8,193 rows, where it measured faster; f16
        on narrower tiles, where it measured slower). score() evaluates the trunk the PC step runs on that many
        rows, so it follows (its result equals the step's own score bit for bit, and the hybrid's error is
        measured through it); the energy, divergence, gradient and ODE kernels keep the six f16 products."""
        if form not in ("f16", "fp8", "auto"):
            raise ValueError(f"unknown form {form!r} (f16 | fp8 | auto)")
        self.pc_small = form
        self.set_arith(self.arith)

    def _s(self):
        return ctypes.c_void_p(stream_handle(self.device))

    def object_proj(self, feat: torch.Tensor) -> torch.Tensor:
        feat = require_device_tensor(feat, "pts_feat")
        B = feat.shape[0]
        pobj = torch.empty((B, 3 * arch.HEAD_HID), dtype=torch.float32, device=self.device)
        check(self.lib.gp_head_object_proj(ctypes.byref(self.w), ctypes.c_void_p(feat.data_ptr()), B,
                                           ctypes.c_void_p(pobj.data_ptr()), self._s()), "head_object_proj")
        return pobj

    def time_proj(self, t: torch.Tensor) -> torch.Tensor:
        t = require_device_tensor(t.reshape(-1), "t")
        out = torch.empty((t.numel(), 3 * arch.HEAD_HID), dtype=torch.float32, device=self.device)
        check(self.lib.gp_head_time_proj(ctypes.byref(self.w), ctypes.c_void_p(t.data_ptr()), t.numel(),
                                         ctypes.c_void_p(out.data_ptr()), self._s()), "head_time_proj")
        return out

    def score(self, pobj, tproj_row, sigma: float, x: torch.Tensor, k: int, out=None) -> torch.Tensor:
        x = require_device_tensor(x, "x")
        R = x.shape[0]
        out = torch.empty((R, arch.POSE_DIM), dtype=torch.float32, device=self.device) if out is None else out
        check(self.lib.gp_score_eval(ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()),
                                     ctypes.c_void_p(tproj_row.data_ptr()), ctypes.c_float(sigma),
                                     ctypes.c_void_p(x.data_ptr()), R, k, ctypes.c_void_p(out.data_ptr()),
                                     self._s()), "score_eval")
        return out

    def score_div(self, pobj, tproj_row, sigma: float, x: torch.Tensor, eps: torch.Tensor, k: int):
        """gp_score_div_eval: score (R,9) and div (R) = eps . (d score / d x) eps per row (forward mode), fp32."""
        x = require_device_tensor(x, "x")
        eps = require_device_tensor(eps, "eps")
        R = x.shape[0]
        if tuple(eps.shape) != (R, arch.POSE_DIM):
            raise ValueError(f"eps must be ({R}, {arch.POSE_DIM}), got {tuple(eps.shape)}")
        score = torch.empty((R, arch.POSE_DIM), dtype=torch.float32, device=self.device)
        div = torch.empty((R,), dtype=torch.float32, device=self.device)
        check(self.lib.gp_score_div_eval(ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()),
                                         ctypes.c_void_p(tproj_row.data_ptr()), ctypes.c_float(sigma),
                                         ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(eps.data_ptr()), R, k,
                                         ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(div.data_ptr()),
                                         self._s()), "score_div_eval")
        return score, div

    def energy(self, pobj, tproj_row, sigma: float, pose: torch.Tensor, k: int) -> torch.Tensor:
        pose = require_device_tensor(pose, "pose")
        R = pose.shape[0]
        out = torch.empty((R, 2), dtype=torch.float32, device=self.device)
        check(self.lib.gp_energy_eval(ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()),
                                      ctypes.c_void_p(tproj_row.data_ptr()), ctypes.c_float(sigma),
                                      ctypes.c_void_p(pose.data_ptr()), R, k, ctypes.c_void_p(out.data_ptr()),
                                      self._s()), "energy_eval")
        return out

    def energy_score(self, pobj, tproj_row, sigma: float, x: torch.Tensor, k: int, want_energy: bool = False):
        """gp_energy_score_eval: the energy model's score grad_x sum_o x_o f_o / sigma (R,9), by a reverse pass on
        the device (exact fp32 whatever set_arith says); with want_energy also that scalar energy (R,), as
        PoseEnergyNet.forward(return_item='score_and_energy') returns the pair."""
        x = require_device_tensor(x, "x")
        R = x.shape[0]
        score = torch.empty((R, arch.POSE_DIM), dtype=torch.float32, device=self.device)
        energy = torch.empty((R,), dtype=torch.float32, device=self.device) if want_energy else None
        check(self.lib.gp_energy_score_eval(ctypes.byref(self.w), ctypes.byref(self.grad_weights),
                                            ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(tproj_row.data_ptr()),
                                            ctypes.c_float(sigma), ctypes.c_void_p(x.data_ptr()), R, k,
                                            ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(_ptr(energy)),
                                            self._s()), "energy_score_eval")
        return (score, energy) if want_energy else score

    def pc_sample(self, pobj, tproj, step_tab: np.ndarray, x: torch.Tensor, k: int, pts_center: torch.Tensor,
                  z1=None, z2=None, seed: int = 0, snr: float = arch.SNR, want_xs: bool = False, global_batch=None,
                  energy_grad: bool = False, coupling: str = "batch", rows_total=None, row_off: int = 0):
        """gp_pc_sample; with ``global_batch`` (shard.GlobalBatch) gp_pc_sample_global: this rank's rows of one
        call on the whole batch (grad_norm over every shard's rows, one partials all-gather per step).
        ``energy_grad``: gp_pc_sample_energy, the sampler driven by the energy model's score (energy_score).
        ``coupling="object"``: gp_pc_sample_object, the corrector's step size from each object's own k rows, so an
        object's result does not depend on the other objects of the call; the rows are rows [row_off, row_off + R)
        of a batch of ``rows_total`` rows (default R: the call is the whole batch), which picks the tile class
        and keys the device draws."""
        if coupling not in ("batch", "object"):
            raise ValueError(f"coupling {coupling!r} (batch | object)")
        if energy_grad and global_batch is not None:
            raise NotImplementedError("the energy-gradient sampler has no global-batch mode")
        R = x.shape[0]
        T = step_tab.shape[0]
        if coupling == "object":
            if energy_grad:
                raise NotImplementedError("coupling='object' is not built for the energy-gradient sampler")
            if global_batch is not None:
                raise NotImplementedError("coupling='object' needs no global batch: its rows are independent of the "
                                          "other shards' (pass rows_total / row_off instead)")
            return self._pc_sample_object(pobj, tproj, step_tab, x, k, pts_center, z1, z2, seed, snr, want_xs,
                                          R if rows_total is None else int(rows_total), int(row_off))
        if rows_total is not None or row_off:
            raise ValueError("rows_total / row_off belong to coupling='object' (global_batch carries the batch's)")
        need = int(self.lib.gp_pc_workspace_size(R))
        if self._pc_ws is None or self._pc_ws.numel() < need:
            self._pc_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        res = torch.empty((R, 9), dtype=torch.float32, device=self.device)
        q = torch.empty((R, 7), dtype=torch.float32, device=self.device)
        xs = torch.empty((R, T, 9), dtype=torch.float32, device=self.device) if want_xs else None
        tab = np.ascontiguousarray(step_tab, np.float32)
        if global_batch is not None:
            from .shard import PartialsExchange
            gb = global_batch
            if z1 is not None or z2 is not None:
                raise ValueError("global-batch sampling draws its noise on the device (z1 / z2 not supported)")
            rows_total, rows_max = gb.total * k, gb.per_max * k
            if R != (gb.hi - gb.lo) * k:
                raise ValueError(f"global-batch shard: {R} rows for objects [{gb.lo}, {gb.hi}) x {k}")
            n = int(self.lib.gp_pc_global_partials(rows_total, rows_max, gb.world, int(self.w.pe2_h is not None)))
            part = torch.zeros(2 * n, dtype=torch.float32, device=self.device)
            ex = PartialsExchange(part, n, gb)
            rc = self.lib.gp_pc_sample_global(
                ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(tproj.data_ptr()),
                tab.ctypes.data_as(ctypes.c_void_p), T, ctypes.c_void_p(x.data_ptr()), R, k,
                ctypes.c_void_p(pts_center.data_ptr()), ctypes.c_uint64(seed), ctypes.c_float(snr),
                ctypes.c_void_p(res.data_ptr()), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(_ptr(xs)),
                rows_total, gb.lo * k, gb.rank, gb.world, rows_max, ctypes.c_void_p(part.data_ptr()), ex.fn, None,
                ctypes.c_void_p(self._pc_ws.data_ptr()), self._pc_ws.numel(), self._s())
            if ex.error is not None:
                raise RuntimeError("pc_sample_global: partials exchange failed") from ex.error
            check(rc, "pc_sample_global")
            return res, q, xs
        if energy_grad:
            check(self.lib.gp_pc_sample_energy(
                ctypes.byref(self.w), ctypes.byref(self.grad_weights), ctypes.c_void_p(pobj.data_ptr()),
                ctypes.c_void_p(tproj.data_ptr()), tab.ctypes.data_as(ctypes.c_void_p), T,
                ctypes.c_void_p(x.data_ptr()), R, k, ctypes.c_void_p(pts_center.data_ptr()),
                ctypes.c_void_p(_ptr(z1)), ctypes.c_void_p(_ptr(z2)), ctypes.c_uint64(seed), ctypes.c_float(snr),
                ctypes.c_void_p(res.data_ptr()), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(_ptr(xs)),
                ctypes.c_void_p(self._pc_ws.data_ptr()), self._pc_ws.numel(), self._s()), "pc_sample_energy")
            return res, q, xs
        check(self.lib.gp_pc_sample(
            ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(tproj.data_ptr()),
            tab.ctypes.data_as(ctypes.c_void_p), T, ctypes.c_void_p(x.data_ptr()), R, k,
            ctypes.c_void_p(pts_center.data_ptr()), ctypes.c_void_p(_ptr(z1)), ctypes.c_void_p(_ptr(z2)),
            ctypes.c_uint64(seed), ctypes.c_float(snr), ctypes.c_void_p(res.data_ptr()),
            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(_ptr(xs)), ctypes.c_void_p(self._pc_ws.data_ptr()),
            self._pc_ws.numel(), self._s()), "pc_sample")
        return res, q, xs

    def _pc_sample_object(self, pobj, tproj, step_tab, x, k, pts_center, z1, z2, seed, snr, want_xs, rows_total,
                          row_off):
        R = x.shape[0]
        T = step_tab.shape[0]
        need = int(self.lib.gp_pc_object_workspace_size(R))
        if self._pc_ws is None or self._pc_ws.numel() < need:
            self._pc_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        res = torch.empty((R, 9), dtype=torch.float32, device=self.device)
        q = torch.empty((R, 7), dtype=torch.float32, device=self.device)
        xs = torch.empty((R, T, 9), dtype=torch.float32, device=self.device) if want_xs else None
        tab = np.ascontiguousarray(step_tab, np.float32)
        check(self.lib.gp_pc_sample_object(
            ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(tproj.data_ptr()),
            tab.ctypes.data_as(ctypes.c_void_p), T, ctypes.c_void_p(x.data_ptr()), R, k,
            ctypes.c_void_p(pts_center.data_ptr()), ctypes.c_void_p(_ptr(z1)), ctypes.c_void_p(_ptr(z2)),
            ctypes.c_uint64(seed), ctypes.c_float(snr), ctypes.c_void_p(res.data_ptr()),
            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(_ptr(xs)), rows_total, row_off,
            ctypes.c_void_p(self._pc_ws.data_ptr()), self._pc_ws.numel(), self._s()), "pc_sample_object")
        return res, q, xs

    def ode_sample_object(self, pobj, x0: torch.Tensor, k: int, pts_center: torch.Tensor, T0: float, eps: float,
                          steps: Optional[int], rows_total=None, rtol: float = 1e-5, atol: float = 1e-5):
        """cond_ode_sampler with one RK45 solve per object (gp_ode_sample_object): x0 (R,9) fp32, the prior sample
        [+ init_x] at T0 -> pose (R,9), q (R,7) fp64, and per object nfev and status (NumPy int32, R // k). The
        call's rows may be a slice of a batch of ``rows_total`` rows (default R), which picks the tile class."""
        R = x0.shape[0]
        rows_total = R if rows_total is None else int(rows_total)
        x0 = x0.to(self.device, torch.float32).contiguous()
        need = int(self.lib.gp_ode_object_workspace_size_k(R, k)) if k >= 1 and R % k == 0 else 0
        if self._ode_obj_ws is None or self._ode_obj_ws.numel() < need:
            self._ode_obj_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        pose = torch.empty((R, arch.POSE_DIM), dtype=torch.float64, device=self.device)
        q = torch.empty((R, 7), dtype=torch.float64, device=self.device)
        nobj = max(R // max(k, 1), 1)
        nfev = np.zeros(nobj, np.int32)
        status = np.zeros(nobj, np.int32)
        pi = ctypes.POINTER(ctypes.c_int)
        check(self.lib.gp_ode_sample_object(
            ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(x0.data_ptr()), R, k, rows_total,
            float(T0), float(eps), 0 if steps is None else int(steps), float(rtol), float(atol),
            ctypes.c_void_p(require_device_tensor(pts_center, "pts_center").data_ptr()),
            ctypes.c_void_p(pose.data_ptr()), ctypes.c_void_p(q.data_ptr()), nfev.ctypes.data_as(pi),
            status.ctypes.data_as(pi), ctypes.c_void_p(self._ode_obj_ws.data_ptr()), self._ode_obj_ws.numel(),
            self._s()), "ode_sample_object")
        return pose, q, nfev, status

    def like_sample_object(self, pobj, x: torch.Tensor, eps_dir: torch.Tensor, k: int, t0: float, t_bound: float,
                           rows_total=None, rtol: float = 1e-5, atol: float = 1e-5):
        """cond_ode_likelihood with one RK45 solve per object (gp_like_sample_object): x (R,9) fp32, the poses the
        model sees, and eps_dir (R,9) fp32, the Hutchinson direction -> z (R,9) and ll (R) fp64 on the device, and per
        object nfev and status (NumPy int32, R // k). The call's rows may be a slice of a batch of ``rows_total``
        rows (default R), which picks the tile class."""
        R = x.shape[0]
        rows_total = R if rows_total is None else int(rows_total)
        x = require_device_tensor(x.to(self.device, torch.float32).contiguous(), "x")
        eps_dir = require_device_tensor(eps_dir.to(self.device, torch.float32).contiguous(), "eps_dir")
        if tuple(eps_dir.shape) != (R, arch.POSE_DIM):
            raise ValueError(f"epsilon must be ({R}, {arch.POSE_DIM}), got {tuple(eps_dir.shape)}")
        need = int(self.lib.gp_like_object_workspace_size_k(R, k)) if k >= 1 and R % k == 0 else 0
        if self._like_obj_ws is None or self._like_obj_ws.numel() < need:
            self._like_obj_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        z = torch.empty((R, arch.POSE_DIM), dtype=torch.float64, device=self.device)
        ll = torch.empty((R,), dtype=torch.float64, device=self.device)
        nobj = max(R // max(k, 1), 1)
        nfev = np.zeros(nobj, np.int32)
        status = np.zeros(nobj, np.int32)
        pi = ctypes.POINTER(ctypes.c_int)
        check(self.lib.gp_like_sample_object(
            ctypes.byref(self.w), ctypes.c_void_p(pobj.data_ptr()), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(eps_dir.data_ptr()), R, k, rows_total, float(t0), float(t_bound), float(rtol), float(atol),
            ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(ll.data_ptr()), nfev.ctypes.data_as(pi),
            status.ctypes.data_as(pi), ctypes.c_void_p(self._like_obj_ws.data_ptr()), self._like_obj_ws.numel(),
            self._s()), "like_sample_object")
        return z, ll, nfev, status

    def ode_sample_energy(self, pobj, x0: torch.Tensor, k: int, pts_center: torch.Tensor, T0: float, eps: float,
                          steps: Optional[int], rtol: float = 1e-5, atol: float = 1e-5):
        """cond_ode_sampler driven by the energy model's score, the whole sampler in the one C call
        (gp_ode_sample_energy, the entry of hosts without Python): x0 (R,9) fp32, the prior sample [+ init_x] at T0
        -> pose (R,9), q (R,7) fp64, nfev, status (1 done, -1 step size below the spacing of t)."""
        R = x0.shape[0]
        x0 = x0.to(self.device, torch.float32).contiguous()
        ws = torch.empty(int(self.lib.gp_ode_sample_workspace_size(R)), dtype=torch.uint8, device=self.device)
        pose = torch.empty((R, arch.POSE_DIM), dtype=torch.float64, device=self.device)
        q = torch.empty((R, 7), dtype=torch.float64, device=self.device)
        nfev, status = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib.gp_ode_sample_energy(
            ctypes.byref(self.w), ctypes.byref(self.grad_weights), ctypes.c_void_p(pobj.data_ptr()),
            ctypes.c_void_p(x0.data_ptr()), R, k, float(T0), float(eps), 0 if steps is None else int(steps),
            float(rtol), float(atol), ctypes.c_void_p(require_device_tensor(pts_center, "pts_center").data_ptr()),
            ctypes.c_void_p(pose.data_ptr()), ctypes.c_void_p(q.data_ptr()), ctypes.byref(nfev), ctypes.byref(status),
            ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._s()), "ode_sample_energy")
        return pose, q, int(nfev.value), int(status.value)

    def ode_denoise(self, pobj, t32: float, sigma: float, g2: float, step: float, x: torch.Tensor, k: int,
                    pts_center: torch.Tensor, ws: torch.Tensor, energy_grad: bool = False):
        """cond_ode_sampler's final denoise + epilogue (gp_ode_denoise) -> pose (R,9), q (R,7) fp64.
        ``energy_grad``: gp_ode_denoise_energy, the step's score is the energy model's gradient."""
        R = x.numel() // arch.POSE_DIM
        pose = torch.empty((R, arch.POSE_DIM), dtype=torch.float64, device=self.device)
        q = torch.empty((R, 7), dtype=torch.float64, device=self.device)
        if energy_grad:
            fn, head = self.lib.gp_ode_denoise_energy, (ctypes.byref(self.w), ctypes.byref(self.grad_weights))
        else:
            fn, head = self.lib.gp_ode_denoise, (ctypes.byref(self.w),)
        check(fn(
            *head, ctypes.c_void_p(pobj.data_ptr()), t32, sigma, g2, step,
            ctypes.c_void_p(x.data_ptr()), R, k, ctypes.c_void_p(require_device_tensor(pts_center, "pts_center").data_ptr()),
            ctypes.c_void_p(pose.data_ptr()), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
            ws.numel(), self._s()), "ode_denoise")
        return pose, q


class ScaleModel:
    def __init__(self, sd: weights.StateDict, device: torch.device):
        self.lib = _lib.load()
        self.device = device
        self.up = _Uploaded(pack.pack_scale(sd), device)
        self.w = _lib.ScaleWeights(**{k: self.up.ptr(k) for k in pack.SCALE_FIELDS})

    def forward(self, axes: torch.Tensor, pts_feat: torch.Tensor) -> torch.Tensor:
        axes = require_device_tensor(axes, "axes")
        pts_feat = require_device_tensor(pts_feat, "pts_feat")
        B = axes.shape[0]
        out = torch.empty((B, 3), dtype=torch.float32, device=self.device)
        check(self.lib.gp_scale_forward(ctypes.byref(self.w), ctypes.c_void_p(axes.data_ptr()),
                                        ctypes.c_void_p(pts_feat.data_ptr()), B, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(stream_handle(self.device))), "scale_forward")
        return out


def pose_epilogue_f64(pose: torch.Tensor, k: int, pts_center: torch.Tensor):
    lib = _lib.load()
    pose = pose.contiguous()
    q = torch.empty((pose.shape[0], 7), dtype=torch.float64, device=pose.device)
    check(lib.gp_pose_epilogue_f64(ctypes.c_void_p(pose.data_ptr()), pose.shape[0], k,
                                   ctypes.c_void_p(require_device_tensor(pts_center, "pts_center").data_ptr()),
                                   ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(stream_handle(pose.device))),
          "pose_epilogue_f64")
    return pose, q


def points_mean(pts: torch.Tensor) -> torch.Tensor:
    """gp_points_mean: (B,N,C>=3) -> (B,3) mean of the first three channels over the points."""
    pts = require_device_tensor(pts, "pts")
    B, N, C = pts.shape
    out = torch.empty((B, 3), dtype=torch.float32, device=pts.device)
    check(_lib.load().gp_points_mean(ctypes.c_void_p(pts.data_ptr()), B, N, C, ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(stream_handle(pts.device))), "points_mean")
    return out


def bbox_length(pcl: torch.Tensor, pose: torch.Tensor) -> torch.Tensor:
    """gp_bbox_length: raw points (B,N,C>=3) and aggregated poses (B,4,4) -> (B,3) box lengths."""
    pcl = require_device_tensor(pcl, "pcl")
    pose = require_device_tensor(pose, "pose")
    B, N, C = pcl.shape
    if pose.shape != (B, 4, 4):
        raise ValueError(f"pose must be ({B},4,4), got {tuple(pose.shape)}")
    out = torch.empty((B, 3), dtype=torch.float32, device=pcl.device)
    check(_lib.load().gp_bbox_length(ctypes.c_void_p(pcl.data_ptr()), B, N, C, ctypes.c_void_p(pose.data_ptr()),
                                     ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream_handle(pcl.device))),
          "bbox_length")
    return out


def randn(seed: int, stream: int, rows: int, cols: int, device) -> torch.Tensor:
    """gp_randn: the device draws gp_pc_sample uses (streams 2j / 2j+1 for step j, cols = 9)."""
    lib = _lib.load()
    out = torch.empty((rows, cols), dtype=torch.float32, device=device)
    check(lib.gp_randn(ctypes.c_uint64(seed), ctypes.c_uint32(stream), rows, cols, ctypes.c_void_p(out.data_ptr()),
                       ctypes.c_void_p(stream_handle(out.device))), "randn")
    return out
