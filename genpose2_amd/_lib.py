"""ctypes binding of libgenpose_hip.so (include/genpose_hip.h).

The library is built in-tree (``genpose2_amd/libgenpose_hip.so``, see ``__graft_entry__.build``).
There is no fallback: if the library is missing or a call fails, a ``GenPoseHipError`` is raised.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterable

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GENPOSE_HIP_LIB", os.path.join(_HERE, "libgenpose_hip.so"))

c_int, c_float, c_size_t, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
c_double = ctypes.c_double
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_uint64 = ctypes.c_uint64


class GenPoseHipError(RuntimeError):
    pass


class HeadWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("pe0_w", "pe0_b", "pe2_w", "pe2_b", "h1p_w", "h2_w", "h2_b",
                                       "h1pts_t", "h1_b", "gfp_w", "te_w_t", "te_b", "h1t_t", "pe2_h", "h1p_h",
                                       "hsc", "pe2_q", "h1p_q")] + [("q8_flags", c_size_t)]


class HeadGradWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("pe0_wt", "pe2_wt", "h1p_wt")]


class ScaleWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ae0_w", "ae0_b", "ae2_w", "ae2_b", "ft0_w", "ft0_b", "ft2_w",
                                       "ft2_b")]


class DinoBlock(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_w", "ln2_b",
                                       "w12_w", "w12_b", "w3_w", "w3_b", "qkv_h", "proj_h", "w12_h", "w3_h")]


class DinoWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("patch_w", "patch_b", "cls_token", "storage_tokens", "norm_w", "norm_b",
                                       "rope")] + [("rope_hp", c_int), ("rope_wp", c_int), ("blocks", DinoBlock * 12)]


# name -> (restype, argtypes)
_SIGS: Dict[str, tuple] = {
    "gp_last_error": (ctypes.c_char_p, []),
    "gp_abi_version": (c_int, []),
    "gp_furthest_point_sampling": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_gather_points": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_ball_query": (c_int, [c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_group_points": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_encoder_workspace_size": (c_size_t, [c_int, c_int]),
    "gp_encoder_workspace_layout": (c_int, [c_int, c_int, c_int64_p]),
    "gp_encoder_forward": (c_int, [c_void_p, c_int64_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p,
                                   c_void_p]),
    "gp_encoder_fps": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gp_encoder_geometry": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gp_encoder_forward_geom": (c_int, [c_void_p, c_int64_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                        c_void_p, c_void_p]),
    "gp_encoder_geometry_levels": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "gp_encoder_forward_geom_levels": (c_int, [c_void_p, c_int64_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                               c_size_t, c_void_p, c_int, c_int, c_void_p]),
    "gp_sa_level": (c_int, [c_void_p, c_int64_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                            c_void_p, c_void_p]),
    "gp_sa_level_geom": (c_int, [c_void_p, c_int64_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p, c_void_p]),
    "gp_linear": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "gp_linear_split_words": (c_size_t, [c_int, c_int]),
    "gp_linear_split": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int,
                                c_void_p, c_int, c_void_p, c_void_p]),
    "gp_add_layernorm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                 c_void_p]),
    "gp_relpe_bias_bytes": (c_size_t, [c_int, c_int]),
    "gp_relpe_bias": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gp_mha_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_mha_relpe_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p]),
    "gp_interp_points": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_fusion_attend_workspace_size": (c_size_t, [c_int, c_int, c_int]),
    "gp_fusion_attend": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_fusion_mix": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gp_weights_pack": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_void_p)]),
    "gp_weights_free": (None, [c_void_p]),
    "gp_weights_heads": (ctypes.POINTER(HeadWeights), [c_void_p]),
    "gp_weights_scale": (ctypes.POINTER(ScaleWeights), [c_void_p]),
    "gp_weights_encoder": (c_void_p, [c_void_p, ctypes.POINTER(c_int64_p)]),
    "gp_weights_pack_host": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     ctypes.POINTER(c_size_t), c_int64_p, c_int64_p]),
    "gp_head_object_proj": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_int, c_void_p, c_void_p]),
    "gp_head_time_proj": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_int, c_void_p, c_void_p]),
    "gp_score_eval": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_float, c_void_p, c_int, c_int,
                              c_void_p, c_void_p]),
    "gp_energy_eval": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_float, c_void_p, c_int, c_int,
                               c_void_p, c_void_p]),
    "gp_head_grad_floats": (c_size_t, []),
    "gp_head_grad_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_energy_score_eval": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_void_p,
                                     c_float, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_pc_sample_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_void_p,
                                    c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_uint64,
                                    c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_debug_q8_probe": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_debug_pose_tail_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_debug_ode_obj_rec_size": (c_size_t, []),
    "gp_debug_ode_obj_control": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_int, c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "gp_pc_workspace_size": (c_size_t, [c_int]),
    "gp_pc_tile_rows": (c_int, [c_int, c_int]),
    "gp_pc_sample": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, c_uint64, c_float, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_size_t, c_void_p]),
    "gp_pc_object_workspace_size": (c_size_t, [c_int]),
    "gp_pc_sample_object": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                    c_int, c_void_p, c_void_p, c_void_p, c_uint64, c_float, c_void_p, c_void_p,
                                    c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gp_pc_global_partials": (c_int, [c_int, c_int, c_int, c_int]),
    "gp_pc_sample_global": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                    c_int, c_void_p, c_uint64, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_pose_epilogue_f64": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_ode_workspace_size": (c_size_t, [c_int]),
    "gp_ode_rhs": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_float, c_float, c_double, c_void_p, c_void_p,
                           c_void_p, c_int, c_double, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_ode_attempt": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_int, c_int,
                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_score_div_eval": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int,
                                  c_int, c_void_p, c_void_p, c_void_p]),
    "gp_like_workspace_size": (c_size_t, [c_int]),
    "gp_like_rhs": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_float, c_float, c_double, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_int, c_double, c_int, c_int, c_void_p, c_void_p, c_size_t,
                            c_void_p]),
    "gp_like_attempt": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double,
                                c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_ode_init_norms": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_double, c_double, c_void_p,
                                  c_void_p]),
    "gp_ode_dense": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_double,
                             ctypes.c_longlong, c_void_p, c_void_p]),
    "gp_ode_denoise": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_float, c_float, c_float, c_float, c_void_p,
                               c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the energy agent's ODE entries: their namesakes' arguments with the transposed weights behind w
    "gp_ode_rhs_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_float,
                                  c_float, c_double, c_void_p, c_void_p, c_void_p, c_int, c_double, c_int, c_int,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_ode_attempt_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                      c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "gp_ode_auto_attempt_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p,
                                           c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_double,
                                           c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gp_ode_denoise_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_float,
                                      c_float, c_float, c_float, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    "gp_ode_sample_energy": (c_int, [ctypes.POINTER(HeadWeights), ctypes.POINTER(HeadGradWeights), c_void_p, c_void_p,
                                     c_int, c_int, c_double, c_double, c_int, c_double, c_double, c_void_p, c_void_p,
                                     c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_size_t,
                                     c_void_p]),
    "gp_ode_ctl_size": (c_size_t, []),
    "gp_ode_auto_workspace_size": (c_size_t, [c_int]),
    "gp_ode_auto_attempt": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_int, c_int, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "gp_ode_auto_attempt_hs": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_int, c_int, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "gp_ode_global_partials": (c_int, [c_int, c_int, c_int, c_int]),
    "gp_ode_global_workspace_size": (c_size_t, [c_int]),
    "gp_ode_auto_partials_offset": (c_size_t, []),
    "gp_ode_auto_attempt_global": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_int, c_int, c_double, c_double,
                                           c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                           c_void_p]),
    "gp_pc_step_table": (c_int, [c_int, c_float, c_void_p]),
    "gp_ode_sample_workspace_size": (c_size_t, [c_int]),
    "gp_ode_sample": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_int, c_int, c_double, c_double,
                              c_int, c_double, c_double, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "gp_ode_object_workspace_size": (c_size_t, [c_int]),
    "gp_ode_object_workspace_size_k": (c_size_t, [c_int, c_int]),
    "gp_ode_sample_object": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                     c_double, c_int, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                     ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "gp_like_object_workspace_size": (c_size_t, [c_int]),
    "gp_like_object_workspace_size_k": (c_size_t, [c_int, c_int]),
    "gp_like_sample_object": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                      ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "gp_debug_like_obj_attempt": (c_int, [ctypes.POINTER(HeadWeights), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double,
                                          c_void_p]),
    "gp_img_encoder_workspace_size": (c_size_t, [c_int, c_int, c_int]),
    "gp_img_encoder": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                               c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_size_t, c_void_p]),
    "gp_img_encoder2": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                                c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_img_encoder3": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                                c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_img_encoder3_workspace_size": (c_size_t, [c_int, c_int, c_int, c_int]),
    "gp_img_geo_table": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "gp_gather_patch_points": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p]),
    "gp_dino_workspace_size": (c_size_t, [c_int, c_int, c_int]),
    "gp_dino_rope_table": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gp_dino_forward": (c_int, [ctypes.POINTER(DinoWeights), c_void_p, c_int, c_int, c_int, c_int,
                                ctypes.POINTER(c_int), ctypes.POINTER(c_void_p), c_int, c_void_p, c_size_t,
                                c_void_p]),
    "gp_scale_forward": (c_int, [ctypes.POINTER(ScaleWeights), c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gp_randn": (c_int, [c_uint64, ctypes.c_uint32, c_int, c_int, c_void_p, c_void_p]),
    "gp_points_mean": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gp_bbox_length": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_rank_aggregate": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "gp_rank_aggregate_modes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_frame_mask_stats": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gp_frame_crop_boxes": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "gp_frame_objects_workspace_size": (c_size_t, [c_int, c_int]),
    "gp_frame_objects": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                 c_float, c_float, c_float, c_float, c_uint64, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "gp_frame_roi_rgb": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gp_frames_mask_stats": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gp_frames_objects": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "gp_frames_roi_rgb": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p]),
}

EXPORTED = tuple(_SIGS)
_lib = None


# gp_pc_exchange_fn (genpose_hip.h): int (*)(void* ctx, int step, float* slot, int n, hipStream_t stream)
PC_EXCHANGE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, c_void_p, c_int, c_void_p)
ODE_EXCHANGE_FN = PC_EXCHANGE_FN   # gp_ode_exchange_fn: the same C signature with an fp64 partials pointer


def load(path: str = LIB_PATH):
    """Load the HIP library (raises GenPoseHipError if it is absent or incomplete)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise GenPoseHipError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; "
                              f"g.build()'` (there is no CPU fallback)")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().gp_last_error().decode(errors="replace")
        raise GenPoseHipError(f"{what or 'genpose_hip'} failed ({rc}): {msg}")


def vp(t) -> ctypes.c_void_p:
    """A device tensor's address as a C pointer argument (None: a null pointer)."""
    return c_void_p(None if t is None else t.data_ptr())


def exported_symbols(path: str = LIB_PATH) -> Iterable[str]:
    lib = ctypes.CDLL(path)
    return [n for n in _SIGS if hasattr(lib, n)]
