"""ctypes binding of libgill_amd.so (C ABI declared in include/gill_amd.h).

The library is the product: there is no Python/torch fallback for any op it exports.  Importing this
module without a built library raises; calling into it without a GPU fails in the HIP runtime.
torch is used only as the owner of device memory and streams (tensor.data_ptr(), current stream).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GILL_AMD_LIB") or os.path.join(_HERE, "libgill_amd.so")   # GILL_AMD_LIB: A/B runs of two builds


class GillNativeError(RuntimeError):
  pass


class gill_tensor(C.Structure):
  _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int32), ("ndim", C.c_int32),
              ("shape", C.c_int64 * 4)]


class gill_opt_config(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ("vocab_size", "hidden_size", "num_layers", "num_heads", "ffn_dim",
                                       "max_positions", "max_batch", "max_seq")]


class gill_mapper_config(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ("in_dim", "out_dim", "hidden_dim", "num_heads", "ffn_dim", "num_enc_layers",
                                       "num_dec_layers", "num_input_tokens", "num_output_tokens", "max_batch")]


class gill_unet_config(C.Structure):
  _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
              ("layers_per_block", C.c_int32), ("cross_attention_dim", C.c_int32), ("num_heads", C.c_int32),
              ("norm_num_groups", C.c_int32), ("sample_size", C.c_int32), ("ctx_len", C.c_int32),
              ("max_batch", C.c_int32), ("heads_per_level", C.c_int32 * 4), ("v_prediction", C.c_int32),
              ("fp8_convs", C.c_int32)]


class gill_decode_rule(C.Structure):
  _fields_ = [("n_ret", C.c_int32), ("ret_ids", C.c_int32 * 16), ("n_gen", C.c_int32), ("gen_ids", C.c_int32 * 16),
              ("step", C.c_int32), ("min_word_tokens", C.c_int32), ("ret_eq_gen", C.c_int32),
              ("ret_scale", C.c_double), ("gen_scale", C.c_double), ("filter_value", C.c_double)]


class gill_decode_sampler(C.Structure):
  _fields_ = [("seed", C.c_uint64), ("draw", C.c_int32), ("row0", C.c_int32), ("temperature", C.c_double), ("top_p", C.c_double)]


class gill_clip_config(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ("image_size", "patch_size", "hidden_size", "num_layers", "num_heads", "intermediate_size",
                                       "max_batch")]


class gill_clip_text_config(C.Structure):
  _fields_ = [(n, C.c_int32) for n in ("vocab_size", "hidden_size", "num_layers", "num_heads", "intermediate_size", "max_positions",
                                       "hidden_act", "max_batch")]


class gill_vae_config(C.Structure):
  _fields_ = [("latent_channels", C.c_int32), ("out_channels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
              ("layers_per_block", C.c_int32), ("norm_num_groups", C.c_int32), ("latent_size", C.c_int32),
              ("scaling_factor", C.c_float), ("max_batch", C.c_int32)]


class gill_sd_sampler(C.Structure):
  _fields_ = [("kind", C.c_int32), ("steps_offset", C.c_int32), ("set_alpha_to_one", C.c_int32), ("eta", C.c_float)]


SD_ROW_DOUBLES = 12     # GILL_SD_ROW_DOUBLES: [mode, slot_new, s1, s2, s3, in_scale, p_x, p_e, c_x, c_0, c_1, c_n]


# every symbol include/gill_amd.h declares: (restype, argtypes)
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
SYMBOLS: Dict[str, Tuple[object, List[object]]] = {
  "gill_last_error": (C.c_char_p, []),
  "gill_version": (_i, []),
  "gill_opt_create": (_i, [C.POINTER(_vp), C.POINTER(gill_opt_config), C.POINTER(gill_tensor), _i]),
  "gill_opt_destroy": (None, [_vp]),
  "gill_opt_create_ex": (_i, [C.POINTER(_vp), C.POINTER(gill_opt_config), C.POINTER(gill_tensor), _i, _i]),
  "gill_opt_weight_mode": (_i, [_vp]),
  "gill_opt_decode_uses_w8": (_i, [_vp, _i]),
  "gill_opt_cached_uses_w8": (_i, [_vp, _i, _i, _i]),
  "gill_w8_max_rows": (_i, []),
  "gill_op_w8_quant": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
  "gill_op_w8_dequant": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
  "gill_op_linear_w8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
  "gill_opt_embed": (_i, [_vp, _vp, _i, _vp, _vp]),
  "gill_opt_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
  "gill_opt_forward_cached": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
  "gill_opt_img_hidden": (_i, [_vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _vp]),
  "gill_opt_img_hidden_ex": (_i, [_vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
  "gill_opt_last_logits": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
  "gill_opt_next_token": (_i, [_vp, _vp, _i, _i, C.POINTER(gill_decode_rule), _vp, _vp, _i, _i, _vp, _vp, _vp]),
  "gill_opt_pick_token": (_i, [_vp, _vp, _i, C.POINTER(gill_decode_rule), _vp, _i, _i, _vp, _vp, _vp]),
  "gill_opt_decode_logits": (_i, [_vp, _vp, _i, _i, C.POINTER(gill_decode_rule), _vp, _vp]),
  "gill_opt_filter_logits": (_i, [_vp, _vp, _vp, _i, C.c_double, C.c_double, C.c_double, _i, _vp]),
  "gill_opt_sample_token": (_i, [_vp, _vp, _i, _i, C.POINTER(gill_decode_rule), C.POINTER(gill_decode_sampler), _vp, _vp, _i, _i, _vp,
                                 _vp, _vp]),
  "gill_opt_draw_token": (_i, [_vp, _vp, _i, C.POINTER(gill_decode_rule), C.POINTER(gill_decode_sampler), _vp, _i, _i, _vp, _vp, _vp]),
  "gill_decode_uniforms": (_i, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
  "gill_attention_decode": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
  "gill_attention_append": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
  "gill_attention_extend": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
  "gill_opt_extend": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
  "gill_attention_fork_ws_bytes": (C.c_int64, [_i, _i, _i, _i]),
  "gill_attention_fork": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_int64, _vp]),
  "gill_attention_branch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
  "gill_kv_branch_adopt": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_opt_branch_reserve": (_i, [_vp, _i, _i]),
  "gill_opt_branch_bytes": (C.c_int64, [_vp]),
  "gill_opt_decode_step_branch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
  "gill_opt_next_token_branch": (_i, [_vp, _vp, _i, C.POINTER(gill_decode_rule), _i, C.POINTER(gill_decode_sampler), _vp, _vp, _vp, _i, _vp,
                                      _vp]),
  "gill_opt_branch_adopt": (_i, [_vp, _i, _i, _i, _i, _vp]),
  "gill_opt_score_candidates": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
  "gill_opt_set_kv_format": (_i, [_vp, _i]),
  "gill_opt_kv_format": (_i, [_vp]),
  "gill_opt_kv_bytes": (C.c_int64, [_vp]),
  "gill_attention_decode_kv8": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
  "gill_attention_extend_kv8": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
  "gill_opt_decode_step": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
  "gill_opt_prefill_ids": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
  "gill_opt_next_token_ragged": (_i, [_vp, _vp, _i, C.POINTER(gill_decode_rule), _i, C.POINTER(gill_decode_sampler), _vp, _vp, _vp, _i, _vp,
                                      _vp]),
  "gill_opt_pick_token_ragged": (_i, [_vp, _vp, _i, C.POINTER(gill_decode_rule), _i, C.POINTER(gill_decode_sampler), _vp, _vp, _i, _vp, _vp]),
  "gill_clip_create": (_i, [C.POINTER(_vp), C.POINTER(gill_clip_config), C.POINTER(gill_tensor), _i]),
  "gill_clip_destroy": (None, [_vp]),
  "gill_clip_forward": (_i, [_vp, _vp, _i, _vp, _vp]),
  "gill_clip_preprocess_workspace": (_i, [C.POINTER(C.c_int64), _i, _i, C.POINTER(C.c_int64)]),
  "gill_clip_preprocess": (_i, [_vp, C.c_int64, C.POINTER(C.c_int64), _i, _i, _i, _vp, _vp, _vp, C.c_int64, _vp]),
  "gill_clip_resize_ksize": (_i, [_i, _i]),
  "gill_clip_resize_taps": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i]),
  "gill_clip_text_create": (_i, [C.POINTER(_vp), C.POINTER(gill_clip_text_config), C.POINTER(gill_tensor), _i]),
  "gill_clip_text_destroy": (None, [_vp]),
  "gill_clip_text_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
  "gill_mapper_create": (_i, [C.POINTER(_vp), C.POINTER(gill_mapper_config), C.POINTER(gill_tensor), _i]),
  "gill_mapper_destroy": (None, [_vp]),
  "gill_mapper_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
  "gill_unet_create": (_i, [C.POINTER(_vp), C.POINTER(gill_unet_config), C.POINTER(gill_tensor), _i]),
  "gill_unet_destroy": (None, [_vp]),
  "gill_unet_forward": (_i, [_vp, _vp, C.POINTER(C.c_float), _vp, _i, _vp, _vp]),
  "gill_sd_denoise": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _f, _vp, _vp]),
  "gill_vae_create": (_i, [C.POINTER(_vp), C.POINTER(gill_vae_config), C.POINTER(gill_tensor), _i]),
  "gill_vae_destroy": (None, [_vp]),
  "gill_vae_decode": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
  "gill_vae_encode": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
  "gill_sd_schedule_from": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double)]),
  "gill_sd_denoise_from": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
  "gill_op_sd_sampler_run_from": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i, C.c_int64, _vp, _vp, _vp]),
  "gill_sd_inpaint_prepare": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
  "gill_sd_inpaint_keep": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_double)]),
  "gill_sd_inpaint": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
  "gill_op_sd_inpaint_run": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _vp, _vp, _vp]),
  "gill_op_conv3x3_ex": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_conv3x3_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_ret_index_create": (_i, [C.POINTER(_vp), _i, C.c_int64]),
  "gill_ret_index_destroy": (None, [_vp]),
  "gill_ret_index_add": (_i, [_vp, _vp, _i, C.c_int64, _i, _f, _vp]),
  "gill_ret_index_size": (C.c_int64, [_vp]),
  "gill_ret_index_rows": (_i, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
  "gill_ret_index_search": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp]),
  "gill_ret_index_slabs": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
  "gill_pndm_schedule": (_i, [_i, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
  "gill_sd_denoise_ex": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _f, _vp, _vp, _vp]),
  "gill_sd_schedule": (_i, [_vp, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
  "gill_op_sd_sampler_run": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp, _i, C.c_int64, _vp, _vp, _vp]),
  "gill_coop_timeouts": (_i, []),
  "gill_op_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _i, _vp]),
  "gill_op_geglu": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
  "gill_op_conv3x3": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp]),
  "gill_op_layernorm": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp]),
  "gill_op_groupnorm": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp]),
  "gill_op_conv3x3_gn_stats": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
  "gill_op_gemm_gn_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
  "gill_op_groupnorm_from_stats": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _f, _vp]),
  "gill_op_conv3x3_gn": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_conv3x3_shortcut": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
  "gill_op_ffn_fused": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
  "gill_op_ffn_fused_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
  "gill_op_geglu_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
  "gill_conv_fp8_kpad": (_i, [_i]),
  "gill_op_quant_fp8": (_i, [_vp, _f, C.c_int64, _vp, _vp]),
  "gill_op_conv_weight_quant_fp8": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp]),
  "gill_op_conv3x3_fp8_q": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_groupnorm_fp8": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _f, _vp, _vp]),
  "gill_op_linear_weight_quant_fp8": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp]),
  "gill_op_ln_quant_fp8": (_i, [_vp, _i, _i, _vp, _i, _i, _f, _f, _vp, _vp]),
  "gill_op_geglu_fp8_q": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
  "gill_op_lnproj": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
  "gill_op_lnproj_ex": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
  "gill_op_cross_attention_folded": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_linear_rowstats": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int), _i, _i, _i, _i, _vp]),
  "gill_op_ln_gemm": (_i, [_i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_op_vae_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(C.c_int), _vp]),
  "gill_op_row_softmax": (_i, [_vp, _i, _i, _vp]),
  "gill_op_conv_out": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int), _vp]),
  "gill_op_conv_in": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
  "gill_op_conv_in_wide": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
  "gill_op_timestep_embed": (_i, [_vp, _i, _i, _vp, _vp]),
  "gill_op_reduce_ln": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
  "gill_op_linear_reduce_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
  "gill_op_skinny_gemm": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
  "gill_op_lm_head_loss": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
  "gill_lm_loss_geometry": (_i, [_i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
  "gill_op_img_block_heads": (_i, [_vp, C.c_int64, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
  "gill_op_img_rerank_scores": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
  "gill_gemm_plan": (_i, [_vp, _i, _i, _i, _i, _vp]),
  "gill_gemm_plan_log": (_i, [_vp, _i, C.POINTER(C.c_int)]),
  "gill_unet_xf_plan": (_i, [_vp, _i, _i, _i, _i, _vp]),
  "gill_gemm_query": (_i, [_vp, _i, _i, _i, _i, _vp]),
  "gill_attention_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp]),
  "gill_opt_forward_loss": (_i, [_vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
  """Load libgill_amd.so (once).  Raises GillNativeError when it has not been built."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise GillNativeError(
        f"{LIB_PATH} is missing: the HIP extension is the only implementation of the GILL hot path. "
        "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C gill_amd/csrc`).")
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
      fn = getattr(l, name)  # AttributeError here == header/library mismatch
      fn.restype = res
      fn.argtypes = args
    _lib = l
  return _lib


def check(rc: int) -> None:
  if rc != 0:
    msg = lib().gill_last_error()
    raise GillNativeError(f"libgill_amd error {rc}: {msg.decode() if msg else '?'}")


def current_stream() -> int:
  return int(torch.cuda.current_stream().cuda_stream)


_DTYPES = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
  if t is None:
    return None
  assert t.is_cuda and t.is_contiguous(), "libgill_amd takes contiguous device tensors"
  return t.data_ptr()


def make_tensor_table(state: Dict[str, torch.Tensor], device: torch.device):
  """state-dict -> (gill_tensor array, keep-alive list).  Tensors are moved to `device` if needed."""
  keep = []
  arr = (gill_tensor * len(state))()
  for i, (k, v) in enumerate(state.items()):
    if v.dtype not in _DTYPES:
      v = v.float()
    v = v.detach().to(device).contiguous()
    name = k.encode()
    keep.append((name, v))
    arr[i].name = name
    arr[i].data = v.data_ptr()
    arr[i].dtype = _DTYPES[v.dtype]
    arr[i].ndim = v.dim()
    for d in range(4):
      arr[i].shape[d] = v.shape[d] if d < v.dim() else 1
  return arr, keep
