"""ctypes binding of libdq_hip.so (include/dq_hip.h).  There is NO fallback: if the library is missing or a call
fails, a RuntimeError is raised -- the product path never routes through PyTorch ops or the test oracle."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DQ_HIP_LIB", os.path.join(os.path.dirname(_HERE), "libdq_hip.so"))

_lib = None
ABI_VERSION = 13  # DQ_ABI_VERSION of include/dq_hip.h this table was written against
PRED_TYPES = {"eps": 0, "x0": 1, "v_prediction": 2}  # DQ_PRED_EPS / DQ_PRED_X0 / DQ_PRED_V
SAMPLERS = {"reference": 0, "ddim": 1, "dpmpp_2m": 2}  # DQ_SAMPLER_*
UPDATE_KINDS = {"ddim": 0, "stochastic": 1, "solver_1": 2, "solver_2m": 3}  # DQ_UPDATE_* (dq_guided_update)
CONSISTENCY_MODES = {"bound": 1, "sum": 2}  # DQ_CONSIST_BOUND / DQ_CONSIST_SUM (dq_group_project, dq_sample_call.consistency)
GROUP_MAX = 8  # DQ_GROUP_MAX
PRECISIONS = {"fp32": 0, "bf16x3": 1}  # DQ_PRECISION_FP32 / DQ_PRECISION_BF16X3
FINAL_ACTS = {"identity": 0, "softplus": 1}  # DQ_FINAL_IDENTITY / DQ_FINAL_SOFTPLUS
RES_FWD_FORMS = ("rt", "level", "v4", "unfused")  # DQ_RES_FWD_* (index = value)
RES_BWD_FORMS = ("wg", "rt", "rows", "cp", "plain", "unfused")  # DQ_RES_BWD_*
LA_FWD_FORMS = ("long", "small", "rows", "register")  # DQ_LA_FWD_*
LA_BWD_FORMS = ("long", "rows", "register")  # DQ_LA_BWD_*
TFM_ATTN_FORMS = ("gemm", "fused")  # DQ_TFM_ATTN_* (index = value)
CONV_BWD_DATA_FORMS = ("wg", "gemm", "plain")  # DQ_CONV_BWD_DATA_*
CONV_WGRAD_FORMS = ("wg", "v4", "scalar")  # DQ_CONV_WGRAD_*
LEVEL_KINDS = ("unfused", "kernel", "tiny")  # DQ_LEVEL_* (index = value)
LEVEL_FORM_FIELDS = ("kind", "img", "la", "post_w", "in_folded", "resample")  # DQ_LEVEL_PLAN_FORM_INTS, in the order dq_debug_level_plan writes them
GROUP_METRIC_NAMES = ("excess", "unexplained", "mix_total")  # DQ_GROUP_* (index = column of dq_group_metrics' `group` output)
METRIC_NAMES = ("mse", "mae", "cosine", "sa", "pearson", "scan_sa", "scan_count", "xic_r", "xic_count")  # DQ_METRIC_* (index = column of dq_recon_metrics' output)
GEMM_PLAN_PART_FIELDS = ("tile_base", "ntiles", "splits", "k_per_split")  # of `full`, then of `rest`, after bm and kv (DQ_GEMM_PLAN_INTS)
MID_FORMS_FIELDS = ("qkv_fused", "out_fused", "pre_fused", "wide_mid", "mid_c", "cond_dim", "prep_ok", "ss_mid1", "ss_mid2", "ss_total")  # DQ_MID_FORMS_INTS, in dq_debug_mid_forms' order
TBUF_FLOATS = 100  # DQ_TBUF_FLOATS: a sample's scratch of the time-embedding kernels (dq_debug_time_fwd / _bwd)
TBUF_SLOTS = {"sinu": 0, "h_pre": 4, "h_act": 20, "temb": 36, "silu": 52, "dtemb": 68, "dh_pre": 84}  # DQ_TBUF_* (tests/test_time_embed.py reads the header)
LEVEL_PLAN_FLAGS = ("prep_ok", "init_fused", "head_shape", "head_train", "use_tb_up", "use_tb_dn", "tb_up_w")  # DQ_LEVEL_PLAN_FLAG_INTS

# name -> (restype, argtypes); this table is checked against include/dq_hip.h by tests/test_abi.py
PROTOTYPES = {
    "dq_last_error": (c_char_p, []),
    "dq_abi_version": (c_int, []),
    "dq_plan_create": (c_void_p, [c_int, c_int, POINTER(c_int), c_int, c_int]),
    "dq_plan_create_ex": (c_void_p, [c_int, c_int, POINTER(c_int), c_int, c_int, c_int]),
    "dq_plan_attn_cond_channels": (c_int, [c_void_p]),
    "dq_plan_destroy": (None, [c_void_p]),
    "dq_plan_num_params": (c_int, [c_void_p]),
    "dq_plan_param_floats": (c_int64, [c_void_p]),
    "dq_plan_param_info": (c_int, [c_void_p, c_int, c_char_p, c_int, POINTER(c_int64), POINTER(c_int), POINTER(c_int64)]),
    "dq_unet_workspace_bytes": (c_int64, [c_void_p, c_int, c_int, c_int]),
    "dq_plan_set_final_act": (c_int, [c_void_p, c_int]),
    "dq_plan_final_act": (c_int, [c_void_p]),
    "dq_q_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "dq_ddim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_ddim_step_x0": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_ddim_step_v": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_mse_loss_v_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int, c_int64, c_void_p]),
    "dq_mse_per_window_v": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int64, c_void_p]),
    "dq_unet_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_float,
                            c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_unet_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_int64, c_int, c_int, c_void_p]),
    "dq_mse_loss_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_mse_loss_weighted_fwd_bwd": (c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int, c_int64, c_void_p]),
    "dq_adamw_clip_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_float, c_float, c_void_p,
                                       c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "dq_plan_set_side_stream": (c_int, [c_void_p, c_int]),
    "dq_set_option": (c_int, [c_char_p, c_int64]),
    "dq_get_option": (c_int64, [c_char_p]),
    "dq_get_option_effective": (c_int64, [c_char_p]),
    "dq_adamw_clip_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_float, c_float, c_double,
                                   c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p]),
    "dq_adamw_clip_ema_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_float, c_float, c_double,
                                       c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "dq_adamw_clip_ema_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_float, c_float, c_void_p,
                                           c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "dq_train_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                              c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_eval_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_mse_per_window_scratch_bytes": (c_int64, [c_int, c_int64]),
    "dq_mse_per_window": (c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64,
                                  c_void_p]),
    "dq_recon_metrics_scratch_bytes": (c_int64, [c_int, c_int, c_int]),
    "dq_recon_metrics": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "dq_ms1_loss_fwd_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_void_p]),
    "dq_ddim_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),  # (plan, params, rope_freqs, const dq_sample_call*)
    "dq_randn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p]),
    "dq_ddim_step_sto": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64,
                                 c_void_p]),
    "dq_ddim_coef_table": (c_int, [POINTER(c_float), c_int, POINTER(c_int32), c_int, c_float, POINTER(c_float), POINTER(c_float)]),
    "dq_sampler_coef_table": (c_int, [POINTER(c_float), c_int, POINTER(c_int32), c_int, c_int, c_float, POINTER(c_float), POINTER(c_float)]),
    "dq_solver_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int64, c_void_p]),
    "dq_guided_update": (c_int, [c_int] + [c_void_p] * 8 + [c_float, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p]),
    "dq_solver_step_v": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "dq_guided_update_v": (c_int, [c_int] + [c_void_p] * 8 + [c_float, c_float, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p]),
    "dq_sample_stat_scratch_bytes": (c_int64, [c_int, c_int64]),
    "dq_window_rescale": (c_int, [c_void_p, c_void_p, c_float, c_double, c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_window_abs_quantile": (c_int, [c_void_p, c_int, c_int64, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_step_update_adaptive": (c_int, [c_int] + [c_void_p] * 8 + [c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p]),
    "dq_group_project": (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, c_int, c_int64, c_int, c_float, c_void_p]),
    "dq_ms1_cond_drop": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_float, c_int, c_int64, c_void_p]),
    "dq_pair_batch_scratch_bytes": (c_int64, [c_int]),
    "dq_pair_batch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int64, c_float, c_float, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_mix_batch_scratch_bytes": (c_int64, [c_int, c_int]),
    "dq_mix_batch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, POINTER(c_float), c_int,
                             c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 6 + [c_int64, c_void_p]),
    "dq_mix_group_batch_scratch_bytes": (c_int64, [c_int, c_int, c_int]),
    "dq_mix_group_batch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, POINTER(c_float),
                                   c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 6 + [c_int64, c_void_p]),
    "dq_group_metrics_scratch_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "dq_group_metrics": (c_int, [c_void_p] * 6 + [c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "dq_run_window_count": (c_int64, [c_int, c_int, c_int]),
    "dq_run_windows_scratch_bytes": (c_int64, [c_int]),
    "dq_run_windows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int] + [c_void_p] * 4 + [c_int64, c_void_p]),
    "dq_run_stitch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "dq_debug_tensor_offset": (c_int64, [c_void_p, c_char_p]),
    "dq_debug_level_plan": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int]),
    "dq_debug_side_tail_store": (c_int, [c_void_p, c_void_p, c_float, c_int]),
    "dq_debug_layout": (c_int, [c_void_p, c_int, c_int]),
    "dq_debug_mid_forms": (c_int, [c_void_p, c_int, c_int, POINTER(c_int32), c_int]),
    "dq_debug_sample_call_layout": (c_int, [POINTER(c_int32), c_int]),
    "dq_debug_mid_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_debug_mid_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_debug_wide_mid_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_debug_wide_mid_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "dq_tfm_create": (c_void_p, [c_int, c_int, c_int, c_int]),
    "dq_tfm_destroy": (None, [c_void_p]),
    "dq_tfm_num_params": (c_int, [c_void_p]),
    "dq_tfm_param_floats": (c_int64, [c_void_p]),
    "dq_tfm_param_info": (c_int, [c_void_p, c_int, c_char_p, c_int, POINTER(c_int64), POINTER(c_int), POINTER(c_int64)]),
    "dq_tfm_workspace_bytes": (c_int64, [c_void_p, c_int, c_int, c_int, c_int]),
    "dq_tfm_fwd": (c_int, [c_void_p] * 9 + [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "dq_tfm_bwd": (c_int, [c_void_p] * 8 + [c_int] + [c_void_p] * 3 + [c_int64, c_int, c_int, c_int, c_void_p]),
    "dq_gemm_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "dq_gemm": (c_int, [c_void_p] * 4 + [c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int64,
                        c_void_p]),
    "dq_gemm_bf16x3": (c_int, [c_void_p] * 4 + [c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int64,
                               c_void_p]),
    "dq_gemm_ex": (c_int, [c_void_p, c_void_p]),
    "dq_debug_gemm_plan": (c_int, [c_int] * 6 + [POINTER(c_int32), c_int, POINTER(c_int64)]),
    "dq_tfm_bwd_buckets": (c_int, [c_void_p] * 8 + [c_int] + [c_void_p] * 3 + [c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dq_tfm_num_buckets": (c_int, [c_void_p]),
    "dq_tfm_bucket_info": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "dq_tfm_set_precision": (c_int, [c_void_p, c_int]),
    "dq_tfm_layernorm_form": (c_int, [c_int, c_int]),
    "dq_tfm_rope_add": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p]),
    "dq_tfm_cond_embed": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p]),
    "dq_tfm_cond_embed_bwd": (c_int, [c_void_p] * 9 + [c_int64] + [c_int] * 4 + [c_void_p]),
    "dq_tfm_time_features": (c_int, [c_void_p] * 3 + [c_int, c_int, c_void_p]),
    "dq_tfm_gelu": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_tfm_gelu_bwd": (c_int, [c_void_p] * 3 + [c_int64, c_void_p]),
    "dq_tfm_layernorm_fwd": (c_int, [c_void_p] * 7 + [c_int, c_int, c_void_p]),
    "dq_tfm_layernorm_bwd": (c_int, [c_void_p] * 8 + [c_int64] + [c_int] * 3 + [c_void_p]),
    "dq_tfm_softmax_rows": (c_int, [c_void_p, c_int64, c_int, c_int, c_float, c_void_p]),
    "dq_tfm_softmax_rows_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_void_p]),
    "dq_tfm_colsum": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "dq_tfm_seqsum": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p, c_void_p]),
    "dq_tfm_attn_form": (c_int, [c_int, c_int, c_int]),
    "dq_tfm_attn_fwd": (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p]),
    "dq_tfm_sample_workspace_bytes": (c_int64, [c_void_p, c_int, c_int, c_int, c_int]),
    "dq_tfm_sample": (c_int, [c_void_p] * 5 + [c_int, c_void_p]),  # (..., S2, const dq_sample_call*)
    "dq_tfm_eval_workspace_bytes": (c_int64, [c_void_p, c_int, c_int, c_int, c_int]),
    "dq_tfm_eval_step": (c_int, [c_void_p] * 12 + [c_int] * 3 + [c_void_p] * 5 + [c_int64] + [c_int] * 4 + [c_void_p]),
    "dq_q_sample_repeats": (c_int, [c_void_p] * 6 + [c_int, c_void_p, c_int, c_int, c_int64, c_int, c_void_p]),
    "dq_mse_per_window_repeats": (c_int, [c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_int] + [c_void_p] * 5
                                  + [c_int, c_int, c_int64, c_void_p]),
    "dq_tfm_kv_broadcast": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p]),
    "dq_linattn_fwd": (c_int, [c_void_p] * 8 + [c_int, c_int, c_int, c_void_p]),
    "dq_linattn_bwd": (c_int, [c_void_p] * 15 + [c_int, c_int, c_int, c_void_p]),
    "dq_linattn_bwd_store": (c_int, [c_void_p] * 15 + [c_int, c_int, c_int, c_void_p]),
    "dq_linattn_forms": (c_int, [c_int] * 4 + [POINTER(c_int), POINTER(c_int)]),
    "dq_linattn_prep_floats": (c_int64, []),
    "dq_linattn_prepare": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "dq_linattn_fwd_prepared": (c_int, [c_void_p] * 9 + [c_int, c_int, c_int, c_void_p]),
    "dq_rmsnorm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "dq_time_mlp_fwd": (c_int, [c_void_p] * 8 + [c_int, c_void_p]),
    "dq_scale_shift_fwd": (c_int, [c_void_p] * 4 + [c_int, c_int, c_void_p]),
    "dq_ms1_feat_fwd": (c_int, [c_void_p] * 3 + [c_float, c_float] + [c_void_p] * 3 + [c_int, c_int, c_int, c_void_p]),
    "dq_ms1_feat_wgrad_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "dq_ms1_feat_wgrad": (c_int, [c_void_p] * 5 + [c_int64, c_int, c_int, c_int, c_void_p]),
    "dq_prep_inputs_fwd": (c_int, [c_void_p] * 4 + [c_float, c_float, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "dq_prep_inputs_bwd_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "dq_prep_inputs_bwd": (c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p] + [c_int] * 5 + [c_void_p, c_int64, c_void_p]),
    "dq_debug_time_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_void_p]),
    "dq_debug_time_bwd": (c_int, [c_void_p] * 5 + [c_int, c_void_p]),
    "dq_conv_fwd": (c_int, [c_void_p] * 4 + [c_int, c_void_p] + [c_int] * 7 + [c_void_p]),
    "dq_conv_bwd_workspace_floats": (c_int64, [c_int] * 9),
    "dq_conv_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 5 + [c_int] * 9 + [c_void_p, c_int64, c_void_p]),
    "dq_conv_bwd_forms": (c_int, [c_int] * 11 + [POINTER(c_int), POINTER(c_int)]),
    "dq_resblock_workspace_floats": (c_int64, [c_int] * 5),
    "dq_level_param_floats": (c_int64, [c_int] * 5),
    "dq_level_fwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_int64, c_void_p]),
    "dq_resblock_dout_offset": (c_int64, [c_int] * 5),
    "dq_resblock_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_int64, c_void_p]),
    "dq_resblock_forms": (c_int, [c_int] * 6 + [POINTER(c_int), POINTER(c_int)]),
    "dq_resblock_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 5 + [c_int] * 4 + [c_void_p, c_int64, c_void_p]),
    "dq_rope": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_float, c_void_p]),
    "dq_attn_fwd": (c_int, [c_void_p] * 5 + [c_int, c_int, c_void_p]),
    "dq_attn_bwd": (c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p]),
    "dq_wide_im2col3": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "dq_wide_col2im3": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    "dq_wide_repitch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "dq_wide_norm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "dq_wide_norm_bwd_scratch_floats": (c_int64, [c_int] * 3),
    "dq_wide_norm_bwd": (c_int, [c_void_p] * 4 + [c_int, c_int] + [c_void_p] * 5 + [c_int64] + [c_int] * 4 + [c_void_p]),
    "dq_wide_rowsum": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "dq_wide_sum_b": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
}


def lib():
    """Load (once) and return the shared library; raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libdq_hip.so not found at {LIB_PATH}: build it with `make -C diffusion-deconvolution-dia-msms-data_amd` "
                "(or python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
        import torch  # noqa: F401  (PyTorch's HIP runtime first: the library's libamdhip64 dependency must resolve to that same copy)

        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.dq_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {L.dq_abi_version()}, this package binds version {ABI_VERSION}: rebuild it")
        _lib = L
    return _lib


def build_id() -> str:
    """Identity of the native sources this tree was built from (sha256 over csrc/, include/dq_hip.h and the Makefile, 16 hex
    digits).  Profiles under profiles/ record it, and bench.py only quotes a counter-derived figure whose build id matches."""
    import hashlib

    root = os.path.dirname(_HERE)
    files = sorted(os.path.join(root, "csrc", f) for f in os.listdir(os.path.join(root, "csrc")) if f.endswith((".hip", ".h", ".cpp")))
    files += [os.path.join(root, "Makefile"), os.path.join(os.path.dirname(root), "include", "dq_hip.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def set_option(key: str, value: int) -> None:
    """``dq_set_option``: a process-wide tuning option of the library (keys: include/dq_hip.h)."""
    check(lib().dq_set_option(key.encode(), int(value)), f"dq_set_option({key!r})")


def get_option(key: str) -> int:
    return int(lib().dq_get_option(key.encode()))


def get_option_effective(key: str) -> int:
    """``dq_get_option_effective``: the threshold the library applies now (the default rule resolved); -1 for an unknown key."""
    return int(lib().dq_get_option_effective(key.encode()))


def resblock_forms(cinA: int, cinB: int, cout: int, rows: int, n: int, rows_per_sample: int):
    """``dq_resblock_forms``: the (forward, backward) kernel forms the stand-alone ResnetBlock calls take for this shape now, as names of
    RES_FWD_FORMS / RES_BWD_FORMS."""
    f, b = c_int(-1), c_int(-1)
    check(lib().dq_resblock_forms(cinA, cinB, cout, rows, n, rows_per_sample, ctypes.byref(f), ctypes.byref(b)), "dq_resblock_forms")
    return RES_FWD_FORMS[f.value], RES_BWD_FORMS[b.value]


def linattn_forms(C: int, rows: int, n: int, prepared: bool = True):
    """``dq_linattn_forms``: the (forward, backward) kernel forms of the stand-alone LinearAttention calls for this shape now, as names of
    LA_FWD_FORMS / LA_BWD_FORMS; the forward is dq_linattn_fwd_prepared's (prepared) or dq_linattn_fwd's."""
    f, b = c_int(-1), c_int(-1)
    check(lib().dq_linattn_forms(C, rows, n, int(prepared), ctypes.byref(f), ctypes.byref(b)), "dq_linattn_forms")
    return LA_FWD_FORMS[f.value], LA_BWD_FORMS[b.value]


def conv_bwd_forms(cout: int, cinA: int, cinB: int, K: int, mode: int, rows: int, n_in: int, n_out: int, rows_per_sample: int,
                   has_bias: bool = True, w_aligned: bool = True):
    """``dq_conv_bwd_forms``: the (data gradient, weight gradient) kernel forms ``dq_conv_bwd`` takes for this shape, as names of
    CONV_BWD_DATA_FORMS / CONV_WGRAD_FORMS."""
    d, g = c_int(-1), c_int(-1)
    check(lib().dq_conv_bwd_forms(cout, cinA, cinB, K, mode, rows, n_in, n_out, rows_per_sample, int(has_bias), int(w_aligned),
                                  ctypes.byref(d), ctypes.byref(g)), "dq_conv_bwd_forms")
    return CONV_BWD_DATA_FORMS[d.value], CONV_WGRAD_FORMS[g.value]


def level_plan(plan, B: int, RT: int, save: bool, twin: bool) -> dict:
    """``dq_debug_level_plan``: the launch the library gives every U-Net level in a pass over (B, RT) windows.  ``dn`` (levels 0 .. L-1)
    and ``up`` (levels 0 .. L-1, then the final ResnetBlock) are lists of dicts with the LEVEL_FORM_FIELDS (``kind`` as a name of
    LEVEL_KINDS, ``img`` an int, the rest bools); the pass-wide LEVEL_PLAN_FLAGS are bools at the top level."""
    cap = 1 + len(LEVEL_FORM_FIELDS) * 21 + len(LEVEL_PLAN_FLAGS)
    buf = (c_int32 * cap)()
    n = lib().dq_debug_level_plan(plan, int(B), int(RT), int(bool(save)), int(bool(twin)), buf, cap)
    if n < 0:
        raise RuntimeError(f"dq_debug_level_plan failed for B={B}, RT={RT}")
    L, nf = buf[0], len(LEVEL_FORM_FIELDS)
    if n != 1 + nf * (2 * L + 1) + len(LEVEL_PLAN_FLAGS):
        raise RuntimeError(f"dq_debug_level_plan wrote {n} ints for {L} levels")

    def form(i):
        v = buf[1 + nf * i: 1 + nf * (i + 1)]
        f = {k: bool(x) for k, x in zip(LEVEL_FORM_FIELDS, v)}
        f["kind"], f["img"] = LEVEL_KINDS[v[0]], int(v[1])
        return f

    out = {"levels": int(L), "dn": [form(i) for i in range(L)], "up": [form(L + i) for i in range(L + 1)]}
    out.update({k: bool(x) for k, x in zip(LEVEL_PLAN_FLAGS, buf[1 + nf * (2 * L + 1): n])})
    return out


def mid_forms(plan, B: int, RT: int) -> dict:
    """``dq_debug_mid_forms``: which pieces of the bottleneck attention ride in a ResnetBlock's launch in a pass over (B, RT) windows (bools),
    with ``mid_c``, ``cond_dim``, the blocks' offsets in a sample's scale / shift vector and its length (ints): MID_FORMS_FIELDS."""
    buf = (c_int32 * len(MID_FORMS_FIELDS))()
    n = lib().dq_debug_mid_forms(plan, int(B), int(RT), buf, len(MID_FORMS_FIELDS))
    if n != len(MID_FORMS_FIELDS):
        raise RuntimeError(f"dq_debug_mid_forms failed for B={B}, RT={RT}")
    out = dict(zip(MID_FORMS_FIELDS, (int(x) for x in buf)))
    for k in ("qkv_fused", "out_fused", "pre_fused", "wide_mid", "prep_ok"):
        out[k] = bool(out[k])
    return out


class GemmDesc(ctypes.Structure):
    """``dq_gemm_desc`` of include/dq_hip.h, field for field."""
    _fields_ = ([(k, c_void_p) for k in ("A", "B", "C", "bias", "bias_m", "add", "scratch")]
                + [(k, c_int64) for k in ("scratch_floats", "lda", "ldb", "ldc", "sAo", "sAi", "sBo", "sBi", "sCo", "sCi", "sAk", "sBk")]
                + [(k, c_int32) for k in ("M", "N", "K", "a_kmajor", "b_kmajor", "batch", "inner", "kbatch", "accumulate", "splits", "precision")]
                + [("alpha", c_float)])


def gemm_desc(**fields) -> GemmDesc:
    """A ``dq_gemm_desc`` with the defaults of a plain fp32 product (k-major operands, batch = inner = kbatch = 1, alpha = 1), then ``fields``;
    pointers are given as integers (``tensor.data_ptr()``) or None."""
    d = GemmDesc(a_kmajor=1, b_kmajor=1, batch=1, inner=1, kbatch=1, alpha=1.0)
    for k, v in fields.items():
        if not hasattr(d, k):
            raise AttributeError(f"dq_gemm_desc has no field {k!r}")
        setattr(d, k, v)
    return d


class SampleCall(ctypes.Structure):
    """``dq_sample_call`` of include/dq_hip.h, field for field (``dq_debug_sample_call_layout`` is the library's side of the layout)."""
    _fields_ = [("struct_bytes", c_int32), ("alpha_bars_host", c_void_p), ("num_timesteps", c_int32), ("x_T", c_void_p), ("ms2_cond", c_void_p),
                ("ms1_cond", c_void_p), ("auto_normalize", c_int32), ("pred_type", c_int32), ("timesteps_host", c_void_p), ("num_steps", c_int32),
                ("out_x", c_void_p), ("out_noise", c_void_p), ("traj_x", c_void_p), ("traj_eps", c_void_p), ("use_graph", c_int32),
                ("workspace", c_void_p), ("workspace_bytes", c_int64), ("B", c_int32), ("RT", c_int32), ("stream", c_void_p), ("eta", c_float),
                ("seed_dev", c_void_p), ("window_ids_dev", c_void_p), ("sampler", c_int32), ("clip_x0", c_float), ("guided", c_int32),
                ("guidance_scale", c_float), ("null_ms1", c_float), ("guidance_rescale", c_double), ("threshold_quantile", c_float),
                ("threshold_max", c_float), ("stat_scratch", c_void_p), ("stat_scratch_bytes", c_int64), ("group_size", c_int32),
                ("consistency", c_int32), ("consistency_strength", c_float)]


def sample_call(**fields) -> SampleCall:
    """A ``dq_sample_call`` with ``struct_bytes`` set and every option at its off value (all zero / NULL, ``group_size`` 1), then ``fields``;
    pointers are given as integers (``tensor.data_ptr()``, ``ctypes.addressof`` of a host array the caller keeps alive) or None."""
    q = SampleCall(struct_bytes=ctypes.sizeof(SampleCall), group_size=1)
    for k, v in fields.items():
        if not hasattr(q, k):
            raise AttributeError(f"dq_sample_call has no field {k!r}")
        setattr(q, k, v)
    return q


def sample_call_layout():
    """``dq_debug_sample_call_layout``: ``(sizeof, [(offset, size), ...])`` of ``dq_sample_call`` as the library was compiled."""
    cap = 1 + 2 * len(SampleCall._fields_) + 16
    buf = (c_int32 * cap)()
    n = lib().dq_debug_sample_call_layout(buf, cap)
    if n < 1 or n % 2 != 1:
        raise RuntimeError("dq_debug_sample_call_layout failed")
    return int(buf[0]), [(int(buf[i]), int(buf[i + 1])) for i in range(1, n, 2)]


def gemm_ex(desc: GemmDesc, stream=None) -> int:
    """``dq_gemm_ex``: returns the library's code (0 = done); the caller decides whether a refusal is an error (``check``)."""
    return int(lib().dq_gemm_ex(ctypes.byref(desc), stream))


def gemm_plan(M: int, N: int, K: int, batch: int = 1, kbatch: int = 1, splits: int = 0) -> dict:
    """``dq_debug_gemm_plan``: ``bm``, ``kv``, the ``full`` and ``rest`` launches (dicts of GEMM_PLAN_PART_FIELDS) and the ``scratch``
    floats of the product, as the launcher itself plans it."""
    buf, scratch = (c_int32 * 10)(), c_int64(-1)
    n = lib().dq_debug_gemm_plan(int(M), int(N), int(K), int(batch), int(kbatch), int(splits), buf, 10, ctypes.byref(scratch))
    if n != 2 + 2 * len(GEMM_PLAN_PART_FIELDS):
        raise RuntimeError(f"dq_debug_gemm_plan failed for M={M}, N={N}, K={K}, batch={batch}, kbatch={kbatch}, splits={splits}")
    nf = len(GEMM_PLAN_PART_FIELDS)
    return {"bm": int(buf[0]), "kv": int(buf[1]), "full": dict(zip(GEMM_PLAN_PART_FIELDS, (int(x) for x in buf[2:2 + nf]))),
            "rest": dict(zip(GEMM_PLAN_PART_FIELDS, (int(x) for x in buf[2 + nf:2 + 2 * nf]))), "scratch": int(scratch.value)}


def last_error():
    msg = lib().dq_last_error()
    return msg.decode() if msg else "?"


def check(rc, what):
    if rc != 0:
        msg = lib().dq_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device/host pointer of a contiguous torch tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream_ptr():
    import torch

    return c_void_p(torch.cuda.current_stream().cuda_stream)
