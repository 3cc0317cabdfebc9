"""ctypes bindings of include/pmgt_capi.h.

The HIP library is the ONLY compute path of this package: if it is missing or cannot be loaded the
import of anything that needs it raises — there is no eager/PyTorch or CPU fallback.
"""
import ctypes as C
import os

from . import _build

c_i64p = C.POINTER(C.c_int64)
c_f32p = C.POINTER(C.c_float)


MAX_FEATS = 4      # PMGT_MAX_FEATS (include/pmgt_capi.h)


class PMGTConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("num_hidden_layers", C.c_int), ("num_attention_heads", C.c_int),
                ("intermediate_size", C.c_int), ("n_feats", C.c_int), ("feat_sizes", C.c_int * MAX_FEATS),
                ("max_position_embeddings", C.c_int), ("layer_norm_eps", C.c_float), ("beta", C.c_float),
                ("hidden_dropout_prob", C.c_float), ("attention_probs_dropout_prob", C.c_float), ("dtype", C.c_int)]


class TensorsC(C.Structure):
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("tables", C.c_void_p * MAX_FEATS),
                ("n_nodes", C.c_int64), ("rng_state", C.c_void_p), ("table_scales", C.c_float * MAX_FEATS)]


class BatchC(C.Structure):
    _fields_ = [("n_targets", C.c_int), ("n_pairs", C.c_int), ("seq_len", C.c_int),
                ("tgt_ids", C.c_void_p), ("tgt_mask", C.c_void_p), ("pair_ids", C.c_void_p), ("pair_mask", C.c_void_p),
                ("num_pairs", C.c_void_p), ("labels", C.c_void_p), ("nfr_masked_ids", C.c_void_p),
                ("nfr_targets", C.c_void_p), ("random_node_ratio", C.c_float), ("mask_node_ratio", C.c_float)]


class OutputsC(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("logits", C.c_void_p), ("last_hidden", C.c_void_p), ("nfr_count", C.c_void_p)]


class EmbedArgsC(C.Structure):
    """pmgt_embed_args (include/pmgt_ops.h): arguments of pmgt_op_embed_mix_fwd / _bwd."""
    _fields_ = [("dtype", C.c_int), ("phase", C.c_int), ("M", C.c_int), ("S", C.c_int), ("d", C.c_int), ("nf", C.c_int),
                ("E", C.c_void_p), ("e_rows", C.c_void_p), ("Wa", C.c_void_p), ("ba", C.c_void_p), ("pos", C.c_void_p),
                ("role", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("eps", C.c_float), ("a", C.c_void_p),
                ("pre", C.c_void_p), ("stats", C.c_void_p), ("h0", C.c_void_p), ("drop_p", C.c_float), ("drop_site", C.c_uint32),
                ("rng", C.c_void_p), ("dh0", C.c_void_p), ("dE", C.c_void_p), ("dF", C.c_void_p), ("dF_f32", C.c_int),
                ("part", C.c_void_p)]


class MirrorDescC(C.Structure):
    """pmgt_mirror_desc (include/pmgt_ops.h): one weight of pmgt_op_mirror."""
    _fields_ = [("src", C.c_int64), ("rows", C.c_int), ("cols", C.c_int), ("dst", C.c_int64), ("dst_t", C.c_int64),
                ("dst_t_hm", C.c_int64), ("hm_d", C.c_int), ("hm_dh", C.c_int), ("tile_start", C.c_int)]


class AdamC(C.Structure):
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("decay", C.c_void_p),
                ("lr", C.c_float), ("weight_decay", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("max_grad_norm", C.c_float), ("step", C.c_void_p), ("scalars", C.c_void_p),
                ("scratch", C.c_void_p)]


class LrScheduleC(C.Structure):
    """pmgt_lr_schedule (include/pmgt_capi.h); type = index in LR_SCHEDULE_TYPES."""
    _fields_ = [("type", C.c_int), ("num_warmup_steps", C.c_int64), ("num_training_steps", C.c_int64)]


class StepGuardC(C.Structure):
    """pmgt_step_guard (include/pmgt_capi.h): device counters int64 [4], log ring fp32 [rows][STEP_LOG_FLOATS] + int64 [rows][2]."""
    _fields_ = [("counters", C.c_void_p), ("log_f", C.c_void_p), ("log_i", C.c_void_p), ("log_rows", C.c_int64), ("loss", C.c_void_p),
                ("skip_nonfinite", C.c_int)]


class AvgStepC(C.Structure):
    """pmgt_avg_step (include/pmgt_capi.h): mode = index in AVG_MODES; state = the AVG_STATE_BYTES device buffer of the "ema" mode."""
    _fields_ = [("mode", C.c_int), ("warmup", C.c_int), ("decay", C.c_double), ("state", C.c_void_p), ("skip_flag", C.c_void_p),
                ("w_old", C.c_float), ("w_new", C.c_float)]


class NcfHeadC(C.Structure):
    """pmgt_ncf_head (include/pmgt_capi.h): kind = index in NCF_KINDS; device pointers of the head's parameters in state_dict layout."""
    _fields_ = [("factor_num", C.c_int), ("num_layers", C.c_int), ("kind", C.c_int), ("reserved", C.c_int),
                ("weight", C.c_void_p * 4), ("bias", C.c_void_p * 4), ("predict_weight", C.c_void_p), ("predict_bias", C.c_void_p),
                ("gmf_user", C.c_void_p), ("gmf_item", C.c_void_p), ("user_num", C.c_int64)]


class NcfTrainC(C.Structure):
    """pmgt_ncf_train (include/pmgt_capi.h)."""
    _fields_ = [("factor_num", C.c_int), ("num_layers", C.c_int), ("kind", C.c_int), ("reserved", C.c_int), ("user_num", C.c_int64),
                ("item_num", C.c_int64), ("table", C.c_void_p), ("params", C.c_void_p), ("grads", C.c_void_p)]


class NcfModelC(C.Structure):
    """pmgt_ncf_model (include/pmgt_capi.h): kind = index in NCF_MODEL_KINDS."""
    _fields_ = [("factor_num", C.c_int), ("num_layers", C.c_int), ("kind", C.c_int), ("use_layer_norm", C.c_int), ("layer_norm_eps", C.c_float),
                ("train_items", C.c_int), ("user_num", C.c_int64), ("item_num", C.c_int64), ("item_table", C.c_void_p), ("params", C.c_void_p),
                ("grads", C.c_void_p), ("table_grad", C.c_void_p)]


class NcfModelHeadC(C.Structure):
    """pmgt_ncf_model_head (include/pmgt_capi.h): kind = index in NCF_MODEL_KINDS; device pointers of the NCF class's parameters in state_dict layout."""
    _fields_ = [("factor_num", C.c_int), ("num_layers", C.c_int), ("kind", C.c_int), ("use_layer_norm", C.c_int), ("layer_norm_eps", C.c_float),
                ("reserved", C.c_int), ("user_num", C.c_int64), ("weight", C.c_void_p * 4), ("bias", C.c_void_p * 4), ("gamma", C.c_void_p * 4),
                ("beta", C.c_void_p * 4), ("predict_weight", C.c_void_p), ("predict_bias", C.c_void_p), ("gmf_user", C.c_void_p),
                ("gmf_item", C.c_void_p)]


class NcfDropoutC(C.Structure):
    """pmgt_ncf_dropout (include/pmgt_capi.h): rng = the device {seed, step} pair."""
    _fields_ = [("rng", C.c_void_p), ("p_emb", C.c_float), ("p_layer", C.c_float * 4)]


class AdamSegmentC(C.Structure):
    """pmgt_adam_segment (include/pmgt_ops.h): one flat buffer of pmgt_op_adamw_segments."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("decay", C.c_void_p), ("n", C.c_int64),
                ("lr_scale", C.c_float)]


ADAM_MAX_SEGMENTS = 8      # PMGT_ADAM_MAX_SEGMENTS
OPTIMS = ("adamw", "sgd")      # PMGT_OPTIM_* in order: the `optim` of pmgt_op_step_segments


class DcnHeadC(C.Structure):
    """pmgt_dcn_head (include/pmgt_capi.h)."""
    _fields_ = [("factor_num", C.c_int), ("deep_layers", C.c_int), ("cross_layers", C.c_int), ("use_layer_norm", C.c_int),
                ("layer_norm_eps", C.c_float), ("reserved", C.c_int), ("user_num", C.c_int64), ("item_num", C.c_int64),
                ("params", C.c_void_p), ("grads", C.c_void_p)]


class DcnDropoutC(C.Structure):
    """pmgt_dcn_dropout (include/pmgt_capi.h): rng = the device {seed, step} pair."""
    _fields_ = [("rng", C.c_void_p), ("p_emb", C.c_float), ("p_deep", C.c_float * 4), ("p_cross", C.c_float * 6)]


NCF_KINDS = ("MLP", "NeuMF-end")      # PMGT_NCF_* in order
NCF_MAX_LAYERS, NCF_MAX_USERS = 4, 1 << 20      # PMGT_NCF_MAX_LAYERS, PMGT_NCF_MAX_USERS
NCF_FACTORS, NCF_MAX_D = (8, 16, 32, 64), 256      # the covered heads (pmgt_ncf_score's comment): factor_num, d = factor_num * 2^(num_layers - 1)
NCF_TRAIN_MAX_PAIRS, NCF_TRAIN_TENSORS = 65536, 13      # PMGT_NCF_TRAIN_*
NCF_MODEL_KINDS, NCF_MODEL_TENSORS = ("MLP", "NeuMF-end", "GMF", "NeuMF-pre"), 22      # PMGT_NCF_* in order (pmgt_ncf_model.kind), PMGT_NCF_MODEL_TENSORS
NCF_SITE_EMB, NCF_SITE_GMF, NCF_SITE_LAYER = 64, 65, 72      # NCF_SITE_* of ops/ncf_head.h (documented in include/pmgt_capi.h): the dropout sites of the trained head; layer l = NCF_SITE_LAYER + l
DCN_MAX_DEEP, DCN_MAX_CROSS, DCN_TENSORS, DCN_MAX_PAIRS = 4, 6, 38, 65536      # PMGT_DCN_*
DCN_SITE_EMB, DCN_SITE_DEEP, DCN_SITE_CROSS = 64, 72, 80      # DCN_SITE_* of ops/ncf_head.h (documented in include/pmgt_capi.h): the dropout sites of the DCN; deep layer l = DCN_SITE_DEEP + l, cross layer c = DCN_SITE_CROSS + c
DCN_SCORE_ROW_STRIDE = 12      # PMGT_DCN_SCORE_ROW_STRIDE: floats a row of pmgt_dcn_score_rows (mu, q, d_0 .. d_C, zeros)
DCN_FACTORS, DCN_MAX_E = (8, 16, 32, 64), 256      # the covered shapes (pmgt_dcn_train_grad's comment): factor_num, E = factor_num * 2^deep_layers
TOPK_MAX_K, TOPK_FLAG_NAN, TOPK_FLAG_SHORT = 1024, 1, 2      # PMGT_TOPK_*
RANK_HELDOUT_CHUNK, RANK_HELDOUT_FLAG_EXCLUDED, RANK_HELDOUT_HEADER_BYTES = 1024, 4, 128      # PMGT_RANK_HELDOUT_*
ITEM_GRAPH_MIN_SLOTS, ITEM_GRAPH_MAX_SLOTS = 16, 1024      # PMGT_ITEM_GRAPH_*_SLOTS
ITEM_SIM_MAX_D = 1024      # PMGT_ITEM_SIM_MAX_D
HISTORY_AGGS = ("mean", "max")      # PMGT_HISTORY_* in order

AVG_MODES = ("swa", "ema")      # PMGT_AVG_* in order
AVG_STATE_BYTES = 32            # PMGT_AVG_STATE_BYTES: int64 n_upd; 32-bit words [2] skip word, [3] w_old, [4] w_new, [5..7] reserved

STEP_LOG_FLOATS = 8      # PMGT_STEP_LOG_FLOATS: loss, pre-clip norm, clip coefficient, lr_t, flag, 3 reserved
STEP_LOG_APPLIED, STEP_LOG_SKIPPED, STEP_LOG_APPLIED_NONFINITE = 0, 1, 2      # the flag column

# PMGT_LR_* in order: the choices of the reference's --scheduler-type (train.py:38-52)
LR_SCHEDULE_TYPES = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")

DTYPE_F32, DTYPE_BF16, DTYPE_FP8 = 0, 1, 2
# void (*pmgt_grad_ready_fn)(void* user, int64_t offset, int64_t numel)  (include/pmgt_capi.h)
GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)
FLAG_TRAINING, FLAG_BACKWARD, FLAG_ACCUMULATE = 1, 2, 4
EPI_NONE, EPI_GELU, EPI_GELU_GRAD = 0, 1, 2

# every symbol include/pmgt_capi.h (product ABI) and include/pmgt_ops.h (single-kernel test entries) declare for libpmgt_hip.so
HIP_SYMBOLS = [
    "pmgt_last_error", "pmgt_abi_version", "pmgt_engine_create", "pmgt_engine_destroy", "pmgt_param_count",
    "pmgt_param_num_entries", "pmgt_param_entry", "pmgt_workspace_bytes", "pmgt_pretrain_step", "pmgt_encode_ids",
    "pmgt_encode_feats", "pmgt_encode_train", "pmgt_encode_backward", "pmgt_optimizer_step", "pmgt_optimizer_step_scheduled", "pmgt_optimizer_step_guarded", "pmgt_profile_begin",
    "pmgt_profile_end", "pmgt_profile_sequence", "pmgt_profile_records", "pmgt_cast_from_f32", "pmgt_cast_to_f32", "pmgt_quantize_e4m3", "pmgt_dequantize_e4m3",
    "pmgt_engine_set_grad_ready_callback", "pmgt_engine_set_option", "pmgt_engine_get_option",
    "pmgt_eval_workspace_bytes", "pmgt_eval_reset", "pmgt_eval_append", "pmgt_eval_reduce",
    "pmgt_weight_average_update", "pmgt_weight_swap",
    "pmgt_rank_workspace_bytes", "pmgt_rank_reset", "pmgt_rank_append", "pmgt_rank_reduce",
    "pmgt_ncf_score", "pmgt_topk_workspace_bytes", "pmgt_topk_rows", "pmgt_rank_heldout", "pmgt_rank_heldout_reduce",
    "pmgt_item_graph_default_slots", "pmgt_item_graph_count", "pmgt_item_graph_fill", "pmgt_item_sim_norms", "pmgt_item_sim_score", "pmgt_history_score",
    "pmgt_knn_score", "pmgt_knn_score_tile",
    "pmgt_ncf_train_layout", "pmgt_ncf_train_workspace_bytes", "pmgt_ncf_train_grad",
    "pmgt_ncf_train_table_workspace_bytes", "pmgt_ncf_train_grad_table", "pmgt_ncf_train_grad_dropout",
    "pmgt_ncf_train_rows_workspace_bytes", "pmgt_ncf_train_grad_rows",
    "pmgt_ncf_model_layout", "pmgt_ncf_model_workspace_bytes", "pmgt_ncf_model_train_grad", "pmgt_ncf_model_score",
    "pmgt_dcn_layout", "pmgt_dcn_workspace_bytes", "pmgt_dcn_forward", "pmgt_dcn_train_grad",
    "pmgt_dcn_train_grad_dropout", "pmgt_dcn_score_rows", "pmgt_dcn_score",
]
OPS_SYMBOLS = [
    "pmgt_op_gemm_nt", "pmgt_op_gemm_tn_slab_elems", "pmgt_op_gemm_tn", "pmgt_op_gemm_tn_bias", "pmgt_op_colsum",
    "pmgt_op_layernorm_fwd", "pmgt_op_layernorm_bwd", "pmgt_op_linear", "pmgt_op_linear_ln_bwd", "pmgt_op_attention_fwd", "pmgt_op_attention_bwd",
    "pmgt_op_qkvc_attention_fwd", "pmgt_op_attention_bwd_wgrad", "pmgt_op_attention_bwd_wgrad_parts",
    "pmgt_op_quant_rows_e4m3", "pmgt_op_gemm_nt_f8", "pmgt_op_gemm_tn_f8", "pmgt_op_qkvc_attention_fwd_f8",
    "pmgt_launch_trace_reset", "pmgt_launch_trace_count", "pmgt_op_seg_sort", "pmgt_op_seg_sort_temp_bytes", "pmgt_op_clock_probe", "pmgt_op_qkvc_attention_fwd_ex", "pmgt_op_attention_bwd_wgrad_vc2_parts",
    "pmgt_op_embed_mix_fwd", "pmgt_op_embed_mix_bwd", "pmgt_op_embed_part_elems", "pmgt_op_embed_bwd_parts", "pmgt_op_pos_role_finish",
    "pmgt_op_seg_part_elems", "pmgt_op_seg_sum", "pmgt_op_pair_offsets", "pmgt_op_nfr_compact", "pmgt_op_gsr", "pmgt_op_nfr_diff_parts",
    "pmgt_op_nfr_diff", "pmgt_op_loss_finish", "pmgt_op_scatter_rows", "pmgt_op_adamw", "pmgt_op_mirror",
    "pmgt_op_adamw_scheduled", "pmgt_op_lr_schedule", "pmgt_op_nfr_generate", "pmgt_op_build_need_rows", "pmgt_op_dropout_keep",
    "pmgt_op_adamw_guarded", "pmgt_op_eval_append_scores", "pmgt_op_eval_small_max",
    "pmgt_op_linear_rows", "pmgt_op_layernorm_bwd_rows", "pmgt_op_gemm_tn_bias_rows",
    "pmgt_op_adamw_segments", "pmgt_op_cls_gather", "pmgt_op_cls_scatter", "pmgt_op_sgd", "pmgt_op_step_segments",
]
# path options: pmgt_engine_set_option keys -> bit in the `path_opts` argument of the pmgt_op_* entries (include/pmgt_ops.h)
OPT = {k: 1 << i for i, k in enumerate((
    "tile_gemm", "valu_attention", "wave_attention_bwd", "no_shortcut", "no_fused_qkvc_attention", "no_head_major",
    "no_table_projection", "no_segment_sum", "consumer_quant", "no_fused_attention_bwd", "store_ln_input", "eager_reduce",
    "side_stream_reduce", "unfused_ln", "one_bucket", "small_arena", "no_role_split_ln", "no_tile_attention", "unfused_ln_bwd", "lockstep_attention_bwd", "side_stream_wgrad", "no_cls_only_attention_bwd", "no_beta_skip", "no_vc2_attention_bwd"))}
SAMPLER_SYMBOLS = [
    "pmgt_sampler_create", "pmgt_sampler_destroy", "pmgt_sampler_last_error", "pmgt_sampler_seed",
    "pmgt_sampler_context", "pmgt_sampler_batch", "pmgt_sampler_batch_mt", "pmgt_sampler_max_pairs",
    "pmgt_sampler_random_sample", "pmgt_sampler_randint", "pmgt_train_valid_split",
]

_hip = None
_sampler = None


def _load(path, what):
    if not os.path.exists(path):
        raise ImportError(f"{what} not built: {path} is missing. Run `python __graft_entry__.py` "
                          f"(or pmgt_amd._build.build_all()); pmgt_amd has no fallback path.")
    try:
        return C.CDLL(path)
    except OSError as e:   # fail loudly: no CPU/eager fallback exists
        raise ImportError(f"cannot load {what} ({path}): {e}") from e


def hip():
    """libpmgt_hip.so with argtypes set."""
    global _hip
    if _hip is not None:
        return _hip
    # PyTorch-ROCm first: it brings its own libamdhip64 / libhsa-runtime64.  If this library is loaded before torch, the
    # loader binds the system ROCm runtime instead and torch's later import mixes the two (device init then fails with
    # "no usable HIP device"); loaded after torch, the same SONAME resolves to the copy torch already mapped.
    import torch  # noqa: F401
    L = _load(_build.hip_lib_path(), "HIP engine library")
    vp, i, i64, f, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
    L.pmgt_last_error.restype = C.c_char_p
    L.pmgt_abi_version.restype = i
    L.pmgt_engine_create.restype = vp
    L.pmgt_engine_create.argtypes = [C.POINTER(PMGTConfigC)]
    L.pmgt_engine_destroy.argtypes = [vp]
    L.pmgt_engine_destroy.restype = None
    L.pmgt_param_count.restype = i64
    L.pmgt_param_count.argtypes = [vp]
    L.pmgt_param_num_entries.argtypes = [vp]
    L.pmgt_param_entry.argtypes = [vp, i, C.c_char_p, i, c_i64p, c_i64p, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.pmgt_workspace_bytes.restype = i64
    L.pmgt_workspace_bytes.argtypes = [vp, i, i, i, i]
    L.pmgt_pretrain_step.argtypes = [vp, C.POINTER(TensorsC), C.POINTER(BatchC), C.POINTER(OutputsC), vp, i64, i, vp]
    L.pmgt_encode_ids.argtypes = [vp, C.POINTER(TensorsC), vp, vp, i, i, vp, vp, vp, vp, i64, vp]
    featp = C.POINTER(C.c_void_p)      # const void* const* feats: host array of n_feats device pointers, or NULL
    L.pmgt_encode_feats.argtypes = [vp, C.POINTER(TensorsC), featp, vp, i, i, vp, vp, vp, vp, i64, vp]
    L.pmgt_encode_train.argtypes = [vp, C.POINTER(TensorsC), vp, featp, vp, i, i, vp, vp, i64, i, vp]
    L.pmgt_encode_backward.argtypes = [vp, C.POINTER(TensorsC), featp, vp, i, i, vp, i64, i, vp]
    L.pmgt_optimizer_step.argtypes = [vp, C.POINTER(TensorsC), C.POINTER(AdamC), vp]
    L.pmgt_optimizer_step_scheduled.argtypes = [vp, C.POINTER(TensorsC), C.POINTER(AdamC), C.POINTER(LrScheduleC), vp]
    L.pmgt_optimizer_step_guarded.argtypes = [vp, C.POINTER(TensorsC), C.POINTER(AdamC), C.POINTER(LrScheduleC), C.POINTER(StepGuardC), vp]
    L.pmgt_profile_begin.argtypes = [vp]
    L.pmgt_profile_end.argtypes = [vp, C.c_char_p, i]
    L.pmgt_profile_sequence.argtypes = [vp, C.c_char_p, i]
    L.pmgt_profile_records.argtypes = [vp, C.c_char_p, i]
    L.pmgt_cast_from_f32.argtypes = [i, vp, vp, i64, vp]
    L.pmgt_cast_to_f32.argtypes = [i, vp, vp, i64, vp]
    L.pmgt_op_gemm_nt.argtypes = [i, vp, i64, vp, vp, i64, vp, i64, i, i, i, vp, i, vp, i64, vp, i64, f, u32, vp, vp, u32, vp]
    L.pmgt_op_gemm_tn_slab_elems.restype = i64
    L.pmgt_op_gemm_tn_slab_elems.argtypes = [i, i, i, i, u32]
    L.pmgt_op_gemm_tn.argtypes = [i, vp, i64, vp, i64, vp, i, i, i, vp, vp, i, vp, u32, vp]
    L.pmgt_op_colsum.argtypes = [i, vp, i64, i, i, vp, vp, vp]
    L.pmgt_op_layernorm_fwd.argtypes = [i, vp, vp, vp, vp, vp, i, i, f, f, u32, vp, vp]
    L.pmgt_op_layernorm_bwd.argtypes = [i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, f, u32, f, u32, vp, vp]
    L.pmgt_op_qkvc_attention_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, u32, u32, vp, vp]
    L.pmgt_engine_set_grad_ready_callback.argtypes = [vp, GRAD_READY_FN, vp]
    L.pmgt_engine_set_grad_ready_callback.restype = None
    L.pmgt_engine_set_option.argtypes = [vp, C.c_char_p, i]
    L.pmgt_engine_get_option.argtypes = [vp, C.c_char_p]
    L.pmgt_op_linear.argtypes = [i, vp, i64, vp, i64, vp, i64, i, i, i, vp, i, vp, i64, vp, i64, f, u32, vp, vp, vp, vp, vp, f, u32, vp]
    L.pmgt_launch_trace_count.argtypes = [C.c_char_p]
    L.pmgt_launch_trace_count.restype = C.c_int64
    L.pmgt_launch_trace_reset.restype = None
    L.pmgt_op_clock_probe.argtypes = [vp, i, vp]
    L.pmgt_op_qkvc_attention_fwd_ex.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, u32, u32, vp, i, vp]
    L.pmgt_op_seg_sort_temp_bytes.argtypes = [i]
    L.pmgt_op_seg_sort_temp_bytes.restype = i64
    L.pmgt_op_seg_sort.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, i64, vp]
    L.pmgt_op_linear_ln_bwd.argtypes = [vp, i64, vp, i64, i, i, i, vp, i64, vp, vp, vp, vp, vp, vp, vp, f, u32, vp, vp, vp, u32, vp]
    L.pmgt_op_attention_fwd.argtypes = [i, vp, vp, vp, vp, i, i, i, i, f, f, u32, u32, vp, u32, vp]
    L.pmgt_op_attention_bwd.argtypes = [i, vp, vp, vp, vp, i, i, i, i, f, f, u32, u32, vp, u32, vp]
    L.pmgt_op_attention_bwd_wgrad.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, f, f, u32, u32, vp, i, vp]
    L.pmgt_op_attention_bwd_wgrad_parts.argtypes = [i]
    L.pmgt_op_attention_bwd_wgrad_vc2_parts.argtypes = [i]
    L.pmgt_op_gemm_tn_bias.argtypes = [i, vp, i64, vp, i64, i, i, i, vp, vp, vp, vp, i, i, u32, vp]
    L.pmgt_op_linear_rows.argtypes = [i, vp, i64, vp, vp, i64, vp, i64, i, i, i, vp, i, vp, i64, vp, i64, i, f, u32, vp, vp, vp, vp, vp, f, vp, u32, vp]
    L.pmgt_op_layernorm_bwd_rows.argtypes = [i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, f, u32, f, u32, vp, vp, vp]
    L.pmgt_op_gemm_tn_bias_rows.argtypes = [i, vp, i64, vp, i64, vp, i, i, i, i, vp, vp, vp, vp, i, vp, u32, vp]
    L.pmgt_quantize_e4m3.argtypes = [vp, vp, i64, f, vp]
    L.pmgt_dequantize_e4m3.argtypes = [vp, vp, i64, f, vp]
    L.pmgt_op_quant_rows_e4m3.argtypes = [i, vp, i64, i, i, vp, i64, vp, vp]
    L.pmgt_op_gemm_nt_f8.argtypes = [vp, i64, vp, vp, f, vp, i64, vp, vp, i64, i, i, i, vp, vp, vp]
    L.pmgt_op_gemm_tn_f8.argtypes = [vp, i64, vp, i64, f, vp, i, i, i, vp, vp, i, vp, vp]
    L.pmgt_op_qkvc_attention_fwd_f8.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, u32, u32, vp, vp]
    L.pmgt_op_embed_mix_fwd.argtypes = [C.POINTER(EmbedArgsC), vp]
    L.pmgt_op_embed_mix_bwd.argtypes = [C.POINTER(EmbedArgsC), vp]
    L.pmgt_op_embed_part_elems.argtypes = [i, i]
    L.pmgt_op_embed_bwd_parts.argtypes = [i]
    L.pmgt_op_pos_role_finish.argtypes = [vp, i, i, i, vp, vp, i, vp]
    L.pmgt_op_seg_part_elems.argtypes = [i, i]
    L.pmgt_op_seg_part_elems.restype = i64
    L.pmgt_op_seg_sum.argtypes = [i, i, vp, i64, vp, vp, vp, i, i, i, vp, vp, vp]
    L.pmgt_op_pair_offsets.argtypes = [vp, i, vp, vp]
    L.pmgt_op_nfr_compact.argtypes = [vp, i, i, i, vp, vp, vp, vp]
    L.pmgt_op_gsr.argtypes = [i, vp, vp, i, i, i, i64, vp, vp, vp, vp, vp]
    L.pmgt_op_nfr_diff_parts.argtypes = [i]
    L.pmgt_op_nfr_diff.argtypes = [i, vp, vp, vp, i, i, C.POINTER(i), C.POINTER(vp), i, c_f32p, vp, vp]
    L.pmgt_op_loss_finish.argtypes = [vp, i, vp, i, vp, i, C.POINTER(i), i, vp, vp, vp]
    L.pmgt_op_scatter_rows.argtypes = [i, vp, vp, vp, i, i, vp, i, vp]
    L.pmgt_op_adamw.argtypes = [vp, vp, vp, vp, vp, i64, f, f, f, f, f, f, vp, vp, vp, vp]
    L.pmgt_op_adamw_scheduled.argtypes = [vp, vp, vp, vp, vp, i64, f, f, f, f, f, f, vp, vp, vp, C.POINTER(LrScheduleC), vp]
    L.pmgt_op_adamw_guarded.argtypes = [vp, vp, vp, vp, vp, i64, f, f, f, f, f, f, vp, vp, vp, C.POINTER(LrScheduleC), C.POINTER(StepGuardC), vp]
    L.pmgt_op_lr_schedule.argtypes = [C.POINTER(LrScheduleC), f, i64, i, vp, vp]
    L.pmgt_op_sgd.argtypes = [vp, vp, vp, i64, f, f, f, vp, vp, vp, C.POINTER(LrScheduleC), C.POINTER(StepGuardC), vp]
    L.pmgt_op_mirror.argtypes = [i, vp, vp, C.POINTER(MirrorDescC), i, i, vp]
    L.pmgt_op_nfr_generate.argtypes = [vp, i, i, i, f, f, vp, vp, vp, vp]
    L.pmgt_op_build_need_rows.argtypes = [i, i, i, vp, vp, vp, vp, vp, i64, vp]
    L.pmgt_op_dropout_keep.argtypes = [vp, f, u32, i, i, vp, vp]
    L.pmgt_eval_workspace_bytes.restype = i64
    L.pmgt_eval_workspace_bytes.argtypes = [i64]
    L.pmgt_eval_reset.argtypes = [vp, i64, vp]
    L.pmgt_eval_append.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, vp]
    L.pmgt_eval_reduce.argtypes = [vp, i64, i64, vp]
    L.pmgt_op_eval_append_scores.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, vp]
    L.pmgt_op_eval_small_max.argtypes = []
    L.pmgt_weight_average_update.argtypes = [vp, vp, i64, C.POINTER(AvgStepC), vp]
    L.pmgt_weight_swap.argtypes = [vp, vp, i64, vp]
    L.pmgt_rank_workspace_bytes.restype = i64
    L.pmgt_rank_workspace_bytes.argtypes = [i64, i]
    L.pmgt_rank_reset.argtypes = [vp, i64, vp, i, vp, vp, vp]
    L.pmgt_rank_append.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, vp]
    L.pmgt_rank_reduce.argtypes = [vp, i64, i64, vp]
    L.pmgt_ncf_score.argtypes = [C.POINTER(NcfHeadC), vp, vp, vp, i64, i64, vp, i64, vp]
    L.pmgt_topk_workspace_bytes.restype = i64
    L.pmgt_topk_workspace_bytes.argtypes = [i64, i64]
    L.pmgt_topk_rows.argtypes = [vp, i64, i64, i64, i, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]
    # (scores, row_stride, n, n_items, users, indptr, excluded, user_num, n_excluded, held_indptr, held_items, n_heldout, ranks, flags, stream)
    L.pmgt_rank_heldout.argtypes = [vp, i64, i64, i64, vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp]
    # (ranks, held_indptr, users, flags, n_users, user_num, n_heldout, ks, n_k, disc, idcg, records, header, stream)
    L.pmgt_rank_heldout_reduce.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, i, vp, vp, vp, vp, vp]
    L.pmgt_item_graph_default_slots.argtypes = []
    # (item_ptr, item_users, user_ptr, user_items, work, num_item, n_users, n_pairs, min_count, slots, deg_flags, max_count, scratch, scratch_rows, stream)
    L.pmgt_item_graph_count.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i, vp, vp, vp, i64, vp]
    # (... slots, deg_flags, row_ptr, node_of_item, total, indices, counts, scratch, scratch_rows, stream)
    L.pmgt_item_graph_fill.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i, vp, vp, vp, i64, vp, vp, vp, i64, vp]
    L.pmgt_item_sim_norms.argtypes = [vp, i64, i, f, vp, vp]      # (table, n_items, d, eps, inv_norm, stream)
    L.pmgt_item_sim_score.argtypes = [vp, vp, vp, i64, i64, i, vp, i64, vp]      # (table, inv_norm or NULL, queries, n, n_items, d, scores, row_stride, stream)
    # (table, inv_norm or NULL, hist_ptr, hist_items, users, n, user_num, n_items, d, agg, scores, row_stride, stream)
    L.pmgt_history_score.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i, i, vp, i64, vp]
    # (nbr, sim, idx_stride, m, hist_ptr, hist_items, hist_weights or NULL, users, n, user_num, n_items, scores, row_stride, stream)
    L.pmgt_knn_score.argtypes = [vp, vp, i64, i, vp, vp, vp, vp, i64, i64, i64, vp, i64, vp]
    L.pmgt_knn_score_tile.argtypes = []      # KNN_T of ops/knn_score.hip: the candidates of a tile
    L.pmgt_ncf_train_layout.restype = i64
    L.pmgt_ncf_train_layout.argtypes = [i, i, i, i64, i64, vp]
    L.pmgt_ncf_train_workspace_bytes.restype = i64
    L.pmgt_ncf_train_workspace_bytes.argtypes = [i, i, i, i64]
    L.pmgt_ncf_train_grad.argtypes = [C.POINTER(NcfTrainC), vp, vp, vp, i64, vp, vp, vp, i64, vp]
    L.pmgt_ncf_train_table_workspace_bytes.restype = i64
    L.pmgt_ncf_train_table_workspace_bytes.argtypes = [i, i, i, i64]
    L.pmgt_ncf_train_grad_table.argtypes = [C.POINTER(NcfTrainC), vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]      # (... logits, table_grad, workspace ...)
    L.pmgt_ncf_train_grad_dropout.argtypes = [C.POINTER(NcfTrainC), vp, vp, vp, i64, vp, vp, vp, C.POINTER(NcfDropoutC), vp, i64, vp]      # (... table_grad or NULL, drop ...)
    L.pmgt_ncf_train_rows_workspace_bytes.restype = i64
    L.pmgt_ncf_train_rows_workspace_bytes.argtypes = [i, i, i, i64]
    L.pmgt_ncf_train_grad_rows.argtypes = [C.POINTER(NcfTrainC), vp, vp, vp, i64, vp, vp, vp, vp, C.POINTER(NcfDropoutC), vp, i64, vp]      # (... logits, x_item, d_item, drop or NULL, workspace ...)
    L.pmgt_ncf_model_layout.restype = i64
    L.pmgt_ncf_model_layout.argtypes = [i, i, i, i, i, i64, i64, vp]
    L.pmgt_ncf_model_workspace_bytes.restype = i64
    L.pmgt_ncf_model_workspace_bytes.argtypes = [i, i, i, i, i, i64]
    L.pmgt_ncf_model_train_grad.argtypes = [C.POINTER(NcfModelC), vp, vp, vp, i64, vp, vp, C.POINTER(NcfDropoutC), vp, i64, vp]      # (... logits, drop or NULL, workspace ...)
    L.pmgt_ncf_model_score.argtypes = [C.POINTER(NcfModelHeadC), vp, vp, vp, i64, i64, vp, i64, vp]
    L.pmgt_op_adamw_segments.argtypes = [C.POINTER(AdamSegmentC), i, f, f, f, f, f, f, vp, vp, vp, vp]
    L.pmgt_op_step_segments.argtypes = [C.POINTER(AdamSegmentC), i, i, f, f, f, f, f, f, vp, vp, vp, C.POINTER(LrScheduleC),
                                        C.POINTER(StepGuardC), vp]      # (segments, count, optim = index in OPTIMS, ...)
    L.pmgt_op_cls_gather.argtypes = [i, vp, i64, i, i, vp, vp]
    L.pmgt_op_cls_scatter.argtypes = [i, vp, i64, i, i, vp, vp]
    L.pmgt_dcn_layout.restype = i64
    L.pmgt_dcn_layout.argtypes = [i, i, i, i, i64, i64, vp]
    L.pmgt_dcn_workspace_bytes.restype = i64
    L.pmgt_dcn_workspace_bytes.argtypes = [i, i, i, i, i64]
    L.pmgt_dcn_forward.argtypes = [C.POINTER(DcnHeadC), vp, vp, i64, vp, vp, i64, vp]
    L.pmgt_dcn_train_grad.argtypes = [C.POINTER(DcnHeadC), vp, vp, vp, i64, vp, vp, vp, i64, vp]
    L.pmgt_dcn_score_rows.argtypes = [C.POINTER(DcnHeadC), vp, i64, i, vp, vp]      # (head, table, rows, half, out, stream)
    L.pmgt_dcn_score.argtypes = [C.POINTER(DcnHeadC), vp, vp, vp, vp, vp, vp, i64, i64, vp, i64, vp]      # (head, pu, pi, user_rows, item_rows, consts, users, n, n_items, scores, row_stride, stream)
    L.pmgt_dcn_train_grad_dropout.argtypes = [C.POINTER(DcnHeadC), vp, vp, vp, i64, vp, vp, C.POINTER(DcnDropoutC), vp, i64, vp]      # (... logits or NULL, drop ...)
    _hip = L
    return L


class Ops:
    """The library as the per-kernel tests and profiling tools call it: every pmgt_op_* entry that takes a `path_opts` bit
    mask (include/pmgt_ops.h) gets it from `self.path` (an int, or option names through `use`), so call sites read as the
    kernel's own argument list.  Everything else passes straight through to the CDLL."""
    _BEFORE_STREAM = {"pmgt_op_gemm_nt", "pmgt_op_gemm_tn", "pmgt_op_gemm_tn_bias", "pmgt_op_linear", "pmgt_op_linear_ln_bwd", "pmgt_op_attention_fwd",
                      "pmgt_op_attention_bwd", "pmgt_op_linear_rows", "pmgt_op_gemm_tn_bias_rows"}
    _LAST = {"pmgt_op_gemm_tn_slab_elems"}

    def __init__(self, lib=None):
        self._L = lib if lib is not None else hip()
        self.path = 0

    def use(self, *names):
        """Select path options by name for the following calls (no names = the product path); returns self."""
        self.path = 0
        for n in names:
            self.path |= OPT[n]
        return self

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if name in Ops._BEFORE_STREAM:
            return lambda *a: fn(*a[:-1], self.path, a[-1])
        if name in Ops._LAST:
            return lambda *a: fn(*a, self.path)
        return fn


def ops():
    """A fresh Ops view of libpmgt_hip.so (path options start at 0)."""
    return Ops()


def stream():
    """The current torch stream as the `void* stream` argument of an entry."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc):
    if rc != 0:
        raise RuntimeError(f"pmgt HIP engine error {rc}: {hip().pmgt_last_error().decode()}")


def sampler():
    """libpmgt_sampler.so (host only) with argtypes set."""
    global _sampler
    if _sampler is not None:
        return _sampler
    L = _load(_build.sampler_lib_path(), "host sampler library")
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.pmgt_sampler_create.restype = vp
    L.pmgt_sampler_create.argtypes = [i64, vp, vp, vp, vp, i, i, i, i]
    L.pmgt_sampler_destroy.argtypes = [vp]
    L.pmgt_sampler_destroy.restype = None
    L.pmgt_sampler_last_error.restype = C.c_char_p
    L.pmgt_sampler_seed.argtypes = [vp, C.c_uint32]
    L.pmgt_sampler_seed.restype = None
    L.pmgt_sampler_context.argtypes = [vp, i64, vp, vp]
    L.pmgt_sampler_batch.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, vp]
    L.pmgt_sampler_batch_mt.argtypes = [vp, vp, i, i, C.c_uint64, C.c_uint64, C.c_uint64, i, vp, vp, vp, vp, vp, vp]
    L.pmgt_sampler_max_pairs.argtypes = [vp, i]
    L.pmgt_sampler_random_sample.restype = C.c_double
    L.pmgt_sampler_random_sample.argtypes = [vp]
    L.pmgt_sampler_randint.restype = i64
    L.pmgt_sampler_randint.argtypes = [vp, i64]
    L.pmgt_train_valid_split.argtypes = [i64, C.c_double, C.c_uint32, vp, vp]
    _sampler = L
    return L
